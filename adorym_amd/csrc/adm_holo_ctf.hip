// libadm -- the contrast-transfer-function forward model of multi-distance holography (SURVEY.md section 8 f1;
// adorym/forward_model.py:1011-1014, adorym/propagate.py:467-476, 590-606: modulate_and_get_ctf / pure_phase_ctf).
//
// One object slice, unknown_type 'delta_beta'; D = delta[:, :, 0] (real), n = ny nx, kappa = 10^lg_kappa:
//     xi_d   = PI lambda d (u^2 + v^2)
//     osc_d  = 2 (sin xi_d + cos xi_d / kappa)                         real, even in (u, v)
//     I_d    = 1 + Re IFFT2( osc_d FFT2(D) )
//     pred_d = sqrt(max(I_d, 0))
//     loss   = mean_{d,pixels} (pred_d - t_d)^2                        t_d = sqrt|data_d| (intensity data) or |data_d|
//     q_d    = (pred_d - t_d) / (pred_d n_dists n)  where I_d > 0, else 0
//     dL/dD  = Re IFFT2( sum_d osc_d FFT2(q_d) )                       (the operator is real and symmetric: its own adjoint)
//     dL/dbeta = 0                                                     (the model never reads beta)
//     dL/dlg_kappa = -(2 ln 10 / kappa) / n  sum_d Re sum_k conj(Q_d) cos xi_d F        Q_d = FFT2(q_d), F = FFT2(D)
//     dL/dd_d [per cm] = (2 PI lambda_nm 1e7 / n)  Re sum_k conj(Q_d) (cos xi_d - sin xi_d / kappa) (u^2 + v^2) F
// A pixel with I_d <= 0 predicts 0 and contributes to no gradient (the reference's autograd returns NaN everywhere then).
//
// The line machinery -- Stockham passes in LDS, LineGeo, the block-cooperative transposed stores, the LDS twiddle copy, the sums
// over a line -- is adm_line_fft.h, shared with adm_holo.hip and adm_ctf_invert.hip; its host setup is adm_line_host.h (DESIGN.md
// section 4).  Five launches per minibatch, like the Fresnel path:
//   C1  rows y      : D row (imag = 0)               -> FFT_x                                    -> T1[kx][y]
//   C2  lines kx    : FFT_y -> F (kept: Ft[kx][ky]) ; per d: x osc_d -> IFFT_y                   -> W[d][y][kx]
//   C3  rows (d, y) : IFFT_x / n -> I_d, pred_d, loss partial, q_d -> FFT_x                      -> T3[d][kx][y]
//   C4  lines kx    : per d: FFT_y -> Q_d ; kappa partial += Re conj(Q_d) cos xi_d F ; G += osc_d Q_d ; IFFT_y -> T4[kx][y]
//                     with grad_dists: the line's sum of Re conj(Q_d) (cos xi_d - sin xi_d / kappa) (u^2 + v^2) F -> partd[d][kx]
//   C5  rows y      : IFFT_x / n -> dL/dD (+= or =) ; the loss and kappa sums of C3 / C4 in a fixed order, then the n_dists
//                     distance sums of C4
// A forward-only call stops after C3 and sums with ctf_sums_kernel.
//
// The distances come from the host (c[d] = fl32(PI lambda dist_nm_d): the reference's Python double, rounded once where it meets
// the float32 tensors) or, for a run that refines them, from a float32 device array in cm that the optimiser moves in place.  Then
//     c_d = fl32( fl32(PI lambda_nm) * fl32(dists_dev[d] * 1e7f) )
// as the reference's float32 run has it when free_prop_cm is a float32 tensor: dist_nm = free_prop_cm * 1e7 is a float32 product,
// and PI * lmbda_nm (a Python double) meets that 0-dim tensor as a float32 scalar (adorym/propagate.py:470, 598).
#include <vector>
#include <cmath>
#include <cstring>
#include "adm_ctf_group.h"
#include "adm_line_host.h"
#include "adm_line_fft.h"
#include "adm_ms_math.h"

#define ADM_CTF_MAX_DISTS 64

namespace adm {
namespace ctf {

using namespace linefft;

struct CtfArgs {
    const float2* obj;                              // [ny][nx] (delta, beta)
    const float *data, *uv2t, *lg_kappa;            // uv2t [nx][ny]
    float2 *T1, *Ft, *W, *T3, *T4;                  // T1 [nx][ny], Ft [nx][ny], W [nd][ny][nx], T3 [nd][nx][ny], T4 [nx][ny]
    const float2 *tw_x, *tw_y;
    float *pred, *part3;                            // part3 [nd][ny]
    double* part4;                                  // [nx]
    float2* grad_obj;
    float *grad_lg_kappa, *loss_sum;
    int ny, nx, nd, intensity, set_obj;
    float inv_n, qscale;                            // 1 / n;  1 / (n_dists n)
    float c[ADM_CTF_MAX_DISTS];                     // fl32(PI lambda dist_nm_d): rounded once on the host, like the reference's Python double
    const float* dists_dev;                         // [nd] cm, or NULL: the distances are c[]
    float pil;                                      // fl32(PI lambda_nm)
    double* partd;                                  // [nd][nx]
    float* grad_dists;                              // [nd] or NULL
    double dscale;                                  // 2 PI lambda_nm 1e7 / n
};

// c_d of distance d: the host's, or formed from the device array with the reference's float32 roundings (head comment)
__device__ __forceinline__ float ctf_c_of(const CtfArgs& A, int d) {
    return A.dists_dev ? mul_rounded(A.pil, mul_rounded(A.dists_dev[d], 1e7f)) : A.c[d];
}

// 1 / kappa = 10^-lg_kappa, formed in double and rounded once (the reference keeps ctf_lg_kappa in float64)
__device__ __forceinline__ double inv_kappa_f64(const float* lg_kappa) { return exp(-2.302585092994045684 * (double)lg_kappa[0]); }

// ... by ONE thread of the block, handed over through LDS (the caller's next barrier orders it): a double exp per thread of C2 / C4
// was work repeated 256 times
__device__ __forceinline__ void stage_inv_kappa(float* slot, const float* lg_kappa) {
    if (threadIdx.x == 0) *slot = (float)inv_kappa_f64(lg_kappa);
}

// sine and cosine of xi_d = c_d (u^2 + v^2), the product in fp32 like the reference's tensors
__device__ __forceinline__ void ctf_sincos(float uv2, float c, float& sn, float& cs) { sincos_fast(c * uv2, sn, cs); }
__device__ __forceinline__ float ctf_osc(float sn, float cs, float inv_kappa) { return 2.f * (sn + inv_kappa * cs); }

template <int NX> __global__ __launch_bounds__(256) void ctf_c1(CtfArgs A) {
    using LG = LineGeo<NX>;
    __shared__ cf buf[2][LG::LPB * LG::LP];
    __shared__ float2 twl[TwLds<NX>::SIZE];
    const float2* tw = stage_twiddles<NX>(twl, A.tw_x);
    const int ll = threadIdx.x / LG::TPR, t = threadIdx.x % LG::TPR;
    const int y0 = blockIdx.x * LG::LPB, y = y0 + ll;
    const bool ok = y < A.ny;
    cf* a = buf[0] + ll * LG::LP;
    cf* b = buf[1] + ll * LG::LP;
    for (int x = t; x < NX; x += LG::TPR) a[x] = make_float2(ok ? A.obj[(size_t)y * NX + x].x : 0.f, 0.f);
    __syncthreads();
    const cf* res = line_fft<NX, false>(a, b, tw, t);
    float2* T1 = A.T1;
    const int ny = A.ny;
    store_lines_transposed<NX>(res - ll * LG::LP, min(LG::LPB, ny - y0), [=](int k, int c) { return T1 + (size_t)k * ny + y0 + c; });
}

// LPB adjacent lines kx per block, one distance per blockIdx.y (the forward transform of a line is repeated for every distance:
// cheaper than a kernel boundary); blockIdx.y == 0 keeps F
template <int NY> __global__ __launch_bounds__(256) void ctf_c2(CtfArgs A) {
    using LG = LineGeo<NY>;
    __shared__ cf buf[2][LG::LPB * LG::LP];
    __shared__ float2 twl[TwLds<NY>::SIZE];
    const float2* tw = stage_twiddles<NY>(twl, A.tw_y);
    const int ll = threadIdx.x / LG::TPR, t = threadIdx.x % LG::TPR;
    const int kx0 = blockIdx.x * LG::LPB, kx = kx0 + ll, d = blockIdx.y;
    const bool ok = kx < A.nx;
    cf* a = buf[0] + ll * LG::LP;
    cf* b = buf[1] + ll * LG::LP;
    for (int j = t; j < NY; j += LG::TPR) a[j] = ok ? A.T1[(size_t)kx * NY + j] : make_float2(0.f, 0.f);
    __shared__ float ik_s;
    stage_inv_kappa(&ik_s, A.lg_kappa);
    __syncthreads();
    const float ik = ik_s;
    cf* F = line_fft<NY, false>(a, b, tw, t);
    cf* p = (F == a) ? b : a;
    if (ok && d == 0)
        for (int k = t; k < NY; k += LG::TPR) A.Ft[(size_t)kx * NY + k] = F[k];
    const float c = ctf_c_of(A, d);
    for (int k = t; k < NY; k += LG::TPR) {
        float sn = 0.f, cs = 0.f;
        if (ok) ctf_sincos(A.uv2t[(size_t)kx * NY + k], c, sn, cs);
        p[k] = ok ? cscale(F[k], ctf_osc(sn, cs, ik)) : make_float2(0.f, 0.f);
    }
    line_sync<LG::TPR>();
    const cf* res = line_fft<NY, true>(p, F, tw, t);      // (F's buffer is free once p is filled)
    float2* W = A.W + (size_t)d * NY * A.nx;
    const int nx = A.nx;
    store_lines_transposed<NY>(res - ll * LG::LP, min(LG::LPB, nx - kx0), [=](int y, int cc) { return W + (size_t)y * nx + kx0 + cc; });
}

template <int NX, bool GRAD> __global__ __launch_bounds__(256) void ctf_c3(CtfArgs A) {
    using LG = LineGeo<NX>;
    __shared__ cf buf[2][LG::LPB * LG::LP];
    __shared__ float red[256];
    __shared__ float2 twl[TwLds<NX>::SIZE];
    const float2* tw = stage_twiddles<NX>(twl, A.tw_x);
    const int ll = threadIdx.x / LG::TPR, t = threadIdx.x % LG::TPR;
    const int job0 = blockIdx.x * LG::LPB, job = job0 + ll;        // job = d * ny + y
    const int ny = A.ny;
    const bool ok = job < A.nd * ny;
    const size_t row = (size_t)(ok ? job : 0) * NX;                // rows (d, y) of W, data and pred are contiguous in job
    cf* a = buf[0] + ll * LG::LP;
    cf* b = buf[1] + ll * LG::LP;
    // the measured row does not depend on the transform: requested ahead of it
    constexpr int PPT = NX / LG::TPR;
    float meas[PPT];
#pragma unroll
    for (int j = 0; j < PPT; ++j) meas[j] = A.data[row + t + j * LG::TPR];
    for (int k = t; k < NX; k += LG::TPR) a[k] = ok ? A.W[row + k] : make_float2(0.f, 0.f);
    __syncthreads();
    cf* res = line_fft<NX, true>(a, b, tw, t);
    cf* oth = (res == a) ? b : a;
    float lsum = 0.f;
#pragma unroll
    for (int j = 0; j < PPT; ++j) {
        const int x = t + j * LG::TPR;
        const float as = fabsf(meas[j]);
        const float tgt = A.intensity ? sqrtf(as) : as;
        const float I = 1.f + res[x].x * A.inv_n;
        const float pr = (I > 0.f) ? sqrtf(I) : 0.f;
        const float diff = pr - tgt;
        if (ok) {
            lsum += diff * diff;
            if (A.pred) A.pred[row + x] = pr;
        }
        if (GRAD) oth[x] = make_float2((ok && I > 0.f) ? A.qscale * diff / pr : 0.f, 0.f);
    }
    const float ls = line_sum<LG::TPR, float>(lsum, red);
    if (ok && t == 0) A.part3[job] = ls;
    if (!GRAD) return;
    line_sync<LG::TPR>();
    const cf* G = line_fft<NX, false>(oth, res, tw, t);
    float2* T3 = A.T3;
    store_lines_transposed<NX>(G - ll * LG::LP, min(LG::LPB, A.nd * ny - job0), [=](int k, int c) {
        const int j = job0 + c, dd = j / ny, yy = j % ny;          // (the lines of a block may belong to different distances when ny < LPB)
        return T3 + (size_t)dd * NX * ny + (size_t)k * ny + yy;
    });
}

// C4's rounds over the distances: slot ll owns distance d0 + ll in round d0.  Returns the thread's terms of the kappa gradient.
// GD: the distance gradient as well, as a code path of its own: a launch without grad_dists executes the instructions it executed
// before the distances became parameters.  Both instantiations live in the one kernel, so that launch runs with the larger register
// allocation too, and the split had no measured effect on the group's time (DESIGN.md sections 4 and 5).
template <int NY, bool GD>
__device__ __forceinline__ double ctf_c4_rounds(const CtfArgs& A, cf* a, cf* b, cf* GF, const float2* tw, double* redd, const float* ik_s,
                                                int ll, int t, int kx) {
    using LG = LineGeo<NY>;
    // the kappa gradient is a sum of O(n_dists n) terms of mixed sign: every thread adds its terms in double
    double kacc = 0.0;
    for (int d0 = 0; d0 < A.nd; d0 += LG::LPB) {
        const int d = d0 + ll;
        const bool ok = d < A.nd;
        for (int j = t; j < NY; j += LG::TPR) a[j] = ok ? A.T3[((size_t)d * A.nx + kx) * NY + j] : make_float2(0.f, 0.f);
        if (d0 == 0) __syncthreads();                 // (also orders the twiddle copy of stage_twiddles and 1 / kappa before the first pass)
        else line_sync<LG::TPR>();
        const float ik = *ik_s;
        const cf* Q = line_fft<NY, false>(a, b, tw, t);
        const float c = ok ? ctf_c_of(A, d) : 0.f;
        double dacc = 0.0;                            // this round's distance: the thread's terms of dL/dd_d, in double like kacc
        if (ok)
            for (int k = t; k < NY; k += LG::TPR) {
                const size_t e = (size_t)kx * NY + k;
                float sn, cs;
                const float uv2 = A.uv2t[e];
                ctf_sincos(uv2, c, sn, cs);
                const cf q = Q[k];
                GF[k] = caxpy(GF[k], ctf_osc(sn, cs, ik), q);
                if (A.grad_lg_kappa) {
                    const cf f = A.Ft[e];
                    kacc += (double)(cs * (q.x * f.x + q.y * f.y));         // Re( conj(Q) cos xi F )
                }
                if (GD) {
                    const cf f = A.Ft[e];
                    dacc += (double)((cs - ik * sn) * uv2) * (double)(q.x * f.x + q.y * f.y);
                }
            }
        if (GD) {
            // the line's TPR sums in a fixed tree: one partial per (d, kx); an idle slot writes nothing
            const double s = line_sum<LG::TPR, double>(dacc, redd);
            if (ok && t == 0) A.partd[(size_t)d * A.nx + kx] = s;
        }
        line_sync<LG::TPR>();                         // a / b are refilled by the next round of distances
    }
    return kacc;
}

// One line kx per block; slot s of the block works on distances s, s + LPB, ...  Q_d = FFT_y(T3_d) is the unnormalised FFT2(q_d).
template <int NY> __global__ __launch_bounds__(256) void ctf_c4(CtfArgs A) {
    using LG = LineGeo<NY>;
    static_assert(3 * LG::LPB * LG::LP * sizeof(cf) + 256 * sizeof(double) + TwLds<NY>::SIZE * sizeof(float2) + 16 <= 64 * 1024,
                  "ctf_c4: three line buffers + reduction scratch + twiddle copy must fit the 64 KB a workgroup may allocate");
    __shared__ cf buf[3][LG::LPB * LG::LP];
    __shared__ double redd[256];
    __shared__ float2 twl[TwLds<NY>::SIZE];
    const float2* tw = stage_twiddles<NY>(twl, A.tw_y);
    const int ll = threadIdx.x / LG::TPR, t = threadIdx.x % LG::TPR;
    const int kx = blockIdx.x;
    cf* a = buf[0] + ll * LG::LP;
    cf* b = buf[1] + ll * LG::LP;
    cf* GF = buf[2] + ll * LG::LP;
    __shared__ float ik_s;
    stage_inv_kappa(&ik_s, A.lg_kappa);
    for (int k = t; k < NY; k += LG::TPR) GF[k] = make_float2(0.f, 0.f);
    const double kacc = A.grad_dists ? ctf_c4_rounds<NY, true>(A, a, b, GF, tw, redd, &ik_s, ll, t, kx)
                                     : ctf_c4_rounds<NY, false>(A, a, b, GF, tw, redd, &ik_s, ll, t, kx);
    __syncthreads();                                  // every slot's GF is complete
    if (A.grad_lg_kappa) {
        // the 256 threads' sums in a fixed tree: one slot per line kx
        redd[threadIdx.x] = kacc;
        __syncthreads();
#pragma unroll
        for (int s = 128; s > 0; s >>= 1) {
            if ((int)threadIdx.x < s) redd[threadIdx.x] += redd[threadIdx.x + s];
            __syncthreads();
        }
        if (threadIdx.x == 0) A.part4[kx] = redd[0];
    }
    // the slots' sums over their distances, added in slot order into slot 0, which transforms back
    if (LG::LPB > 1) {
        for (int k = threadIdx.x; k < NY; k += 256) {
            cf sum = buf[2][k];
#pragma unroll
            for (int s_ = 1; s_ < LG::LPB; ++s_) sum = cadd(sum, buf[2][s_ * LG::LP + k]);
            buf[2][k] = sum;
        }
        __syncthreads();
    }
    const cf* gy = line_fft<NY, true>(GF, a, tw, t);      // (every slot runs it on its own buffers; slot 0's counts)
    if (ll == 0)
        for (int y = t; y < NY; y += LG::TPR) A.T4[(size_t)kx * NY + y] = gy[y];
}

// the per-line sums of C3 / C4 in a fixed order, one wave per output: o < nd: loss_sum[o] =; o == nd: grad_lg_kappa (+)=
__device__ __forceinline__ void ctf_sum_one(const CtfArgs& A, bool grad, int o) {      // called by one whole wave
    const int lane = threadIdx.x & 63;
    if (o < A.nd) {
        float s = 0.f;
        for (int y = lane; y < A.ny; y += 64) s += A.part3[(size_t)o * A.ny + y];
#pragma unroll
        for (int off = 32; off > 0; off >>= 1) s += __shfl_down(s, off, 64);
        if (lane == 0) A.loss_sum[o] = s;
        return;
    }
    if (!grad || !A.grad_lg_kappa) return;
    double s = 0.0;
    for (int x = lane; x < A.nx; x += 64) s += A.part4[x];
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) s += __shfl_down(s, off, 64);
    if (lane == 0) {
        // -(2 ln 10 / kappa) / n in double, one rounding
        const float g = (float)(-2.0 * 2.302585092994045684 * inv_kappa_f64(A.lg_kappa) * (double)A.inv_n * s);
        A.grad_lg_kappa[0] = (A.set_obj ? 0.f : A.grad_lg_kappa[0]) + g;
    }
}
// dL/dd_o from C4's per-line sums, by one whole wave: (2 PI lambda_nm 1e7 / n) x the sum, in double, one rounding
__device__ __forceinline__ void ctf_sum_dist(const CtfArgs& A, int o) {
    const int lane = threadIdx.x & 63;
    double s = 0.0;
    for (int x = lane; x < A.nx; x += 64) s += A.partd[(size_t)o * A.nx + x];
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) s += __shfl_down(s, off, 64);
    if (lane == 0) {
        const float g = (float)(A.dscale * s);
        A.grad_dists[o] = (A.set_obj ? 0.f : A.grad_dists[o]) + g;
    }
}
__global__ __launch_bounds__(64) void ctf_sums_kernel(CtfArgs A) { ctf_sum_one(A, false, blockIdx.x); }

template <int NX> __global__ __launch_bounds__(256) void ctf_c5(CtfArgs A) {
    using LG = LineGeo<NX>;
    __shared__ cf buf[2][LG::LPB * LG::LP];
    __shared__ float2 twl[TwLds<NX>::SIZE];
    const float2* tw = stage_twiddles<NX>(twl, A.tw_x);
    const int ll = threadIdx.x / LG::TPR, t = threadIdx.x % LG::TPR;
    const int y0 = blockIdx.x * LG::LPB, y = y0 + ll;
    const bool ok = y < A.ny;
    cf* a = buf[0] + ll * LG::LP;
    cf* b = buf[1] + ll * LG::LP;
    // the gradient's old values (+= mode) are requested before the line is fetched and transformed
    constexpr int PPT = NX / LG::TPR;
    float2 old[PPT];
#pragma unroll
    for (int j = 0; j < PPT; ++j)
        old[j] = (A.set_obj || !ok) ? make_float2(0.f, 0.f) : A.grad_obj[(size_t)y * NX + t + j * LG::TPR];
    // T4[kx][y]: thread e fetches column e / LPB of row e % LPB, so LPB consecutive lanes read LPB * 8 contiguous bytes
    {
        const int ny = A.ny;
        for (int e = threadIdx.x; e < NX * LG::LPB; e += 256) {
            const int c = e % LG::LPB, k = e / LG::LPB;
            buf[0][c * LG::LP + k] = (y0 + c < ny) ? A.T4[(size_t)k * ny + y0 + c] : make_float2(0.f, 0.f);
        }
    }
    __syncthreads();
    const cf* res = line_fft<NX, true>(a, b, tw, t);
    if (ok)
#pragma unroll
        for (int j = 0; j < PPT; ++j) {
            const int x = t + j * LG::TPR;
            float2 go = old[j];                          // (the beta channel: its old bits, or +0 when overwriting)
            go.x = go.x + mul_rounded(res[x].x, A.inv_n);
            A.grad_obj[(size_t)y * NX + x] = go;
        }
    // the sums of C3 / C4: output o by wave 0 of block o % gridDim.x
    if (threadIdx.x < 64) {
        for (int o = blockIdx.x; o <= A.nd; o += gridDim.x) ctf_sum_one(A, true, o);
        if (A.grad_dists)
            for (int o = blockIdx.x; o < A.nd; o += gridDim.x) ctf_sum_dist(A, o);
    }
}

static hipError_t ctf_run(const CtfArgs& A, bool want_grad, hipStream_t st) {
#define C1(N_) case N_: hipLaunchKernelGGL((ctf_c1<N_>), dim3(blocks_for<N_>(A.ny)), dim3(256), 0, st, A); break;
#define C2(N_) case N_: hipLaunchKernelGGL((ctf_c2<N_>), dim3(blocks_for<N_>(A.nx), A.nd), dim3(256), 0, st, A); break;
#define C3G(N_) case N_: hipLaunchKernelGGL((ctf_c3<N_, true>), dim3(blocks_for<N_>(A.nd * A.ny)), dim3(256), 0, st, A); break;
#define C3N(N_) case N_: hipLaunchKernelGGL((ctf_c3<N_, false>), dim3(blocks_for<N_>(A.nd * A.ny)), dim3(256), 0, st, A); break;
#define C4(N_) case N_: hipLaunchKernelGGL((ctf_c4<N_>), dim3(A.nx), dim3(256), 0, st, A); break;
#define C5(N_) case N_: hipLaunchKernelGGL((ctf_c5<N_>), dim3(blocks_for<N_>(A.ny)), dim3(256), 0, st, A); break;
    switch (A.nx) { ADM_LINE_SIZES(C1) default: return hipErrorInvalidValue; }
    switch (A.ny) { ADM_LINE_SIZES(C2) default: return hipErrorInvalidValue; }
    if (want_grad) {
        switch (A.nx) { ADM_LINE_SIZES(C3G) default: return hipErrorInvalidValue; }
        switch (A.ny) { ADM_LINE_SIZES(C4) default: return hipErrorInvalidValue; }
        switch (A.nx) { ADM_LINE_SIZES(C5) default: return hipErrorInvalidValue; }
    } else {
        switch (A.nx) { ADM_LINE_SIZES(C3N) default: return hipErrorInvalidValue; }
        hipLaunchKernelGGL(ctf_sums_kernel, dim3(A.nd), dim3(64), 0, st, A);
    }
#undef C1
#undef C2
#undef C3G
#undef C3N
#undef C4
#undef C5
    return hipGetLastError();
}

}  // namespace ctf
}  // namespace adm

using namespace adm;

extern "C" int adm_ctf_create(adm_ctx* ctx, const adm_ctf_desc* desc, adm_ctf** out) {
    if (!ctx || !desc || !out) return fail(ADM_ERR_INVALID, "adm_ctf_create: null argument");
    const adm_ctf_desc& d = *desc;
    if (!line_side_ok(d.ny) || !line_side_ok(d.nx))
        return fail(ADM_ERR_UNSUPPORTED, "adm_ctf_create: field sizes must be powers of two in [16, 2048]");
    if (d.n_dists < 1 || d.n_dists > ADM_CTF_MAX_DISTS) return fail(ADM_ERR_UNSUPPORTED, "adm_ctf_create: n_dists must be in [1, 64]");
    if (!(d.energy_ev > 0.0) || !(d.psize_cm > 0.0)) return fail(ADM_ERR_INVALID, "adm_ctf_create: energy_ev and psize_cm must be positive");
    adm_ctf* h = new adm_ctf();
    std::memset(h, 0, sizeof(*h));
    h->ctx = ctx;
    h->d = d;
    const size_t n = (size_t)d.ny * d.nx;
    const double voxel_nm = d.psize_cm * 1e7;
    int rc = line_upload_twiddles(ctx, d.ny, &h->tw_y);
    if (!rc) rc = line_upload_twiddles(ctx, d.nx, &h->tw_x);
    if (!rc) rc = line_upload_uv2t(ctx, d.ny, d.nx, voxel_nm, voxel_nm, &h->uv2t);
    if (!rc) rc = adm_malloc(ctx, n * sizeof(float2), (void**)&h->T14);
    if (!rc) rc = adm_malloc(ctx, n * sizeof(float2), (void**)&h->Ft);
    if (!rc) rc = adm_malloc(ctx, n * d.n_dists * sizeof(float2), (void**)&h->W);
    if (!rc) rc = adm_malloc(ctx, n * d.n_dists * sizeof(float2), (void**)&h->T3);
    if (!rc) rc = adm_malloc(ctx, (size_t)d.n_dists * d.ny * sizeof(float), (void**)&h->part3);
    if (!rc) rc = adm_malloc(ctx, (size_t)d.nx * sizeof(double), (void**)&h->part4);
    if (!rc) rc = adm_malloc(ctx, (size_t)d.n_dists * sizeof(float), (void**)&h->loss_scratch);
    if (rc) {
        adm_ctf_destroy(h);
        return rc;
    }
    *out = h;
    return ADM_OK;
}

extern "C" int adm_ctf_destroy(adm_ctf* h) {
    if (!h) return ADM_OK;
    void* bufs[] = {h->tw_y, h->tw_x, h->uv2t, h->T14, h->Ft, h->W, h->T3, h->part3, h->part4, h->loss_scratch, h->partd};
    for (void* b : bufs)
        if (b) adm_free(h->ctx, b);
    delete h;
    return ADM_OK;
}

int adm::ctf::group_run(adm_ctf* h, const char* who, const float* obj, const double* dists_cm, const float* dists_dev, const float* lg_kappa,
                        const float* data, int want_grad, float* grad_obj, float* grad_lg_kappa, float* grad_dists, float* pred, float* loss_sum) {
    if (!h || !obj || (!dists_cm && !dists_dev) || !lg_kappa || !data) return fail(ADM_ERR_INVALID, std::string(who) + ": null argument");
    if (want_grad < 0 || want_grad > 2) return fail(ADM_ERR_INVALID, std::string(who) + ": want_grad must be 0, 1 or 2");
    if (want_grad && !grad_obj) return fail(ADM_ERR_INVALID, std::string(who) + ": want_grad needs grad_obj");
    const adm_ctf_desc& d = h->d;
    const size_t n = (size_t)d.ny * d.nx;
    ctf::CtfArgs A;
    std::memset(&A, 0, sizeof(A));
    A.obj = (const float2*)obj; A.data = data; A.uv2t = h->uv2t; A.lg_kappa = lg_kappa;
    A.T1 = h->T14; A.Ft = h->Ft; A.W = h->W; A.T3 = h->T3; A.T4 = h->T14;
    A.tw_x = h->tw_x; A.tw_y = h->tw_y;
    A.pred = pred; A.part3 = h->part3; A.part4 = h->part4;
    A.grad_obj = (float2*)grad_obj;
    A.grad_lg_kappa = want_grad ? grad_lg_kappa : nullptr;
    A.grad_dists = want_grad ? grad_dists : nullptr;
    A.partd = h->partd;
    if (A.grad_dists && !A.partd) return fail(ADM_ERR_INVALID, std::string(who) + ": grad_dists without the partial sums' buffer");
    A.loss_sum = loss_sum ? loss_sum : h->loss_scratch;
    A.ny = d.ny; A.nx = d.nx; A.nd = d.n_dists; A.intensity = d.raw_intensity;
    A.set_obj = (want_grad == 2) ? 1 : 0;
    A.inv_n = (float)(1.0 / (double)n);
    A.qscale = (float)(1.0 / ((double)n * d.n_dists));
    const double lambda_nm = 1240.0 / d.energy_ev;
    A.dists_dev = dists_dev;
    A.pil = (float)(3.14159265359 * lambda_nm);
    A.dscale = 2.0 * 3.14159265359 * lambda_nm * 1e7 / (double)n;
    if (!dists_dev)
        for (int i = 0; i < d.n_dists; ++i) A.c[i] = (float)(3.14159265359 * lambda_nm * (dists_cm[i] * 1e7));
    ADM_HIP(ctf::ctf_run(A, want_grad != 0, h->ctx->stream));
    return ADM_OK;
}

extern "C" int adm_ctf_fwd_adj(adm_ctf* h, const float* obj, const double* dists_cm, const float* lg_kappa, const float* data,
                               int want_grad, float* grad_obj, float* grad_lg_kappa, float* pred, float* loss_sum) {
    if (!dists_cm) return fail(ADM_ERR_INVALID, "adm_ctf_fwd_adj: null argument");
    return ctf::group_run(h, "adm_ctf_fwd_adj", obj, dists_cm, nullptr, lg_kappa, data, want_grad, grad_obj, grad_lg_kappa, nullptr, pred, loss_sum);
}
