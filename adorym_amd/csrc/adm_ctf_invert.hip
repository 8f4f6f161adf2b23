// libadm -- the direct inversion of the contrast-transfer-function model of multi-distance holography
// (update_using_external_algorithm='ctf': adorym/array_ops.py:274-286, adorym/conventional.py:112-152, multidistance_ctf_wrapped).
//
// D holograms I_d of one angle, kappa = 10^lg_kappa, alpha > 0 the regulariser (the reference's 1e-10, or a table per frequency):
//     xi_d  = PI lambda d (u^2 + v^2)
//     w_d   = sin xi_d + cos xi_d / kappa                              real, even in (u, v)
//     phase = Re IFFT2( sum_d w_d FFT2(I_d - 1) / (sum_d 2 w_d^2 + alpha) )
// The data are used as given, no sqrt, no loss.  A batch of angles goes through one launch group.
//
// The line machinery is adm_line_fft.h, its host setup adm_line_host.h (both shared with adm_holo.hip and adm_holo_ctf.hip).  Three
// launches per call, no atomics:
//   I1  rows (b, d, y) : I_d row - 1 (imag = 0)   -> FFT_x                                              -> T1[b][d][kx][y]
//   I2  lines (b, kx)  : per d: FFT_y -> F_d ; num += w_d F_d ; den += 2 w_d^2  (registers) ;
//                        A = num / (den + alpha)  -> IFFT_y                                             -> T2[b][y][kx]
//   I3  rows (b, y)    : IFFT_x / n -> real part                                                        -> out
// Every sum runs in a fixed order inside one thread: two calls give the same bits.
#include <vector>
#include <cmath>
#include <cstring>
#include "adm_line_host.h"
#include "adm_line_fft.h"
#include "adm_ms_math.h"

#define ADM_CTFINV_MAX_DISTS 64

struct adm_ctfinv {
    adm_ctx* ctx;
    adm_ctfinv_desc d;
    float2 *tw_y, *tw_x;      // exp(-2 pi i j / N) for N = ny, nx
    float* uv2t;              // [nx][ny]: u^2 + v^2 (nm^-2) of frequency (ky, kx) at [kx][ky], fp32 like the reference's tensors
    float* alpha_t;           // [nx][ny]: the regulariser of frequency (ky, kx) at [kx][ky]
    float2 *T1, *T2;          // T1 [max_batch][n_dists][nx][ny], T2 [max_batch][ny][nx]
};

namespace adm {
namespace ctfinv {

using namespace linefft;

struct InvArgs {
    const float *data, *uv2t, *alpha_t, *lg_kappa;  // data [nb][nd][ny][nx]; uv2t, alpha_t [nx][ny]
    float2 *T1, *T2;                                // T1 [nb][nd][nx][ny], T2 [nb][ny][nx]
    const float2 *tw_x, *tw_y;
    float* out;
    int ny, nx, nd, nb, out_stride;
    float inv_n;                                    // 1 / (ny nx)
    float c[ADM_CTFINV_MAX_DISTS];                  // fl32(PI lambda dist_nm_d): rounded once on the host, like the reference's Python double
};

// 1 / kappa = 10^-lg_kappa, formed in double and rounded once, by ONE thread of the block and handed over through LDS (the caller's
// next barrier orders it)
__device__ __forceinline__ void stage_inv_kappa(float* slot, const float* lg_kappa) {
    if (threadIdx.x == 0) *slot = (float)exp(-2.302585092994045684 * (double)lg_kappa[0]);
}

template <int NX> __global__ __launch_bounds__(256) void ctfinv_i1(InvArgs A) {
    using LG = LineGeo<NX>;
    __shared__ cf buf[2][LG::LPB * LG::LP];
    __shared__ float2 twl[TwLds<NX>::SIZE];
    const float2* tw = stage_twiddles<NX>(twl, A.tw_x);
    const int ll = threadIdx.x / LG::TPR, t = threadIdx.x % LG::TPR;
    const int job0 = blockIdx.x * LG::LPB, job = job0 + ll;        // job = b * nd * ny + d * ny + y
    const int ny = A.ny, n_jobs = A.nb * A.nd * ny;
    const bool ok = job < n_jobs;
    const size_t row = (size_t)(ok ? job : 0) * NX;                // rows (b, d, y) of the data are contiguous in job
    cf* a = buf[0] + ll * LG::LP;
    cf* b = buf[1] + ll * LG::LP;
    for (int x = t; x < NX; x += LG::TPR) a[x] = make_float2(ok ? A.data[row + x] - 1.f : 0.f, 0.f);
    __syncthreads();
    const cf* res = line_fft<NX, false>(a, b, tw, t);
    float2* T1 = A.T1;
    store_lines_transposed<NX>(res - ll * LG::LP, min(LG::LPB, n_jobs - job0), [=](int k, int c) {
        const int j = job0 + c, bd = j / ny, yy = j % ny;          // (the lines of a block may belong to different distances and batch entries)
        return T1 + (size_t)bd * NX * ny + (size_t)k * ny + yy;
    });
}

// LPB adjacent lines kx of batch entry blockIdx.y per block.  Thread t of a line keeps points k = t + j TPR, j < 8, of the
// numerator and the denominator in registers over the loop of distances.
template <int NY> __global__ __launch_bounds__(256) void ctfinv_i2(InvArgs A) {
    using LG = LineGeo<NY>;
    constexpr int PPT = NY / LG::TPR;
    __shared__ cf buf[2][LG::LPB * LG::LP];
    __shared__ float2 twl[TwLds<NY>::SIZE];
    __shared__ float ik_s;
    const float2* tw = stage_twiddles<NY>(twl, A.tw_y);
    stage_inv_kappa(&ik_s, A.lg_kappa);
    const int ll = threadIdx.x / LG::TPR, t = threadIdx.x % LG::TPR;
    const int kx0 = blockIdx.x * LG::LPB, kx = kx0 + ll, bb = blockIdx.y;
    const int nx = A.nx, nd = A.nd;
    const bool ok = kx < nx;
    cf* a = buf[0] + ll * LG::LP;
    cf* b = buf[1] + ll * LG::LP;
    const size_t line = (size_t)(ok ? kx : 0) * NY;
    const float2* src = A.T1 + (size_t)bb * nd * nx * NY + line;   // distance d: + d * nx * NY
    float uv[PPT], al[PPT], den[PPT];
    cf num[PPT], nxt[PPT];
#pragma unroll
    for (int j = 0; j < PPT; ++j) {
        const int k = t + j * LG::TPR;
        nxt[j] = ok ? src[k] : make_float2(0.f, 0.f);
        uv[j] = A.uv2t[line + k];
        al[j] = A.alpha_t[line + k];
        num[j] = make_float2(0.f, 0.f);
        den[j] = 0.f;
    }
    float ik = 0.f;
    for (int d = 0; d < nd; ++d) {
#pragma unroll
        for (int j = 0; j < PPT; ++j) a[t + j * LG::TPR] = nxt[j];
        // the line of distance d + 1 is requested before the transform of d
        if (d + 1 < nd) {
            const float2* s1 = src + (size_t)(d + 1) * nx * NY;
#pragma unroll
            for (int j = 0; j < PPT; ++j) nxt[j] = ok ? s1[t + j * LG::TPR] : make_float2(0.f, 0.f);
        }
        if (d == 0) {
            __syncthreads();                          // (also orders the twiddle copy of stage_twiddles and 1 / kappa before the first pass)
            ik = ik_s;
        } else {
            line_sync<LG::TPR>();
        }
        const cf* F = line_fft<NY, false>(a, b, tw, t);
        const float c = A.c[d];
#pragma unroll
        for (int j = 0; j < PPT; ++j) {
            float sn, cs;
            sincos_fast(c * uv[j], sn, cs);
            const float w = sn + ik * cs;
            num[j] = caxpy(num[j], w, F[t + j * LG::TPR]);
            den[j] = fmaf(2.f * w, w, den[j]);
        }
        line_sync<LG::TPR>();                         // a / b are refilled by the next distance (or by the quotient below)
    }
#pragma unroll
    for (int j = 0; j < PPT; ++j) {
        const float q = den[j] + al[j];
        a[t + j * LG::TPR] = make_float2(num[j].x / q, num[j].y / q);
    }
    line_sync<LG::TPR>();
    const cf* res = line_fft<NY, true>(a, b, tw, t);
    float2* T2 = A.T2 + (size_t)bb * NY * nx;
    store_lines_transposed<NY>(res - ll * LG::LP, min(LG::LPB, nx - kx0), [=](int y, int cc) { return T2 + (size_t)y * nx + kx0 + cc; });
}

template <int NX> __global__ __launch_bounds__(256) void ctfinv_i3(InvArgs A) {
    using LG = LineGeo<NX>;
    __shared__ cf buf[2][LG::LPB * LG::LP];
    __shared__ float2 twl[TwLds<NX>::SIZE];
    const float2* tw = stage_twiddles<NX>(twl, A.tw_x);
    const int ll = threadIdx.x / LG::TPR, t = threadIdx.x % LG::TPR;
    const int job = blockIdx.x * LG::LPB + ll;                     // job = b * ny + y
    const bool ok = job < A.nb * A.ny;
    const size_t row = (size_t)(ok ? job : 0) * NX;                // rows (b, y) of T2 and of the output are contiguous in job
    cf* a = buf[0] + ll * LG::LP;
    cf* b = buf[1] + ll * LG::LP;
    for (int k = t; k < NX; k += LG::TPR) a[k] = ok ? A.T2[row + k] : make_float2(0.f, 0.f);
    __syncthreads();
    const cf* res = line_fft<NX, true>(a, b, tw, t);
    if (ok)
        for (int x = t; x < NX; x += LG::TPR) A.out[(row + x) * A.out_stride] = res[x].x * A.inv_n;
}

static hipError_t ctfinv_run(const InvArgs& A, hipStream_t st) {
#define I1(N_) case N_: hipLaunchKernelGGL((ctfinv_i1<N_>), dim3(blocks_for<N_>(A.nb * A.nd * A.ny)), dim3(256), 0, st, A); break;
#define I2(N_) case N_: hipLaunchKernelGGL((ctfinv_i2<N_>), dim3(blocks_for<N_>(A.nx), A.nb), dim3(256), 0, st, A); break;
#define I3(N_) case N_: hipLaunchKernelGGL((ctfinv_i3<N_>), dim3(blocks_for<N_>(A.nb * A.ny)), dim3(256), 0, st, A); break;
    switch (A.nx) { ADM_LINE_SIZES(I1) default: return hipErrorInvalidValue; }
    switch (A.ny) { ADM_LINE_SIZES(I2) default: return hipErrorInvalidValue; }
    switch (A.nx) { ADM_LINE_SIZES(I3) default: return hipErrorInvalidValue; }
#undef I1
#undef I2
#undef I3
    return hipGetLastError();
}

}  // namespace ctfinv
}  // namespace adm

using namespace adm;

extern "C" int adm_ctfinv_create(adm_ctx* ctx, const adm_ctfinv_desc* desc, const float* alpha_host, adm_ctfinv** out) {
    if (!ctx || !desc || !out) return fail(ADM_ERR_INVALID, "adm_ctfinv_create: null argument");
    const adm_ctfinv_desc& d = *desc;
    if (!line_side_ok(d.ny) || !line_side_ok(d.nx))
        return fail(ADM_ERR_UNSUPPORTED, "adm_ctfinv_create: field sizes must be powers of two in [16, 2048]");
    if (d.n_dists < 1 || d.n_dists > ADM_CTFINV_MAX_DISTS) return fail(ADM_ERR_INVALID, "adm_ctfinv_create: n_dists must be in [1, 64]");
    if (d.max_batch < 1) return fail(ADM_ERR_INVALID, "adm_ctfinv_create: max_batch must be at least 1");
    // the batch entry is I2's blockIdx.y, and I1's jobs (b, d, y) are counted in an int
    if (d.max_batch > 65535 || (size_t)d.max_batch * d.n_dists * d.ny > ((size_t)1 << 30))
        return fail(ADM_ERR_INVALID, "adm_ctfinv_create: max_batch must be at most 65535 and max_batch n_dists ny at most 2^30");
    if (!(d.energy_ev > 0.0) || !(d.psize_cm > 0.0)) return fail(ADM_ERR_INVALID, "adm_ctfinv_create: energy_ev and psize_cm must be positive");
    const size_t n = (size_t)d.ny * d.nx;
    // the regulariser, transposed to [kx][ky]
    std::vector<float> al(n, 1e-10f);
    if (alpha_host)
        for (int y = 0; y < d.ny; ++y)
            for (int x = 0; x < d.nx; ++x) {
                const float v = alpha_host[(size_t)y * d.nx + x];
                if (!std::isfinite(v) || !(v > 0.f)) return fail(ADM_ERR_INVALID, "adm_ctfinv_create: every alpha must be finite and > 0");
                al[(size_t)x * d.ny + y] = v;
            }
    adm_ctfinv* h = new adm_ctfinv();
    std::memset(h, 0, sizeof(*h));
    h->ctx = ctx;
    h->d = d;
    const double voxel_nm = d.psize_cm * 1e7;
    int rc = line_upload_twiddles(ctx, d.ny, &h->tw_y);
    if (!rc) rc = line_upload_twiddles(ctx, d.nx, &h->tw_x);
    if (!rc) rc = line_upload_uv2t(ctx, d.ny, d.nx, voxel_nm, voxel_nm, &h->uv2t);
    if (!rc) rc = adm_malloc(ctx, n * sizeof(float), (void**)&h->alpha_t);
    if (!rc) rc = adm_h2d(ctx, h->alpha_t, al.data(), n * sizeof(float));
    if (!rc) rc = adm_malloc(ctx, n * d.n_dists * d.max_batch * sizeof(float2), (void**)&h->T1);
    if (!rc) rc = adm_malloc(ctx, n * d.max_batch * sizeof(float2), (void**)&h->T2);
    if (rc) {
        adm_ctfinv_destroy(h);
        return rc;
    }
    *out = h;
    return ADM_OK;
}

extern "C" int adm_ctfinv_destroy(adm_ctfinv* h) {
    if (!h) return ADM_OK;
    void* bufs[] = {h->tw_y, h->tw_x, h->uv2t, h->alpha_t, h->T1, h->T2};
    for (void* b : bufs)
        if (b) adm_free(h->ctx, b);
    delete h;
    return ADM_OK;
}

extern "C" int adm_ctfinv_run(adm_ctfinv* h, const float* data, int n_batch, const double* dists_cm, const float* lg_kappa, float* out,
                              int out_stride) {
    if (!h || !data || !dists_cm || !lg_kappa || !out) return fail(ADM_ERR_INVALID, "adm_ctfinv_run: null argument");
    const adm_ctfinv_desc& d = h->d;
    if (n_batch < 1 || n_batch > d.max_batch) return fail(ADM_ERR_INVALID, "adm_ctfinv_run: n_batch must be in [1, max_batch]");
    if (out_stride != 1 && out_stride != 2) return fail(ADM_ERR_INVALID, "adm_ctfinv_run: out_stride must be 1 or 2");
    ctfinv::InvArgs A;
    std::memset(&A, 0, sizeof(A));
    A.data = data; A.uv2t = h->uv2t; A.alpha_t = h->alpha_t; A.lg_kappa = lg_kappa;
    A.T1 = h->T1; A.T2 = h->T2; A.tw_x = h->tw_x; A.tw_y = h->tw_y;
    A.out = out;
    A.ny = d.ny; A.nx = d.nx; A.nd = d.n_dists; A.nb = n_batch; A.out_stride = out_stride;
    A.inv_n = (float)(1.0 / ((double)d.ny * d.nx));
    const double lambda_nm = 1240.0 / d.energy_ev;
    for (int i = 0; i < d.n_dists; ++i) A.c[i] = (float)(3.14159265359 * lambda_nm * (dists_cm[i] * 1e7));
    ADM_HIP(ctfinv::ctfinv_run(A, h->ctx->stream));
    return ADM_OK;
}
