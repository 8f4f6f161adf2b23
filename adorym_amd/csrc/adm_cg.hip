// Conjugate-gradient object optimiser (CGOptimizer.apply_gradient, adorym/optimizers.py:594-704): the whole-object sums of the
// Polak-Ribiere beta and of the line search's entry values, the direction update, the trial points and the accepted point.
// Streaming kernels over flat float32 arrays: 16-byte accesses when every pointer is 16-byte aligned (the driver's arrays are),
// 4-byte ones otherwise (a view that starts at an odd element), a grid sized to the chip, LDS for the workgroup sums only.
// Sums: products formed in double from the float inputs, one double accumulator per thread (its elements in ascending order), one
// partial per workgroup (shuffle tree, then the waves in ascending order), and a one-workgroup finishing kernel that adds the
// partials in ascending order (from LDS).  No atomics: the same inputs at the same alignment give the same bits on every run.
#include <hip/hip_runtime.h>
#include "adm_host.h"
#include "adm_optim.h"

namespace adm {
// (the walk over the flat arrays, the grid, the alignment test and the workgroup's double sum: adm_optim.h, shared with adm_kappa_tie.hip)
#define CG_THREADS FLAT_THREADS
// sums block (device: scratch[0 .. 8), host: sums_host[0 .. 8)), then the partials
enum { CG_A = 0, CG_B = 1, CG_BETA = 2, CG_C = 3, CG_E = 4, CG_D = 5, CG_SUMS = 8 };

// A = sum d (d - d_old), B = sum d_old^2 with d = -g   (_calculate_PR_beta, adorym/optimizers.py:606-628)
template <bool VEC>
__global__ __launch_bounds__(CG_THREADS) void cg_beta_kernel(const float* __restrict__ g, const float* __restrict__ d_old, size_t n,
                                                             double* __restrict__ part) {
    __shared__ double red[CG_THREADS / 64];
    double a = 0.0, b = 0.0;
    auto term = [&](float gv, float ov) {
        const double d = -(double)gv, o = (double)ov;
        a += d * (d - o);
        b += o * o;
    };
    flat_walk<VEC>(n, [&](size_t i) { term(g[i], d_old[i]); },
                 [&](size_t q) {
                     const float4 gv = ((const float4*)g)[q], ov = ((const float4*)d_old)[q];
                     term(gv.x, ov.x); term(gv.y, ov.y); term(gv.z, ov.z); term(gv.w, ov.w);
                 });
    const double ta = flat_block_sum(a, red), tb = flat_block_sum(b, red);
    if (threadIdx.x == 0) { part[2 * blockIdx.x] = ta; part[2 * blockIdx.x + 1] = tb; }
}

// s <- d + beta s, d_old <- d (d = -g), with C = sum s_new g, E = sum s_new^2, D = sum g^2   (optimizers.py:650, 669-672, 700-701;
// linesearch.py:148-149).  beta is where the finishing kernel of the beta sums left it.
template <bool VEC>
__global__ __launch_bounds__(CG_THREADS) void cg_direction_kernel(const float* __restrict__ g, float* __restrict__ s, float* __restrict__ d_old,
                                                                  const double* __restrict__ sums, size_t n, double* __restrict__ part) {
    __shared__ double red[CG_THREADS / 64];
    const float beta = (float)sums[CG_BETA];
    double c = 0.0, e = 0.0, dd = 0.0;
    auto term = [&](float gv, float sv) {
        const float sn = -gv + beta * sv;
        const double s64 = (double)sn, g64 = (double)gv;
        c += s64 * g64;
        e += s64 * s64;
        dd += g64 * g64;
        return sn;
    };
    flat_walk<VEC>(n, [&](size_t i) { const float gv = g[i]; s[i] = term(gv, s[i]); d_old[i] = -gv; },
                 [&](size_t q) {
                     const float4 gv = ((const float4*)g)[q], sv = ((const float4*)s)[q];
                     ((float4*)s)[q] = make_float4(term(gv.x, sv.x), term(gv.y, sv.y), term(gv.z, sv.z), term(gv.w, sv.w));
                     ((float4*)d_old)[q] = make_float4(-gv.x, -gv.y, -gv.z, -gv.w);
                 });
    const double tc = flat_block_sum(c, red), te = flat_block_sum(e, red), td = flat_block_sum(dd, red);
    if (threadIdx.x == 0) { part[3 * blockIdx.x] = tc; part[3 * blockIdx.x + 1] = te; part[3 * blockIdx.x + 2] = td; }
}

// The partials of nq quantities added in ascending order of the workgroups, quantity k on thread k; first = CG_A or CG_C.  The
// workgroup first brings the partials into LDS together (one trip to memory: a thread that reads them from memory as it adds waits
// for a trip every few terms -- beta + direction at 256^3 x 2 took 0.217 ms that way and 0.184 ms this way).  After the beta sums:
// beta = max(A / B, 0) when i_batch > 0 and B > 0, else 0 (the reference divides by B = 0 and carries a NaN).  The sums go to the
// device block (the direction kernel reads beta there) and to the host's (page-locked, written in place like the loss sums).
__global__ __launch_bounds__(CG_THREADS) void cg_finish_kernel(const double* __restrict__ part, int nb, int nq, int first, int i_batch,
                                                               double* __restrict__ sums, double* __restrict__ sums_host) {
    __shared__ double sh[3 * ADM_CG_MAX_BLOCKS];
    for (int i = threadIdx.x; i < nb * nq; i += CG_THREADS) sh[i] = part[i];
    __syncthreads();
    double t = 0.0;
    if ((int)threadIdx.x < nq) {
        for (int b = 0; b < nb; ++b) t += sh[b * nq + threadIdx.x];
        sums[first + threadIdx.x] = t;
        sums_host[first + threadIdx.x] = t;
    }
    if (first == CG_A && threadIdx.x < 64) {
        const double a = __shfl(t, 0, 64), b = __shfl(t, 1, 64);
        if (threadIdx.x == 0) {
            const double beta = (i_batch > 0 && b > 0.0) ? fmax(a / b, 0.0) : 0.0;
            sums[CG_BETA] = beta;
            sums_host[CG_BETA] = beta;
        }
    }
}

// s <- -g: the direction when the conjugate one does not descend (optimizers.py:672-674)
template <bool VEC>
__global__ __launch_bounds__(CG_THREADS) void cg_fallback_kernel(const float* __restrict__ g, float* __restrict__ s, size_t n) {
    flat_walk<VEC>(n, [&](size_t i) { s[i] = -g[i]; },
                 [&](size_t q) { const float4 gv = ((const float4*)g)[q]; ((float4*)s)[q] = make_float4(-gv.x, -gv.y, -gv.z, -gv.w); });
}

// x_trial <- x0 + alpha s: a trial point of the line search (optimizers.py:676-677, linesearch.py:160, 173)
template <bool VEC>
__global__ __launch_bounds__(CG_THREADS) void cg_trial_kernel(const float* __restrict__ x0, const float* __restrict__ s, float alpha,
                                                              float* __restrict__ xt, size_t n) {
    flat_walk<VEC>(n, [&](size_t i) { xt[i] = x0[i] + alpha * s[i]; },
                 [&](size_t q) {
                     const float4 xv = ((const float4*)x0)[q], sv = ((const float4*)s)[q];
                     ((float4*)xt)[q] = make_float4(xv.x + alpha * sv.x, xv.y + alpha * sv.y, xv.z + alpha * sv.z, xv.w + alpha * sv.w);
                 });
}

// x[i] <- constrain(src[i]) for i in [lo, lo + n): the accepted point under the constraints and the support mask of the optimiser
// steps (adm_optim.h; the channel is the parity of i, the mask entry i / 2).  src may be x itself.  VEC: lo is a multiple of 4.
template <bool VEC>
__global__ __launch_bounds__(CG_THREADS) void cg_accept_kernel(float* x, const float* src, size_t lo, size_t n, int flags,
                                                               const float* __restrict__ mask) {
    float* xl = x + lo;
    const float* sl = src + lo;
    flat_walk<VEC>(n, [&](size_t i) { xl[i] = constrain(sl[i], lo + i, flags, mask); },
                 [&](size_t q) {
                     const float4 v = ((const float4*)sl)[q];
                     const size_t i = lo + 4 * q;
                     ((float4*)xl)[q] = make_float4(constrain(v.x, i, flags, mask), constrain(v.y, i + 1, flags, mask),
                                                   constrain(v.z, i + 2, flags, mask), constrain(v.w, i + 3, flags, mask));
                 });
}
}  // namespace adm
using namespace adm;

#define CG_LAUNCH(kernel, vec, n, ...)                                                                                     \
    do {                                                                                                                   \
        if (vec) hipLaunchKernelGGL(kernel<true>, dim3(flat_grid(n)), dim3(CG_THREADS), 0, ctx->stream, __VA_ARGS__);        \
        else hipLaunchKernelGGL(kernel<false>, dim3(flat_grid(n)), dim3(CG_THREADS), 0, ctx->stream, __VA_ARGS__);           \
        ADM_HIP(hipGetLastError());                                                                                        \
    } while (0)

extern "C" int adm_cg_beta(adm_ctx* ctx, const float* g, const float* d_old, size_t n, int i_batch, double* scratch, double* sums_host) {
    if (!ctx || !g || !d_old || !scratch || !sums_host) return fail(ADM_ERR_INVALID, "adm_cg_beta: null argument");
    if (!n) return fail(ADM_ERR_INVALID, "adm_cg_beta: n = 0");
    double* part = scratch + CG_SUMS;
    CG_LAUNCH(cg_beta_kernel, flat_aligned(g, d_old), n, g, d_old, n, part);
    hipLaunchKernelGGL(cg_finish_kernel, dim3(1), dim3(CG_THREADS), 0, ctx->stream, (const double*)part, flat_grid(n), 2, (int)CG_A, i_batch, scratch,
                       sums_host);
    ADM_HIP(hipGetLastError());
    return ADM_OK;
}

extern "C" int adm_cg_direction(adm_ctx* ctx, const float* g, float* s, float* d_old, size_t n, double* scratch, double* sums_host) {
    if (!ctx || !g || !s || !d_old || !scratch || !sums_host) return fail(ADM_ERR_INVALID, "adm_cg_direction: null argument");
    if (!n) return fail(ADM_ERR_INVALID, "adm_cg_direction: n = 0");
    double* part = scratch + CG_SUMS;
    CG_LAUNCH(cg_direction_kernel, flat_aligned(g, s, d_old), n, g, s, d_old, (const double*)scratch, n, part);
    hipLaunchKernelGGL(cg_finish_kernel, dim3(1), dim3(CG_THREADS), 0, ctx->stream, (const double*)part, flat_grid(n), 3, (int)CG_C, 0, scratch,
                       sums_host);
    ADM_HIP(hipGetLastError());
    return ADM_OK;
}

extern "C" int adm_cg_fallback(adm_ctx* ctx, const float* g, float* s, size_t n) {
    if (!ctx || !g || !s) return fail(ADM_ERR_INVALID, "adm_cg_fallback: null argument");
    if (!n) return ADM_OK;
    CG_LAUNCH(cg_fallback_kernel, flat_aligned(g, s), n, g, s, n);
    return ADM_OK;
}

extern "C" int adm_cg_trial(adm_ctx* ctx, const float* x0, const float* s, float alpha, float* x_trial, size_t n) {
    if (!ctx || !x0 || !s || !x_trial) return fail(ADM_ERR_INVALID, "adm_cg_trial: null argument");
    if (!n) return ADM_OK;
    CG_LAUNCH(cg_trial_kernel, flat_aligned(x0, s, x_trial), n, x0, s, alpha, x_trial, n);
    return ADM_OK;
}

extern "C" int adm_cg_accept(adm_ctx* ctx, float* x, const float* x_src, size_t lo, size_t hi, int flags, const float* mask) {
    if (!ctx || !x || !x_src) return fail(ADM_ERR_INVALID, "adm_cg_accept: null argument");
    if (hi <= lo) return ADM_OK;
    CG_LAUNCH(cg_accept_kernel, flat_aligned(x + lo, x_src + lo) && !(lo & 3), hi - lo, x, x_src, lo, hi - lo, flags, mask);
    return ADM_OK;
}
