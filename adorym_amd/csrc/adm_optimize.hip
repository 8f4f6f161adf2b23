// Fused optimiser steps (R13-R15): Adam / GD / momentum + constraints, the small parameters' one launch, the drift guard, axpy.
#include <hip/hip_runtime.h>
#include <cstring>
#include "adm_host.h"
#include "adm_optim.h"
#include "adm_block_sum.h"

namespace adm {
// x[r][c] -= mean_r x[r][c]   (adorym/optimizers.py:1046-1048), one workgroup
// body of center_rows_kernel for one workgroup of 256 threads (also the tail of small_adam_kernel: same sums, same bits)
__device__ __forceinline__ void center_rows_block(float* __restrict__ x, size_t n_rows, int n_cols, float* red, float* mean) {
    for (int c = 0; c < n_cols; ++c) {
        float acc = 0.f;
        for (size_t r = threadIdx.x; r < n_rows; r += blockDim.x) acc += x[r * n_cols + c];
        const float t = block_sum_f32(acc, red, 4);
        if (threadIdx.x == 0) *mean = t / (float)n_rows;
        __syncthreads();
        const float mu = *mean;
        for (size_t r = threadIdx.x; r < n_rows; r += blockDim.x) x[r * n_cols + c] -= mu;
        __syncthreads();
    }
}

__global__ __launch_bounds__(256) void center_rows_kernel(float* __restrict__ x, size_t n_rows, int n_cols) {
    __shared__ float red[4];
    __shared__ float mean;
    center_rows_block(x, n_rows, n_cols, red, &mean);
}

// --------------------------------------------------------------------------------------------
// Fused optimiser steps.  AdamOptimizer.apply_gradient (adorym/optimizers.py:309-318):
//   m = b1*m; m = m + (1-b1)*g; v = b2*v; v = v + (1-b2)*g^2;
//   x = x - step*(m/q1) / (sqrt(v/q2) + eps),  q = 1 - b^(i_batch+1)
// followed by the constraints of adorym/ptychography.py:1135-1158 and the support mask
// (adorym/array_ops.py:239-251).  Same operation order as the reference, fp32.
// --------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void adam_kernel(float* __restrict__ x, const float* __restrict__ g, float* __restrict__ m,
                                                   float* __restrict__ v, size_t lo, size_t hi, AdamScalars a) {
    for (size_t i = lo + (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < hi; i += (size_t)gridDim.x * blockDim.x) {
        float mv, vv;
        const float xn = adam_value(x[i], g[i], m[i], v[i], a, i, mv, vv);
        m[i] = mv;
        v[i] = vv;
        x[i] = xn;
    }
}

// The small optimisable parameters of a minibatch (probe modes, sub-pixel position corrections, propagation distances, affine
// matrices: KBs each) updated in ONE launch, one workgroup per array: Adam with adam_kernel's arithmetic, then -- per array, as
// asked -- the drift guard of the position corrections (center_rows_kernel's sums), the pin of the first entries to fixed values,
// and the zero fill of the gradient accumulator for the next minibatch.  These paths are launch-bound (4-5 us per launch whatever
// its size): config-5 shape 24 -> 17 launches per minibatch, config-1 shape 17 -> 10.
// An array without a drift guard is element-wise, so it is spread over ceil(n / chunk) workgroups (five probe modes of
// 64 x 64 took 77 us in ONE workgroup, 40 % of a config-1-shape minibatch); an array with one stays in a single workgroup
// (its column means need every element).  first_block[i]: the first workgroup of array i; first_block[count] = grid size.
// Elements per workgroup of an element-wise array: 2048 for the genuinely small ones (a few KB); anything larger -- five 64 x 64
// probe modes, the 2-D object itself, which the driver adds to this launch on one rank -- gets 256: one element per thread, like adam_kernel
// (8 dependent iterations per thread made the launch 8.4 us for a 512 x 512 x 2 object against adam_kernel's 5.6 us).
static inline int small_chunk(uint64_t n) { return n > 4096 ? 256 : 2048; }
struct SmallParams { adm_small_param p[ADM_SMALL_PARAMS_MAX]; int first_block[ADM_SMALL_PARAMS_MAX + 1]; int chunk[ADM_SMALL_PARAMS_MAX]; int count; };

// An array with a drift guard, held in registers: thread t owns the rows t, t + 256, ... (all NC columns of each), so that the
// Adam step, the column sums (in center_rows_block's order: rows ascending per thread, the same shuffle tree, the same four partial
// sums -- the same bits), the subtraction and the pin need ONE round of loads and ONE of stores.  The generic path below makes
// ~35 dependent trips to memory for the 1 400 x 2 position corrections of a config-1 minibatch (17 us, the longest block of the launch).
#define SMALL_WHOLE_RPT 8
template <int NC>
__device__ __forceinline__ void small_adam_whole(const adm_small_param& q, const AdamScalars& a, float* red, float* mean) {
    const size_t n_rows = q.n / NC;
    float xv[SMALL_WHOLE_RPT][NC];
#pragma unroll
    for (int j = 0; j < SMALL_WHOLE_RPT; ++j) {
        const size_t r = threadIdx.x + (size_t)256 * j;
        if (r < n_rows) {
            float gv[NC], mv[NC], vv[NC];
#pragma unroll
            for (int c = 0; c < NC; ++c) { const size_t i = r * NC + c; xv[j][c] = q.x[i]; gv[c] = q.g[i]; mv[c] = q.m[i]; vv[c] = q.v[i]; }
#pragma unroll
            for (int c = 0; c < NC; ++c) {
                const size_t i = r * NC + c;
                float mo, vo;
                xv[j][c] = adam_value(xv[j][c], gv[c], mv[c], vv[c], a, i, mo, vo);
                q.m[i] = mo;
                q.v[i] = vo;
                if (q.zero_grad) q.g[i] = 0.f;
            }
        } else {
#pragma unroll
            for (int c = 0; c < NC; ++c) xv[j][c] = 0.f;
        }
    }
#pragma unroll
    for (int c = 0; c < NC; ++c) {
        float acc = 0.f;
#pragma unroll
        for (int j = 0; j < SMALL_WHOLE_RPT; ++j)
            if (threadIdx.x + (size_t)256 * j < n_rows) acc += xv[j][c];
        const float t = block_sum_f32(acc, red, 4);
        if (threadIdx.x == 0) *mean = t / (float)n_rows;
        __syncthreads();
        const float mu = *mean;
#pragma unroll
        for (int j = 0; j < SMALL_WHOLE_RPT; ++j) xv[j][c] -= mu;
        __syncthreads();
    }
#pragma unroll
    for (int j = 0; j < SMALL_WHOLE_RPT; ++j) {
        const size_t r = threadIdx.x + (size_t)256 * j;
        if (r < n_rows) {
#pragma unroll
            for (int c = 0; c < NC; ++c) {
                const size_t i = r * NC + c;
                q.x[i] = (q.pin && i < q.pin_n) ? q.pin[i] : xv[j][c];
            }
        }
    }
}

__global__ __launch_bounds__(256) void small_adam_kernel(SmallParams sp, AdamScalars a) {
    __shared__ float red[4];
    __shared__ float mean;
    int k = 0;
    while (k + 1 < sp.count && (int)blockIdx.x >= sp.first_block[k + 1]) ++k;
    const adm_small_param q = sp.p[k];
    const bool whole = q.center_cols > 0;
    if (whole && q.center_cols <= 2 && q.n / (size_t)q.center_cols <= (size_t)256 * SMALL_WHOLE_RPT) {
        a.step = (float)q.step_size;
        if (q.center_cols == 1) small_adam_whole<1>(q, a, red, &mean);
        else small_adam_whole<2>(q, a, red, &mean);
        return;
    }
    const size_t chunk = (size_t)sp.chunk[k];
    const size_t lo = whole ? 0 : (size_t)(blockIdx.x - sp.first_block[k]) * chunk;
    const size_t hi = whole ? q.n : (lo + chunk < q.n ? lo + chunk : q.n);
    a.step = (float)q.step_size;
    for (size_t i = lo + threadIdx.x; i < hi; i += blockDim.x) {
        float mv, vv;
        float xn = adam_value(q.x[i], q.g[i], q.m[i], q.v[i], a, i, mv, vv);
        q.m[i] = mv;
        q.v[i] = vv;
        if (!whole && q.pin && i < q.pin_n) xn = q.pin[i];       // (with a drift guard the pin follows the re-centring, below)
        q.x[i] = xn;
        if (q.zero_grad) q.g[i] = 0.f;
    }
    if (!whole) return;
    __syncthreads();
    center_rows_block(q.x, q.n / (size_t)q.center_cols, q.center_cols, red, &mean);
    if (q.pin) {
        for (size_t i = threadIdx.x; i < q.pin_n; i += blockDim.x) q.x[i] = q.pin[i];
    }
}

__global__ __launch_bounds__(256) void gd_kernel(float* __restrict__ x, const float* __restrict__ g, size_t lo, size_t hi,
                                                 float step, int flags, const float* __restrict__ mask) {
    for (size_t i = lo + (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < hi; i += (size_t)gridDim.x * blockDim.x)
        x[i] = gd_value(x[i], g[i], step, i, flags, mask);
}

__global__ __launch_bounds__(256) void momentum_kernel(float* __restrict__ x, const float* __restrict__ g, float* __restrict__ v,
                                                       size_t lo, size_t hi, float step, float gamma, int flags,
                                                       const float* __restrict__ mask) {
    for (size_t i = lo + (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < hi; i += (size_t)gridDim.x * blockDim.x) {
        float vv;
        x[i] = momentum_value(x[i], g[i], v[i], step, gamma, i, flags, mask, vv);
        v[i] = vv;
    }
}

__global__ __launch_bounds__(256) void axpy_kernel(float* __restrict__ y, const float* __restrict__ x, float a, size_t n) {
    for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (size_t)gridDim.x * blockDim.x)
        y[i] += a * x[i];
}
}  // namespace adm
using namespace adm;

extern "C" int adm_center_rows(adm_ctx* ctx, float* x, size_t n_rows, int n_cols) {
    if (!ctx || !x) return fail(ADM_ERR_INVALID, "adm_center_rows: null argument");
    if (n_rows == 0 || n_cols <= 0) return ADM_OK;
    hipLaunchKernelGGL(center_rows_kernel, dim3(1), dim3(256), 0, ctx->stream, x, n_rows, n_cols);
    ADM_HIP(hipGetLastError());
    return ADM_OK;
}

extern "C" int adm_adam_step(adm_ctx* ctx, float* x, const float* g, float* m, float* v, size_t lo, size_t hi, int i_batch,
                             double step_size, double b1, double b2, double eps, int flags, const float* mask) {
    if (!ctx || !x || !g || !m || !v) return fail(ADM_ERR_INVALID, "adm_adam_step: null argument");
    if (hi <= lo) return ADM_OK;
    hipLaunchKernelGGL(adam_kernel, dim3(stream_grid(hi - lo)), dim3(256), 0, ctx->stream, x, g, m, v, lo, hi,
                       adam_scalars(i_batch, step_size, b1, b2, eps, flags, mask));
    ADM_HIP(hipGetLastError());
    return ADM_OK;
}

extern "C" int adm_adam_step_small(adm_ctx* ctx, const adm_small_param* params, int count, int i_batch, double b1, double b2, double eps) {
    if (!ctx || !params) return fail(ADM_ERR_INVALID, "adm_adam_step_small: null argument");
    if (count <= 0) return ADM_OK;
    if (count > ADM_SMALL_PARAMS_MAX) return fail(ADM_ERR_INVALID, "adm_adam_step_small: too many arrays in one call");
    SmallParams sp;
    std::memset(&sp, 0, sizeof(sp));
    int nblocks = 0;
    for (int k = 0; k < count; ++k) {
        const adm_small_param& q = params[k];
        if (!q.x || !q.g || !q.m || !q.v) return fail(ADM_ERR_INVALID, "adm_adam_step_small: null array");
        if (q.center_cols > 0 && q.n % (uint64_t)q.center_cols) return fail(ADM_ERR_INVALID, "adm_adam_step_small: n is not a multiple of center_cols");
        if (q.pin && q.pin_n > q.n) return fail(ADM_ERR_INVALID, "adm_adam_step_small: pin_n exceeds n");
        sp.p[k] = q;
        sp.first_block[k] = nblocks;
        sp.chunk[k] = small_chunk(q.n);
        nblocks += q.center_cols > 0 ? 1 : (int)((q.n + sp.chunk[k] - 1) / sp.chunk[k]);
    }
    sp.first_block[count] = nblocks;
    sp.count = count;
    if (nblocks == 0) return ADM_OK;
    hipLaunchKernelGGL(small_adam_kernel, dim3(nblocks), dim3(256), 0, ctx->stream, sp, adam_scalars(i_batch, 0.0, b1, b2, eps, 0, nullptr));
    ADM_HIP(hipGetLastError());
    return ADM_OK;
}

extern "C" int adm_gd_step(adm_ctx* ctx, float* x, const float* g, size_t lo, size_t hi, double step_size, int flags,
                           const float* mask) {
    if (!ctx || !x || !g) return fail(ADM_ERR_INVALID, "adm_gd_step: null argument");
    if (hi <= lo) return ADM_OK;
    hipLaunchKernelGGL(gd_kernel, dim3(stream_grid(hi - lo)), dim3(256), 0, ctx->stream, x, g, lo, hi, (float)step_size, flags, mask);
    ADM_HIP(hipGetLastError());
    return ADM_OK;
}

extern "C" int adm_momentum_step(adm_ctx* ctx, float* x, const float* g, float* v, size_t lo, size_t hi, double step_size,
                                 double gamma, int flags, const float* mask) {
    if (!ctx || !x || !g || !v) return fail(ADM_ERR_INVALID, "adm_momentum_step: null argument");
    if (hi <= lo) return ADM_OK;
    hipLaunchKernelGGL(momentum_kernel, dim3(stream_grid(hi - lo)), dim3(256), 0, ctx->stream, x, g, v, lo, hi, (float)step_size,
                       (float)gamma, flags, mask);
    ADM_HIP(hipGetLastError());
    return ADM_OK;
}

extern "C" int adm_axpy(adm_ctx* ctx, float* y, const float* x, float a, size_t n) {
    if (!ctx || !y || !x) return fail(ADM_ERR_INVALID, "adm_axpy: null argument");
    if (!n) return ADM_OK;
    hipLaunchKernelGGL(axpy_kernel, dim3(stream_grid(n)), dim3(256), 0, ctx->stream, y, x, a, n);
    ADM_HIP(hipGetLastError());
    return ADM_OK;
}
