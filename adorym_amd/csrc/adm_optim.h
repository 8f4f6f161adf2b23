// Element-wise optimiser arithmetic shared by the kernels that apply it: adam_kernel / small_adam_kernel / gd_kernel /
// momentum_kernel (adm_optimize.hip: one rank, or the owned shard after an RCCL reduce-scatter) and the peer-to-peer fused
// exchange (adm_p2p.hip: sum over the ranks' gradient buffers + the same step + write to every replica).  One definition,
// contraction off, so that every caller produces the same bits.
//   AdamOptimizer.apply_gradient      adorym/optimizers.py:309-318
//   GDOptimizer.apply_gradient        adorym/optimizers.py:440-464
//   MomentumOptimizer.apply_gradient  adorym/optimizers.py:376-411
//   constraints / support mask        adorym/ptychography.py:1135-1158, adorym/array_ops.py:239-251
#pragma once
#include <hip/hip_runtime.h>
#include "../../include/adm.h"     // ADM_FLAG_*
#include "adm_common.h"

namespace adm {

__device__ __forceinline__ float constrain(float xv, size_t i, int flags, const float* mask) {
    if ((flags & ADM_FLAG_NONNEG) && xv < 0.f) xv = 0.f;
    if ((flags & ADM_FLAG_ZERO_CH0) && !(i & 1)) xv *= 0.f;
    if ((flags & ADM_FLAG_ZERO_CH1) && (i & 1)) xv *= 0.f;
    if (mask) xv *= mask[i >> 1];
    return xv;
}

struct AdamScalars {
    float step, b1, b2, omb1, omb2, q1, q2, eps;
    int flags;
    const float* mask;
};

// one element of AdamOptimizer.apply_gradient + constraints
__device__ __forceinline__ float adam_value(float xv, float gv, float m_in, float v_in, const AdamScalars& a, size_t i, float& m_out,
                                            float& v_out) {
#pragma clang fp contract(off)
    float mv = a.b1 * m_in;
    mv = mv + a.omb1 * gv;
    float vv = a.b2 * v_in;
    vv = vv + a.omb2 * (gv * gv);
    const float mhat = mv / a.q1;
    const float vhat = vv / a.q2;
    const float d = a.step * mhat / (sqrtf(vhat) + a.eps);
    m_out = mv;
    v_out = vv;
    return constrain(xv - d, i, a.flags, a.mask);
}

__device__ __forceinline__ float gd_value(float xv, float gv, float step, size_t i, int flags, const float* mask) {
#pragma clang fp contract(off)
    return constrain(xv - step * gv, i, flags, mask);
}

__device__ __forceinline__ float momentum_value(float xv, float gv, float v_in, float step, float gamma, size_t i, int flags,
                                                const float* mask, float& v_out) {
#pragma clang fp contract(off)
    const float vv = gamma * v_in + step * gv;
    v_out = vv;
    return constrain(xv - vv, i, flags, mask);
}

// ---- streaming kernels over flat float32 arrays (adm_cg.hip, adm_kappa_tie.hip): FLAT_THREADS threads, a grid sized to the chip,
// wide accesses when every pointer of a call is 16-byte aligned, a workgroup's double sum in a fixed order
#define FLAT_THREADS 256

static inline int flat_grid(size_t n) {     // 16 elements per thread until the cap: ADM_CG_MAX_BLOCKS = 4 workgroups per CU
    size_t b = (n + 16 * FLAT_THREADS - 1) / (16 * FLAT_THREADS);
    return (int)(b > ADM_CG_MAX_BLOCKS ? ADM_CG_MAX_BLOCKS : (b ? b : 1));
}
static inline bool flat_aligned(const void* a, const void* b = nullptr, const void* c = nullptr, const void* d = nullptr) {
    return (((uintptr_t)a | (uintptr_t)b | (uintptr_t)c | (uintptr_t)d) & 15) == 0;
}

// the sum of one double per thread over the workgroup, on thread 0; red: FLAT_THREADS / 64 doubles of LDS
__device__ __forceinline__ double flat_block_sum(double v, double* red) {
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) v += __shfl_down(v, off, 64);
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = v;
    __syncthreads();
    double t = 0.0;
    if (threadIdx.x == 0) {
        t = red[0];
        for (int w = 1; w < FLAT_THREADS / 64; ++w) t += red[w];
    }
    __syncthreads();
    return t;
}

// Every kernel walks its n elements the same way: VEC, group q (W elements, one wide access) of thread t, t + T, ... (T = all
// threads of the grid), then the n % W last elements one each on the first threads; otherwise element by element.  `one(i)` handles
// element i, `wide(q)` elements W q ... W q + W - 1.
template <bool VEC, int W = 4, class One, class Wide>
__device__ __forceinline__ void flat_walk(size_t n, One one, Wide wide) {
    const size_t t = (size_t)blockIdx.x * FLAT_THREADS + threadIdx.x, T = (size_t)gridDim.x * FLAT_THREADS;
    if (VEC) {
        const size_t nw = n / W;
        for (size_t q = t; q < nw; q += T) wide(q);
        const size_t i = nw * W + t;
        if (i < n) one(i);
    } else {
        for (size_t i = t; i < n; i += T) one(i);
    }
}

static inline AdamScalars adam_scalars(int i_batch, double step_size, double b1, double b2, double eps, int flags, const float* mask) {
    // the reference evaluates the scalars in Python doubles and torch casts them to fp32 at the op
    AdamScalars a;
    double p1 = 1.0, p2 = 1.0;
    for (int k = 0; k < i_batch + 1; ++k) { p1 *= b1; p2 *= b2; }
    a.step = (float)step_size; a.b1 = (float)b1; a.b2 = (float)b2;
    a.omb1 = (float)(1.0 - b1); a.omb2 = (float)(1.0 - b2);
    a.q1 = (float)(1.0 - p1); a.q2 = (float)(1.0 - p2);
    a.eps = (float)eps; a.flags = flags; a.mask = mask;
    return a;
}

}  // namespace adm
