// The fp32 sum of one value per thread over a workgroup, in a fixed order, for the element-wise kernels (adm_regularize.hip,
// adm_optimize.hip).  The multislice kernels keep reductions of their own (adm_multislice.hip, adm_ms_gen.h, adm_ms_col.h).
#pragma once
#include <hip/hip_runtime.h>
namespace adm {
// Every wave adds its 64 lanes with a __shfl_down tree (offsets 32 ... 1), the wave leaders leave their sums in red[wave] (LDS,
// n_waves = blockDim.x / 64 floats), and thread 0 adds red[0] + red[1] + ... in ascending order; the sum is returned on thread 0 only.
// One barrier inside, NONE at the end: a caller that writes red[] again (center_rows_block's loop) puts its own in between.  The value
// comes by reference and is copied: by value, the CALLER's element loop is compiled differently (reg_grad_weighted_kernel: +2 VGPRs).
__device__ __forceinline__ float block_sum_f32(const float& value, float* red, int n_waves) {
    float v = value;
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) v += __shfl_down(v, off, 64);
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = v;
    __syncthreads();
    if (threadIdx.x != 0) return 0.f;
    float t = red[0];
    for (int w = 1; w < n_waves; ++w) t += red[w];
    return t;
}
}  // namespace adm
