// The single-material (homogeneous-object) constraint of Fresnel multi-distance holography: beta = kappa delta with
// kappa = 10^lg_kappa, applied to the OBJECT in front of the forward model (multislice_propagate_batch(..., kappa=...),
// adorym/propagate.py:223-225; MultiDistModel.predict, adorym/forward_model.py:876-878, 1003-1010), and its transpose, which folds
// the gradient w.r.t. the tied object back into the gradients w.r.t. delta and lg_kappa.  (The CTF model divides by the same
// number, cos(xi) / kappa: adm_holo_ctf.hip.  The two senses are the reference's and stay apart.)
// Two streaming kernels over interleaved (delta, beta) voxels, built like adm_cg.hip from the pieces of adm_optim.h: 16-byte
// accesses (two voxels) when every pointer is 16-byte aligned, 8-byte ones (one voxel) otherwise, a grid capped by
// ADM_CG_MAX_BLOCKS, LDS for kappa and the workgroup sum only.  kappa = exp(ln10 (double)lg_kappa[0]) is formed in double by one
// thread per workgroup, rounded once to float and handed over through LDS.  The sum S = sum_v delta_v g_beta_v: products in double
// from the float inputs, one accumulator per thread (its voxels in ascending order), one partial per workgroup (shuffle tree, then
// the waves in ascending order), and a one-workgroup finishing kernel that adds the partials in ascending order.  No atomics.
#include <hip/hip_runtime.h>
#include "adm_host.h"
#include "adm_optim.h"

namespace adm {
#define KAPPA_LN10 2.302585092994045684

__device__ __forceinline__ double kappa_f64(const float* lg_kappa) { return exp(KAPPA_LN10 * (double)lg_kappa[0]); }

// kappa32 for every thread of the workgroup: one double exp, not FLAT_THREADS of them
__device__ __forceinline__ float stage_kappa(float* slot, const float* lg_kappa) {
    if (threadIdx.x == 0) *slot = (float)kappa_f64(lg_kappa);
    __syncthreads();
    return *slot;
}

// Products and sums that are rounded to float one by one.  (__fmul_rn / __fadd_rn are plain operators in this toolchain's headers,
// compiled under the default -ffp-contract=fast: a product and a sum of theirs can still merge into one fused multiply-add.  With
// contraction off in the function that spells the operators out, as in mul_rounded of adm_line_fft.h, they cannot.)
__device__ __forceinline__ float mul_rn(float a, float b) {
#pragma clang fp contract(off)
    return a * b;
}
__device__ __forceinline__ float add_rn(float a, float b) {
#pragma clang fp contract(off)
    return a + b;
}
// u = g_delta + kappa32 g_beta
__device__ __forceinline__ float fold_u(float k, float gd, float gb) {
#pragma clang fp contract(off)
    const float p = k * gb;
    return gd + p;
}

// out_v = (delta_v, kappa32 delta_v); obj's beta channel is loaded with its voxel and not used
template <bool VEC>
__global__ __launch_bounds__(FLAT_THREADS) void kappa_tie_kernel(const float2* __restrict__ obj, const float* __restrict__ lg_kappa,
                                                                 size_t n_vox, float2* __restrict__ out) {
    __shared__ float ks;
    const float k = stage_kappa(&ks, lg_kappa);
    flat_walk<VEC, 2>(n_vox, [&](size_t v) { const float d = obj[v].x; out[v] = make_float2(d, mul_rn(k, d)); },
                      [&](size_t q) {
                          const float4 o = ((const float4*)obj)[q];
                          ((float4*)out)[q] = make_float4(o.x, mul_rn(k, o.x), o.z, mul_rn(k, o.z));
                      });
}

// u_v = g_delta_v + kappa32 g_beta_v (multiply and add rounded separately);  MODE 1: grad_obj_v.delta += u_v, beta untouched;
// MODE 2: grad_obj_v = (u_v, 0).  SUM: the workgroup's part of S = sum_v delta_v g_beta_v.
template <bool VEC, int MODE, bool SUM>
__global__ __launch_bounds__(FLAT_THREADS) void kappa_fold_kernel(const float2* __restrict__ obj, const float* __restrict__ lg_kappa,
                                                                  const float2* __restrict__ gt, size_t n_vox, float2* __restrict__ go,
                                                                  double* __restrict__ part) {
    __shared__ float ks;
    __shared__ double red[FLAT_THREADS / 64];
    const float k = stage_kappa(&ks, lg_kappa);
    double s = 0.0;
    flat_walk<VEC, 2>(n_vox,
                      [&](size_t v) {
                          const float2 g = gt[v];
                          const float u = fold_u(k, g.x, g.y);
                          if (SUM) s += (double)obj[v].x * (double)g.y;
                          if (MODE == 1) go[v].x = add_rn(go[v].x, u);
                          else go[v] = make_float2(u, 0.f);
                      },
                      [&](size_t q) {
                          const float4 g = ((const float4*)gt)[q];
                          const float u0 = fold_u(k, g.x, g.y), u1 = fold_u(k, g.z, g.w);
                          if (SUM) {
                              const float4 o = ((const float4*)obj)[q];
                              s += (double)o.x * (double)g.y;
                              s += (double)o.z * (double)g.w;
                          }
                          if (MODE == 1) {
                              float4 r = ((float4*)go)[q];          // (the beta channels go back with the bits they came with)
                              r.x = add_rn(r.x, u0);
                              r.z = add_rn(r.z, u1);
                              ((float4*)go)[q] = r;
                          } else {
                              ((float4*)go)[q] = make_float4(u0, 0.f, u1, 0.f);
                          }
                      });
    if (SUM) {
        const double t = flat_block_sum(s, red);
        if (threadIdx.x == 0) part[blockIdx.x] = t;
    }
}

// S = the nb partials in ascending order (brought into LDS together, as in cg_finish_kernel), left in scratch[0];
// grad_lg_kappa[0] (+)= (float)(ln10 kappa S) with kappa in double: dL/dlg_kappa = dkappa/dlg_kappa sum_v delta_v dL/dbeta_v
__global__ __launch_bounds__(FLAT_THREADS) void kappa_finish_kernel(double* __restrict__ scratch, int nb, const float* __restrict__ lg_kappa,
                                                                    int mode, float* __restrict__ grad_lg_kappa) {
    __shared__ double sh[ADM_CG_MAX_BLOCKS];
    const double* part = scratch + 1;
    for (int i = threadIdx.x; i < nb; i += FLAT_THREADS) sh[i] = part[i];
    __syncthreads();
    if (threadIdx.x != 0) return;
    double t = 0.0;
    for (int b = 0; b < nb; ++b) t += sh[b];
    scratch[0] = t;
    const float g = (float)(KAPPA_LN10 * kappa_f64(lg_kappa) * t);
    grad_lg_kappa[0] = mode == 1 ? add_rn(grad_lg_kappa[0], g) : g;
}
}  // namespace adm
using namespace adm;

static inline bool kappa_misaligned(const void* a, const void* b = nullptr, const void* c = nullptr) {       // a voxel is 8 bytes
    return (((uintptr_t)a | (uintptr_t)b | (uintptr_t)c) & 7) != 0;
}

#define KAPPA_LAUNCH(kernel, n_vox, ...)                                                                                   \
    do {                                                                                                                   \
        hipLaunchKernelGGL(kernel, dim3(flat_grid(2 * (n_vox))), dim3(FLAT_THREADS), 0, ctx->stream, __VA_ARGS__);        \
        ADM_HIP(hipGetLastError());                                                                                        \
    } while (0)

extern "C" int adm_kappa_tie(adm_ctx* ctx, const float* obj, const float* lg_kappa, size_t n_vox, float* out) {
    if (!ctx || !obj || !lg_kappa || !out) return fail(ADM_ERR_INVALID, "adm_kappa_tie: null argument");
    if (kappa_misaligned(obj, out)) return fail(ADM_ERR_INVALID, "adm_kappa_tie: a voxel array is not 8-byte aligned");
    if (!n_vox) return ADM_OK;
    if (flat_aligned(obj, out)) KAPPA_LAUNCH(kappa_tie_kernel<true>, n_vox, (const float2*)obj, lg_kappa, n_vox, (float2*)out);
    else KAPPA_LAUNCH(kappa_tie_kernel<false>, n_vox, (const float2*)obj, lg_kappa, n_vox, (float2*)out);
    return ADM_OK;
}

template <bool VEC, int MODE>
static int kappa_fold_launch(adm_ctx* ctx, const float2* obj, const float* lg_kappa, const float2* gt, size_t n_vox, float2* go, double* part) {
    if (part) KAPPA_LAUNCH((kappa_fold_kernel<VEC, MODE, true>), n_vox, obj, lg_kappa, gt, n_vox, go, part);
    else KAPPA_LAUNCH((kappa_fold_kernel<VEC, MODE, false>), n_vox, obj, lg_kappa, gt, n_vox, go, part);
    return ADM_OK;
}

extern "C" int adm_kappa_fold(adm_ctx* ctx, const float* obj, const float* lg_kappa, const float* grad_tied, size_t n_vox, int mode,
                              float* grad_obj, float* grad_lg_kappa, double* scratch) {
    if (!ctx || !obj || !lg_kappa || !grad_tied || !grad_obj) return fail(ADM_ERR_INVALID, "adm_kappa_fold: null argument");
    if (grad_lg_kappa && !scratch) return fail(ADM_ERR_INVALID, "adm_kappa_fold: grad_lg_kappa needs scratch");
    if (mode != 1 && mode != 2) return fail(ADM_ERR_INVALID, "adm_kappa_fold: mode must be 1 (add) or 2 (set)");
    if (!n_vox) return fail(ADM_ERR_INVALID, "adm_kappa_fold: n_vox = 0");
    if (kappa_misaligned(obj, grad_tied, grad_obj)) return fail(ADM_ERR_INVALID, "adm_kappa_fold: a voxel array is not 8-byte aligned");
    const float2 *o = (const float2*)obj, *gt = (const float2*)grad_tied;
    float2* go = (float2*)grad_obj;
    double* part = grad_lg_kappa ? scratch + 1 : nullptr;
    const bool vec = flat_aligned(obj, grad_tied, grad_obj);
    int rc;
    if (mode == 1) rc = vec ? kappa_fold_launch<true, 1>(ctx, o, lg_kappa, gt, n_vox, go, part) : kappa_fold_launch<false, 1>(ctx, o, lg_kappa, gt, n_vox, go, part);
    else rc = vec ? kappa_fold_launch<true, 2>(ctx, o, lg_kappa, gt, n_vox, go, part) : kappa_fold_launch<false, 2>(ctx, o, lg_kappa, gt, n_vox, go, part);
    if (rc != ADM_OK || !grad_lg_kappa) return rc;
    hipLaunchKernelGGL(kappa_finish_kernel, dim3(1), dim3(FLAT_THREADS), 0, ctx->stream, scratch, flat_grid(2 * n_vox), (const float*)lg_kappa, mode,
                       grad_lg_kappa);
    ADM_HIP(hipGetLastError());
    return ADM_OK;
}
