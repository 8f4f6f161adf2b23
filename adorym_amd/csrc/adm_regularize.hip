// Regularisers (R9): L1 + TV gradient and value for delta_beta and real_imag unknowns, reweighted L1.  Element-wise, HBM-bound.
#include <hip/hip_runtime.h>
#include "adm_host.h"
#include "adm_block_sum.h"

namespace adm {
// --------------------------------------------------------------------------------------------
// Regulariser gradient.  L1Regularizer (adorym/regularizers.py:30-46): alpha_c * mean|x_c|;
// TVRegularizer (regularizers.py:95-110 -> util.py:1427-1440): gamma * sum_axes sum|roll(a,1)-a| / V.
// --------------------------------------------------------------------------------------------
__device__ __forceinline__ float sgn(float v) { return (float)((v > 0.f) - (v < 0.f)); }

// The float2 offsets of row (y, xx) of the object and of its four periodic neighbour rows (z is the fastest axis)
struct RegRows { size_t row, row_xm, row_xp, row_ym, row_yp; };
__device__ __forceinline__ RegRows reg_rows(int y, int xx, int Y, int X, int Z) {
    const size_t sx = (size_t)Z, sy = (size_t)Z * X;
    return {(size_t)y * sy + (size_t)xx * sx,
            (size_t)y * sy + (size_t)((xx + X - 1) % X) * sx, (size_t)y * sy + (size_t)((xx + 1) % X) * sx,
            (size_t)((y + Y - 1) % Y) * sy + (size_t)xx * sx, (size_t)((y + 1) % Y) * sy + (size_t)xx * sx};
}

// The L1 + TV gradient of voxel z of that row; VALUE: its share of the regulariser value is added to val.  (The compiler contracts
// a * b + c here: one copy of the expressions, one set of bits.)
template <bool VALUE>
__device__ __forceinline__ float2 reg_stencil(const float2* __restrict__ x, const RegRows& r, int z, int Z, float a_d, float a_b,
                                              float gamma, float invV, float& val) {
    const float2 v = x[r.row + z];
    float2 gr = make_float2(0.f, 0.f);
    if (a_d != 0.f) { gr.x += a_d * sgn(v.x) * invV; if (VALUE) val += a_d * fabsf(v.x) * invV; }
    if (a_b != 0.f) { gr.y += a_b * sgn(v.y) * invV; if (VALUE) val += a_b * fabsf(v.y) * invV; }
    if (gamma != 0.f) {
        const float2 zm = x[r.row + (z + Z - 1) % Z], zp = x[r.row + (z + 1) % Z];
        const float2 xm = x[r.row_xm + z], xp = x[r.row_xp + z];
        const float2 ym = x[r.row_ym + z], yp = x[r.row_yp + z];
        gr.x += gamma * invV * ((sgn(v.x - zp.x) - sgn(zm.x - v.x)) + (sgn(v.x - xp.x) - sgn(xm.x - v.x)) + (sgn(v.x - yp.x) - sgn(ym.x - v.x)));
        gr.y += gamma * invV * ((sgn(v.y - zp.y) - sgn(zm.y - v.y)) + (sgn(v.y - xp.y) - sgn(xm.y - v.y)) + (sgn(v.y - yp.y) - sgn(ym.y - v.y)));
        if (VALUE) val += gamma * invV * (fabsf(zm.x - v.x) + fabsf(xm.x - v.x) + fabsf(ym.x - v.x));
        if (VALUE) val += gamma * invV * (fabsf(zm.y - v.y) + fabsf(xm.y - v.y) + fabsf(ym.y - v.y));
    }
    return gr;
}

// SET: g = regulariser gradient (replaces a zero fill + accumulate when the gradient buffer is being initialised).
// One thread per voxel (both channels, float2), threads along z (the fastest axis), blockIdx = (x, y): no integer divisions,
// every load an 8-byte coalesced access (the y / x neighbours are whole rows one plane / one row away).
// MODE 0: g += gradient; 1: g = gradient; 2: value only (g untouched)
template <int SET>
__global__ __launch_bounds__(256) void reg_grad_kernel(const float2* __restrict__ x, float2* __restrict__ g, int Y, int X, int Z,
                                                       float a_d, float a_b, float gamma, float* reg_partial) {
    const float invV = 1.0f / (float)((size_t)Y * X * Z);
    float val = 0.f;
    const RegRows r = reg_rows(blockIdx.y, blockIdx.x, Y, X, Z);
    for (int z = threadIdx.x; z < Z; z += blockDim.x) {
        const float2 gr = reg_stencil<true>(x, r, z, Z, a_d, a_b, gamma, invV, val);
        if (SET == 1) g[r.row + z] = gr;
        else if (SET == 0) { float2 o = g[r.row + z]; o.x += gr.x; o.y += gr.y; g[r.row + z] = o; }
    }
    if (reg_partial) {
        // one partial per (y, x) row, summed in a fixed order by reg_value_reduce_kernel: 65 536 atomics on ONE address
        // serialise at the memory side and made this kernel 6x slower (0.84 instead of 0.13 ms at 256^3)
        __shared__ float red[4];
        const float t = block_sum_f32(val, red, (int)(blockDim.x >> 6));
        if (threadIdx.x == 0) reg_partial[(size_t)blockIdx.y * gridDim.x + blockIdx.x] = t;
    }
}

// The same gradient for the flat fp32 elements [lo, hi) of the object only (a rank's shard of a sharded update), ADDED where the
// element lies in [add_lo, add_hi) and WRITTEN elsewhere: the footprint-restricted exchange reduces the data term over the planes
// the global batch touched and leaves everything else of the gradient buffer undefined -- the regulariser term, the same on every
// rank, is put in afterwards by the owner with R-fold weights.  blockIdx.y counts planes from y0.
__global__ __launch_bounds__(256) void reg_grad_range_kernel(const float2* __restrict__ x, float* __restrict__ g, int Y, int X, int Z,
                                                             float a_d, float a_b, float gamma, int y0, size_t lo, size_t hi, size_t add_lo,
                                                             size_t add_hi) {
    const float invV = 1.0f / (float)((size_t)Y * X * Z);
    float unused = 0.f;
    const RegRows r = reg_rows(y0 + blockIdx.y, blockIdx.x, Y, X, Z);
    for (int z = threadIdx.x; z < Z; z += blockDim.x) {
        const size_t e = 2 * (r.row + z);
        if (e + 1 < lo || e >= hi) continue;
        const float2 gr = reg_stencil<false>(x, r, z, Z, a_d, a_b, gamma, invV, unused);
        if (e >= lo && e < hi) g[e] = (e >= add_lo && e < add_hi) ? g[e] + gr.x : gr.x;
        if (e + 1 >= lo && e + 1 < hi) g[e + 1] = (e + 1 >= add_lo && e + 1 < add_hi) ? g[e + 1] + gr.y : gr.y;
    }
}

// *out += sum(partial[0..n)) in a fixed order (one block)
__global__ __launch_bounds__(1024) void reg_value_reduce_kernel(const float* __restrict__ partial, int n, float* out) {
    __shared__ float red[16];
    float acc = 0.f;
    for (int i = threadIdx.x; i < n; i += 1024) acc += partial[i];
    const float t = block_sum_f32(acc, red, 16);
    if (threadIdx.x == 0) *out += t;
}

// real_imag branches (adorym/regularizers.py:38-45, 105-110): the regularised quantities are u = re^2 + im^2 (TV),
// |o| = sqrt(u) (L1, about its mean) and phi = atan2(im, re) (TV and L1); chain rule back to (re, im).
// stats[0] = sum |o|, stats[1] = sum sgn(|o| - mean|o|) (filled by the two pre-passes when alpha_d != 0).
// wgt (reweighted L1, adorym/regularizers.py:73-82): the sign sum of pass 1 is weighted with wm = w_re^2 + w_im^2 per voxel.
__global__ __launch_bounds__(256) void ri_stats_kernel(const float2* __restrict__ x, size_t V, float* stats, int pass,
                                                       const float2* __restrict__ wgt = nullptr) {
    float acc = 0.f;
    const float mean = pass ? stats[0] / (float)V : 0.f;
    for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < V; i += (size_t)gridDim.x * blockDim.x) {
        const float2 o = x[i];
        const float om = sqrtf(o.x * o.x + o.y * o.y);
        float wm = 1.f;
        if (wgt && pass) { const float2 w = wgt[i]; wm = w.x * w.x + w.y * w.y; }
        acc += pass ? wm * sgn(om - mean) : om;
    }
    __shared__ float red[4];
    const float t = block_sum_f32(acc, red, 4);
    if (threadIdx.x == 0) atomicAdd(stats + pass, t);
}

__device__ __forceinline__ void ri_up(const float2* __restrict__ x, size_t i, float& u, float& ph) {
    const float2 o = x[i];
    u = o.x * o.x + o.y * o.y;
    ph = atan2f(o.y, o.x);
}

__global__ __launch_bounds__(256) void reg_grad_ri_kernel(const float2* __restrict__ x, float2* __restrict__ g, int Y, int X, int Z,
                                                          float a_d, float a_b, float gamma, const float* __restrict__ stats,
                                                          float* reg_value, int set) {
    const size_t V = (size_t)Y * X * Z;
    const float invV = 1.0f / (float)V;
    float val = 0.f;
    const float mean_om = (a_d != 0.f) ? stats[0] * invV : 0.f;
    const float mean_sg = (a_d != 0.f) ? stats[1] * invV : 0.f;
    for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < V; i += (size_t)gridDim.x * blockDim.x) {
        size_t vox = i;
        const int z = (int)(vox % Z);
        vox /= Z;
        const int xx = (int)(vox % X);
        const int y = (int)(vox / X);
        const float2 o = x[i];
        const float u = o.x * o.x + o.y * o.y;
        const float ph = atan2f(o.y, o.x);
        float gr = 0.f, gi = 0.f;
        if (a_d != 0.f) {
            const float om = sqrtf(u);
            const float dev = om - mean_om;
            const float gom = a_d * (sgn(dev) - mean_sg) * invV;
            gr += gom * o.x / om;
            gi += gom * o.y / om;
            val += a_d * fabsf(dev) * invV;
        }
        if (a_b != 0.f) {
            const float gph = a_b * sgn(ph) * invV;
            gr += -gph * o.y / u;
            gi += gph * o.x / u;
            val += a_b * fabsf(ph) * invV;
        }
        if (gamma != 0.f) {
            const size_t sz = 1, sx = (size_t)Z, sy = (size_t)Z * X;
            float um, pm, up, pp, gu = 0.f, gp = 0.f;
            ri_up(x, i - (size_t)z * sz + (size_t)((z + Z - 1) % Z) * sz, um, pm);
            ri_up(x, i - (size_t)z * sz + (size_t)((z + 1) % Z) * sz, up, pp);
            gu += sgn(u - up) - sgn(um - u); gp += sgn(ph - pp) - sgn(pm - ph);
            val += gamma * invV * (fabsf(um - u) + fabsf(pm - ph));
            ri_up(x, i - (size_t)xx * sx + (size_t)((xx + X - 1) % X) * sx, um, pm);
            ri_up(x, i - (size_t)xx * sx + (size_t)((xx + 1) % X) * sx, up, pp);
            gu += sgn(u - up) - sgn(um - u); gp += sgn(ph - pp) - sgn(pm - ph);
            val += gamma * invV * (fabsf(um - u) + fabsf(pm - ph));
            ri_up(x, i - (size_t)y * sy + (size_t)((y + Y - 1) % Y) * sy, um, pm);
            ri_up(x, i - (size_t)y * sy + (size_t)((y + 1) % Y) * sy, up, pp);
            gu += sgn(u - up) - sgn(um - u); gp += sgn(ph - pp) - sgn(pm - ph);
            val += gamma * invV * (fabsf(um - u) + fabsf(pm - ph));
            gr += gamma * invV * (gu * 2.f * o.x - gp * o.y / u);
            gi += gamma * invV * (gu * 2.f * o.y + gp * o.x / u);
        }
        float2 gv = set ? make_float2(0.f, 0.f) : g[i];
        gv.x += gr;
        gv.y += gi;
        g[i] = gv;
    }
    if (reg_value) {
        __shared__ float red[4];
        const float t = block_sum_f32(val, red, 4);
        if (threadIdx.x == 0) atomicAdd(reg_value, t);
    }
}

// Reweighted L1 for complex-transmission unknowns (adorym/regularizers.py:73-82): with wm = w_re^2 + w_im^2 (constants),
//   alpha_d * mean(wm * | |o| - mean|o| |) + alpha_b * mean(wm * |atan2(im, re)|);   stats as in reg_grad_ri_kernel, the
// sign sum weighted.  g += gradient w.r.t. (re, im); value added to *reg_value.
__global__ __launch_bounds__(256) void reg_grad_ri_weighted_kernel(const float2* __restrict__ x, const float2* __restrict__ wgt,
                                                                   float2* __restrict__ g, size_t V, float a_d, float a_b,
                                                                   const float* __restrict__ stats, float* reg_value) {
    const float invV = 1.0f / (float)V;
    float val = 0.f;
    const float mean_om = (a_d != 0.f) ? stats[0] * invV : 0.f;
    const float mean_sg = (a_d != 0.f) ? stats[1] * invV : 0.f;
    for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < V; i += (size_t)gridDim.x * blockDim.x) {
        const float2 o = x[i];
        const float2 w = wgt[i];
        const float wm = w.x * w.x + w.y * w.y;
        const float u = o.x * o.x + o.y * o.y;
        float gr = 0.f, gi = 0.f;
        if (a_d != 0.f) {
            const float om = sqrtf(u);
            const float dev = om - mean_om;
            const float gom = a_d * (wm * sgn(dev) - mean_sg) * invV;
            gr += gom * o.x / om;
            gi += gom * o.y / om;
            val += a_d * wm * fabsf(dev) * invV;
        }
        if (a_b != 0.f) {
            const float ph = atan2f(o.y, o.x);
            const float gph = a_b * wm * sgn(ph) * invV;
            gr += -gph * o.y / u;
            gi += gph * o.x / u;
            val += a_b * wm * fabsf(ph) * invV;
        }
        float2 gv = g[i];
        gv.x += gr;
        gv.y += gi;
        g[i] = gv;
    }
    if (reg_value) {
        __shared__ float red[4];
        const float t = block_sum_f32(val, red, 4);
        if (threadIdx.x == 0) atomicAdd(reg_value, t);
    }
}

// reweighted L1: block partials of (max, sum) -> final scalars -> weights
__global__ __launch_bounds__(256) void rwl1_partial_kernel(const float* __restrict__ x, size_t n, float* __restrict__ part) {
    float mx = -3.4e38f;
    double sm = 0.0;
    for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (size_t)gridDim.x * blockDim.x) {
        const float v = x[i];
        mx = fmaxf(mx, v);
        sm += (double)v;
    }
    __shared__ float smx[256];
    __shared__ double ssm[256];
    smx[threadIdx.x] = mx; ssm[threadIdx.x] = sm;
    __syncthreads();
    for (int o = 128; o > 0; o >>= 1) {
        if (threadIdx.x < o) { smx[threadIdx.x] = fmaxf(smx[threadIdx.x], smx[threadIdx.x + o]); ssm[threadIdx.x] += ssm[threadIdx.x + o]; }
        __syncthreads();
    }
    if (threadIdx.x == 0) { part[2 * blockIdx.x] = smx[0]; part[2 * blockIdx.x + 1] = (float)(ssm[0] / (double)n); }
}
__global__ void rwl1_final_kernel(float* part, int nblocks) {
    if (threadIdx.x == 0 && blockIdx.x == 0) {
        float mx = -3.4e38f; double mean = 0.0;
        for (int b = 0; b < nblocks; ++b) { mx = fmaxf(mx, part[2 * b]); mean += (double)part[2 * b + 1]; }
        part[2 * nblocks] = mx; part[2 * nblocks + 1] = (float)mean;
    }
}
__global__ __launch_bounds__(256) void rwl1_weight_kernel(const float* __restrict__ x, float* __restrict__ w, size_t n,
                                                          const float* __restrict__ scal) {
    const float mx = scal[0], off = 1e-4f * scal[1];
    for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (size_t)gridDim.x * blockDim.x)
        w[i] = mx / (fabsf(x[i]) + off);
}
// The value goes through a double: w = max / (|x| + off) makes every term w * |x| nearly the same number, so the block sums are
// nearly equal and up to 4096 float atomic adds of one addend round the same way every time (2.749612 for 2.749665 at
// 4 x 1030 x 257 voxels, 1.9e-5).  The blocks add their sums to *acc (zeroed by the caller), reg_value_add_kernel rounds once.
__global__ void reg_value_add_kernel(const double* __restrict__ acc, float* out) {
    if (threadIdx.x == 0 && blockIdx.x == 0) *out += (float)*acc;
}
__global__ __launch_bounds__(256) void reg_grad_weighted_kernel(const float* __restrict__ x, const float* __restrict__ w,
                                                                float* __restrict__ g, size_t n, float a_d, float a_b,
                                                                float invV, double* reg_value) {
    float val = 0.f;
    for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (size_t)gridDim.x * blockDim.x) {
        const float al = (i & 1) ? a_b : a_d;
        const float v = x[i], wi = w[i];
        g[i] += al * wi * sgn(v) * invV;
        val += al * wi * fabsf(v) * invV;
    }
    if (reg_value) {
        __shared__ float red[4];
        const float t = block_sum_f32(val, red, 4);
        if (threadIdx.x == 0) atomicAdd(reg_value, (double)t);
    }
}
}  // namespace adm
using namespace adm;

// threads of a block of reg_grad_kernel / reg_grad_range_kernel (one z row of a delta_beta object)
static inline int reg_threads(int obj_z) { return obj_z >= 192 ? 256 : (obj_z >= 96 ? 128 : 64); }
// plan->reg_stats (allocated on first use) = the two sums of ri_stats_kernel over a real_imag object of V voxels
static int ri_stats_launch(adm_plan* plan, const float2* obj, size_t V, const float2* wgt) {
    hipStream_t st = plan->ctx->stream;
    if (!plan->reg_stats) ADM_HIP(hipMalloc((void**)&plan->reg_stats, 2 * sizeof(float)));
    ADM_HIP(hipMemsetAsync(plan->reg_stats, 0, 2 * sizeof(float), st));
    int nb = stream_grid(V);
    if (nb > 1024) nb = 1024;
    hipLaunchKernelGGL(ri_stats_kernel, dim3(nb), dim3(256), 0, st, obj, V, plan->reg_stats, 0, wgt);
    hipLaunchKernelGGL(ri_stats_kernel, dim3(nb), dim3(256), 0, st, obj, V, plan->reg_stats, 1, wgt);
    return ADM_OK;
}

static int reg_grad_impl(adm_plan* plan, const float* obj, float alpha_d, float alpha_b, float gamma, float* grad_obj,
                         float* reg_value, bool set) {
    if (!plan || !obj || (!grad_obj && !reg_value)) return fail(ADM_ERR_INVALID, "adm_reg_grad: null argument");
    if (!grad_obj && plan->d.unknown_type == 1) return fail(ADM_ERR_UNSUPPORTED, "adm_reg_grad: value-only evaluation is built for delta_beta unknowns");
    const adm_plan_desc& d = plan->d;
    const size_t n = (size_t)d.obj_y * d.obj_x * d.obj_z * 2;
    hipStream_t st = plan->ctx->stream;
    if (d.unknown_type == 1) {
        const size_t V = n / 2;
        const int rc = alpha_d != 0.f ? ri_stats_launch(plan, (const float2*)obj, V, (const float2*)nullptr) : ADM_OK;
        if (rc) return rc;
        hipLaunchKernelGGL(reg_grad_ri_kernel, dim3(stream_grid(V)), dim3(256), 0, st, (const float2*)obj, (float2*)grad_obj, d.obj_y,
                           d.obj_x, d.obj_z, alpha_d, alpha_b, gamma, (const float*)plan->reg_stats, reg_value, set ? 1 : 0);
        ADM_HIP(hipGetLastError());
        return ADM_OK;
    }
    const int nt = reg_threads(d.obj_z);
    const dim3 grid(d.obj_x, d.obj_y);
    float* partial = nullptr;
    if (reg_value) {
        if (!plan->reg_partial) ADM_HIP(hipMalloc((void**)&plan->reg_partial, (size_t)d.obj_x * d.obj_y * sizeof(float)));
        partial = plan->reg_partial;
    }
    if (!grad_obj)
        hipLaunchKernelGGL(reg_grad_kernel<2>, grid, dim3(nt), 0, st, (const float2*)obj, (float2*)nullptr, d.obj_y, d.obj_x, d.obj_z,
                           alpha_d, alpha_b, gamma, partial);
    else if (set)
        hipLaunchKernelGGL(reg_grad_kernel<1>, grid, dim3(nt), 0, st, (const float2*)obj, (float2*)grad_obj, d.obj_y, d.obj_x, d.obj_z,
                           alpha_d, alpha_b, gamma, partial);
    else
        hipLaunchKernelGGL(reg_grad_kernel<0>, grid, dim3(nt), 0, st, (const float2*)obj, (float2*)grad_obj, d.obj_y, d.obj_x, d.obj_z,
                           alpha_d, alpha_b, gamma, partial);
    if (reg_value)
        hipLaunchKernelGGL(reg_value_reduce_kernel, dim3(1), dim3(1024), 0, st, (const float*)partial, d.obj_x * d.obj_y, reg_value);
    ADM_HIP(hipGetLastError());
    return ADM_OK;
}

extern "C" int adm_reg_grad(adm_plan* plan, const float* obj, float alpha_d, float alpha_b, float gamma, float* grad_obj,
                            float* reg_value) {
    return reg_grad_impl(plan, obj, alpha_d, alpha_b, gamma, grad_obj, reg_value, false);
}

extern "C" int adm_reg_grad_set(adm_plan* plan, const float* obj, float alpha_d, float alpha_b, float gamma, float* grad_obj,
                                float* reg_value) {
    return reg_grad_impl(plan, obj, alpha_d, alpha_b, gamma, grad_obj, reg_value, true);
}

extern "C" int adm_reg_grad_range(adm_plan* plan, const float* obj, float alpha_d, float alpha_b, float gamma, float* grad_obj,
                                  size_t lo, size_t hi, size_t add_lo, size_t add_hi) {
    if (!plan || !obj || !grad_obj) return fail(ADM_ERR_INVALID, "adm_reg_grad_range: null argument");
    const adm_plan_desc& d = plan->d;
    if (d.unknown_type != 0) return fail(ADM_ERR_UNSUPPORTED, "adm_reg_grad_range: built for delta_beta unknowns");
    const size_t n = (size_t)d.obj_y * d.obj_x * d.obj_z * 2, plane = (size_t)d.obj_x * d.obj_z * 2;
    if (hi > n) hi = n;
    if (lo >= hi) return ADM_OK;
    const int y0 = (int)(lo / plane), y1 = (int)((hi + plane - 1) / plane);
    const int nt = reg_threads(d.obj_z);
    hipLaunchKernelGGL(reg_grad_range_kernel, dim3(d.obj_x, y1 - y0), dim3(nt), 0, plan->ctx->stream, (const float2*)obj, grad_obj, d.obj_y,
                       d.obj_x, d.obj_z, alpha_d, alpha_b, gamma, y0, lo, hi, add_lo, add_hi);
    ADM_HIP(hipGetLastError());
    return ADM_OK;
}

extern "C" int adm_rwl1_update(adm_plan* plan, const float* obj, float* weight, float* scratch) {
    if (!plan || !obj || !weight || !scratch) return fail(ADM_ERR_INVALID, "adm_rwl1_update: null argument");
    const adm_plan_desc& d = plan->d;
    const size_t n = (size_t)d.obj_y * d.obj_x * d.obj_z * 2;
    int nb = stream_grid(n);
    if (nb > 1024) nb = 1024;
    hipStream_t st = plan->ctx->stream;
    hipLaunchKernelGGL(rwl1_partial_kernel, dim3(nb), dim3(256), 0, st, obj, n, scratch);
    hipLaunchKernelGGL(rwl1_final_kernel, dim3(1), dim3(64), 0, st, scratch, nb);
    hipLaunchKernelGGL(rwl1_weight_kernel, dim3(stream_grid(n)), dim3(256), 0, st, obj, weight, n, (const float*)(scratch + 2 * nb));
    ADM_HIP(hipGetLastError());
    return ADM_OK;
}

extern "C" int adm_reg_grad_weighted(adm_plan* plan, const float* obj, const float* weight, float alpha_d, float alpha_b,
                                     float* grad_obj, float* reg_value) {
    if (!plan || !obj || !weight || !grad_obj) return fail(ADM_ERR_INVALID, "adm_reg_grad_weighted: null argument");
    const adm_plan_desc& d = plan->d;
    const size_t n = (size_t)d.obj_y * d.obj_x * d.obj_z * 2;
    if (d.unknown_type == 1) {          // real_imag (adorym/regularizers.py:73-82)
        const size_t V = n / 2;
        hipStream_t st = plan->ctx->stream;
        const int rc = alpha_d != 0.f ? ri_stats_launch(plan, (const float2*)obj, V, (const float2*)weight) : ADM_OK;
        if (rc) return rc;
        hipLaunchKernelGGL(reg_grad_ri_weighted_kernel, dim3(stream_grid(V)), dim3(256), 0, st, (const float2*)obj, (const float2*)weight,
                           (float2*)grad_obj, V, alpha_d, alpha_b, (const float*)plan->reg_stats, reg_value);
        ADM_HIP(hipGetLastError());
        return ADM_OK;
    }
    hipStream_t st = plan->ctx->stream;
    double* acc = nullptr;
    if (reg_value) {                    // plan->reg_stats: 8 bytes, which a delta_beta plan uses for nothing else
        if (!plan->reg_stats) ADM_HIP(hipMalloc((void**)&plan->reg_stats, 2 * sizeof(float)));
        acc = (double*)plan->reg_stats;
        ADM_HIP(hipMemsetAsync(acc, 0, sizeof(double), st));
    }
    hipLaunchKernelGGL(reg_grad_weighted_kernel, dim3(stream_grid(n)), dim3(256), 0, st, obj, weight, grad_obj, n,
                       alpha_d, alpha_b, 1.0f / (float)(n / 2), acc);
    if (reg_value) hipLaunchKernelGGL(reg_value_add_kernel, dim3(1), dim3(64), 0, st, (const double*)acc, reg_value);
    ADM_HIP(hipGetLastError());
    return ADM_OK;
}
