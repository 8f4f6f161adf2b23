// Projection approximation (adorym/propagate.py:158-193, pure_projection=True): the rotated object summed along the beam, and the
// transpose of that sum.  Both kernels stream: the rows [y_lo, y_hi) of one slice of a rotated-frame buffer [Z][Yp][Xp][2] are ONE
// contiguous run of (y_hi - y_lo) * Xp pixels, Z such runs lie Yp * Xp pixels apart, and the one-slice image is a single run.
//
//   adm_project_z      proj[run]      = round_fp32(sum over z of obj_rot[z][run]), the sum kept in double
//   adm_project_z_adj  grad_rot[z][run] = grad_proj[run] for every z
//
// A thread owns a UNIT of W pixels (W = 2: one 16-byte access, where the runs start on 16-byte boundaries in every slice; else W = 1).
// A run of uneven length ends in a unit of one pixel.
#include "adm_host.h"

namespace adm {
#define PRJ_LANES 64      // units per workgroup of the sum: one wave along the run, blockDim.y waves along z
#define PRJ_DEPTH 8       // loads a thread of the sum keeps in flight

struct PrjGeom {
    size_t start;         // first pixel of the run inside a slice: (pad_y0 + y_lo) * Xp
    size_t slice;         // pixels per slice: Yp * Xp
    size_t n_pix;         // pixels of the run: (y_hi - y_lo) * Xp
    int Z;
};

template <int W> struct PrjUnit;
template <> struct PrjUnit<1> { typedef float2 T; };
template <> struct PrjUnit<2> { typedef float4 T; };

// the unit at pixel p of a run; `whole`: all W pixels lie inside the run (W = 2 only: else the first alone)
template <int W>
__device__ __forceinline__ typename PrjUnit<W>::T prj_load(const float2* p, bool whole);
template <>
__device__ __forceinline__ float2 prj_load<1>(const float2* p, bool) { return *p; }
template <>
__device__ __forceinline__ float4 prj_load<2>(const float2* p, bool whole) {
    if (whole) return *(const float4*)p;
    const float2 v = *p;
    return make_float4(v.x, v.y, 0.f, 0.f);
}
__device__ __forceinline__ void prj_store(float2* p, float2 v, bool) { *p = v; }
__device__ __forceinline__ void prj_store(float2* p, float4 v, bool whole) {
    if (whole) *(float4*)p = v;
    else *p = make_float2(v.x, v.y);
}
__device__ __forceinline__ void prj_add(double* a, float2 v) { a[0] += (double)v.x; a[1] += (double)v.y; }
__device__ __forceinline__ void prj_add(double* a, float4 v) {
    a[0] += (double)v.x; a[1] += (double)v.y; a[2] += (double)v.z; a[3] += (double)v.w;
}
__device__ __forceinline__ void prj_round(const double* a, float2& v) { v = make_float2((float)a[0], (float)a[1]); }
__device__ __forceinline__ void prj_round(const double* a, float4& v) { v = make_float4((float)a[0], (float)a[1], (float)a[2], (float)a[3]); }

// Workgroup = PRJ_LANES units x TZ waves.  Wave t adds the slices t, t + TZ, t + 2 TZ, ... of its units in that order, PRJ_DEPTH
// independent loads ahead of the additions; the TZ partial sums of a unit meet in LDS and wave 0 adds them t = 0, 1, ... and rounds
// once.  No atomics: the bits depend on (Z, TZ) only, and TZ is a function of the call's arguments.
template <int W>
__global__ void __launch_bounds__(1024) project_z_kernel(const float2* __restrict__ rot, float2* __restrict__ proj, PrjGeom g) {
    typedef typename PrjUnit<W>::T T;
    extern __shared__ double prj_part[];                  // [TZ][PRJ_LANES][2 W]
    const int lane = threadIdx.x, t = threadIdx.y, TZ = blockDim.y;
    const size_t pix = ((size_t)blockIdx.x * PRJ_LANES + lane) * W;
    const bool live = pix < g.n_pix;
    const bool whole = pix + W <= g.n_pix;
    double acc[2 * W];
#pragma unroll
    for (int k = 0; k < 2 * W; ++k) acc[k] = 0.0;
    if (live) {
        const float2* src = rot + g.start + pix;
        int z = t;
        for (; z + (PRJ_DEPTH - 1) * TZ < g.Z; z += PRJ_DEPTH * TZ) {
            T v[PRJ_DEPTH];
#pragma unroll
            for (int i = 0; i < PRJ_DEPTH; ++i) v[i] = prj_load<W>(src + (size_t)(z + i * TZ) * g.slice, whole);
#pragma unroll
            for (int i = 0; i < PRJ_DEPTH; ++i) prj_add(acc, v[i]);
        }
        for (; z < g.Z; z += TZ) prj_add(acc, prj_load<W>(src + (size_t)z * g.slice, whole));
    }
    double* mine = prj_part + ((size_t)t * PRJ_LANES + lane) * (2 * W);
#pragma unroll
    for (int k = 0; k < 2 * W; ++k) mine[k] = acc[k];
    __syncthreads();
    if (t != 0 || !live) return;
    for (int u = 1; u < TZ; ++u) {
        const double* other = prj_part + ((size_t)u * PRJ_LANES + lane) * (2 * W);
#pragma unroll
        for (int k = 0; k < 2 * W; ++k) acc[k] += other[k];
    }
    T out;
    prj_round(acc, out);
    prj_store(proj + g.start + pix, out, whole);
}

#define PRJ_ADJ_SLICES 8  // slices a workgroup of the broadcast writes with the unit it loaded once

// Workgroup = 256 units x PRJ_ADJ_SLICES slices: every thread loads its unit once and stores it to the slices of blockIdx.y's group;
// a wave's store is 1 KiB (W = 2) of one slice's run.
template <int W>
__global__ void __launch_bounds__(256) project_z_adj_kernel(const float2* __restrict__ gproj, float2* __restrict__ grot, PrjGeom g) {
    typedef typename PrjUnit<W>::T T;
    const size_t pix = ((size_t)blockIdx.x * 256 + threadIdx.x) * W;
    if (pix >= g.n_pix) return;
    const bool whole = pix + W <= g.n_pix;
    const T v = prj_load<W>(gproj + g.start + pix, whole);
    float2* dst = grot + g.start + pix;
    const int z0 = blockIdx.y * PRJ_ADJ_SLICES;
#pragma unroll
    for (int i = 0; i < PRJ_ADJ_SLICES; ++i)
        if (z0 + i < g.Z) prj_store(dst + (size_t)(z0 + i) * g.slice, v, whole);
}

static int prj_geom(const adm_plan* plan, int y_lo, int y_hi, const char* who, PrjGeom* g) {
    const adm_plan_desc& d = plan->d;
    if (y_lo < 0 || y_hi > d.obj_y || y_lo > y_hi) return fail(ADM_ERR_INVALID, std::string(who) + ": bad y range");
    g->start = (size_t)(d.pad_y0 + y_lo) * plan->Xp;
    g->slice = (size_t)plan->Yp * plan->Xp;
    g->n_pix = (size_t)(y_hi - y_lo) * plan->Xp;
    g->Z = d.obj_z;
    return ADM_OK;
}
// 16-byte units where the run starts on a 16-byte boundary in every slice (device allocations are aligned far beyond that)
static bool prj_wide(const PrjGeom& g, const void* a, const void* b) {
    return g.start % 2 == 0 && g.slice % 2 == 0 && ((uintptr_t)a | (uintptr_t)b) % 16 == 0;
}
}  // namespace adm
using namespace adm;

extern "C" int adm_project_z(adm_plan* plan, const float* obj_rot, int y_lo, int y_hi, float* proj) {
    if (!plan || !obj_rot || !proj) return fail(ADM_ERR_INVALID, "adm_project_z: null argument");
    PrjGeom g;
    if (const int rc = prj_geom(plan, y_lo, y_hi, "adm_project_z", &g)) return rc;
    if (g.n_pix == 0) return ADM_OK;
    const int W = prj_wide(g, obj_rot, proj) ? 2 : 1;
    const size_t blocks = (g.n_pix + (size_t)W * PRJ_LANES - 1) / ((size_t)W * PRJ_LANES);
    // waves along z: 4, or 16 where 4 would leave the chip short of waves (a minibatch's few rows) and the object is deep enough to
    // give every wave a full round of loads; never more than slices
    int tz = (blocks < 1024 && g.Z >= 16 * PRJ_DEPTH) ? 16 : 4;
    while (tz > 1 && tz > g.Z) tz >>= 1;
    const size_t lds = (size_t)tz * PRJ_LANES * 2 * W * sizeof(double);
    if (W == 2)
        hipLaunchKernelGGL(project_z_kernel<2>, dim3((unsigned)blocks), dim3(PRJ_LANES, tz), lds, plan->ctx->stream, (const float2*)obj_rot,
                           (float2*)proj, g);
    else
        hipLaunchKernelGGL(project_z_kernel<1>, dim3((unsigned)blocks), dim3(PRJ_LANES, tz), lds, plan->ctx->stream, (const float2*)obj_rot,
                           (float2*)proj, g);
    ADM_HIP(hipGetLastError());
    return ADM_OK;
}

extern "C" int adm_project_z_adj(adm_plan* plan, const float* grad_proj, int y_lo, int y_hi, float* grad_rot) {
    if (!plan || !grad_proj || !grad_rot) return fail(ADM_ERR_INVALID, "adm_project_z_adj: null argument");
    PrjGeom g;
    if (const int rc = prj_geom(plan, y_lo, y_hi, "adm_project_z_adj", &g)) return rc;
    if (g.n_pix == 0) return ADM_OK;
    const int W = prj_wide(g, grad_proj, grad_rot) ? 2 : 1;
    const dim3 grid((unsigned)((g.n_pix + (size_t)W * 256 - 1) / ((size_t)W * 256)), (unsigned)((g.Z + PRJ_ADJ_SLICES - 1) / PRJ_ADJ_SLICES));
    if (W == 2)
        hipLaunchKernelGGL(project_z_adj_kernel<2>, grid, dim3(256), 0, plan->ctx->stream, (const float2*)grad_proj, (float2*)grad_rot, g);
    else
        hipLaunchKernelGGL(project_z_adj_kernel<1>, grid, dim3(256), 0, plan->ctx->stream, (const float2*)grad_proj, (float2*)grad_rot, g);
    ADM_HIP(hipGetLastError());
    return ADM_OK;
}
