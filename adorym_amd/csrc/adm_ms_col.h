// The column workgroups of the streamed multislice path, defined once for the translation units that launch them
// (adm_ms_streamed.hip, adm_ms_exitshift.hip, adm_ms_probeshift.hip, adm_ms_multidist.hip, adm_ms_distgrad.hip): how many adjacent columns a workgroup takes, its threads and
// its LDS (st_col_geom, the one place where the launch geometry is computed), the LDS context and the load / store / transform
// helpers of the kernels, fftfreq, and the fp64 workgroup sum of the gradient partials.
#pragma once
#include <hip/hip_runtime.h>
#include "adm_common.h"
#include "adm_fft.h"
#include "adm_ms_math.h"
#include "adm_ms_gen.h"

namespace adm {

constexpr int ST_COL_NT = 512;                 // most threads of a column workgroup (GEN_E elements each)
// adjacent columns of a column workgroup: 8 (64-byte runs per row) up to Py = 1024, 4 at larger Py (the group is at most
// ST_COL_NT * GEN_E elements: with more threads the detector kernel's per-element state no longer fits the registers)
__host__ __device__ __forceinline__ int st_cw(int py) { return py <= ST_COL_NT * GEN_E / 8 ? 8 : 4; }

// column transform passes of the line group in LDS (INV: conjugate twiddles)
template <bool INV> __device__ __forceinline__ void st_col_fft(const GenCtx& g, const MsParams& p, cf (&v)[GEN_E]) {
    int Ns = 1;
    for (int s = 0; s < p.gen_nry; ++s) { gen_pass<true, INV>(g, p.gen_ry[s], Ns, v); Ns *= p.gen_ry[s]; }
}

// LDS of a column workgroup: the [Py][cw] group, then W_Py^j
__device__ __forceinline__ void st_col_ctx(GenCtx& g, cf* lds, const MsParams& p, int c0, int cw) {
    g.Py = p.gen_py; g.Px = min(cw, p.gen_px - c0); g.n = g.Py * g.Px;
    g.tid = threadIdx.x; g.nt = blockDim.x;
    g.ne = (g.n + g.nt - 1) / g.nt;
    g.fld = lds;
    cf* twy = lds + (size_t)g.Py * cw;
    for (int i = g.tid; i < g.Py; i += g.nt) twy[i] = p.gen_twid_y[i];
    g.twx = nullptr; g.twy = twy;
}
__device__ __forceinline__ void st_col_load(const GenCtx& g, const float2* f, int Px, int c0) {
    for (int i = g.tid; i < g.n; i += g.nt) {
        const int y = i / g.Px;
        g.fld[i] = f[(size_t)y * Px + c0 + (i - y * g.Px)];
    }
}
__device__ __forceinline__ void st_col_store(const GenCtx& g, float2* f, int Px, int c0) {
    for (int i = g.tid; i < g.n; i += g.nt) {
        const int y = i / g.Px;
        f[(size_t)y * Px + c0 + (i - y * g.Px)] = g.fld[i];
    }
}

// fftfreq(n)[i] * n
__device__ __forceinline__ int st_freq_index(int i, int n) { return i <= (n - 1) / 2 ? i : i - n; }
// fftfreq(n, 1)[i], one rounding (fftfreq_f of adm_multislice.hip)
__device__ __forceinline__ float st_freq(int i, int n) { return (float)((double)st_freq_index(i, n) / (double)n); }

// N fp64 sums over the workgroup, always in the same order: the caller's per-thread sums in acc, __shfl_down over the 64 lanes,
// the wave leaders write red[waves][N] (LDS, ST_COL_NT / 64 waves at most), and thread 0 adds the waves in ascending order: with
// `want`, acc holds the totals on thread 0 afterwards (and nothing of use on the others).  The barrier in the middle runs on every
// thread whether or not sums are wanted: in the column kernels it is also the barrier between their element-wise LDS writes and
// the inverse column transform that follows.
template <int N> __device__ __forceinline__ void st_block_sum_f64(double (&acc)[N], double* red, int tid, int nt, bool want) {
    if (want) {
#pragma unroll
        for (int off = 32; off > 0; off >>= 1) {
#pragma unroll
            for (int k = 0; k < N; ++k) acc[k] += __shfl_down(acc[k], off, 64);
        }
        if ((tid & 63) == 0) {
#pragma unroll
            for (int k = 0; k < N; ++k) red[N * (tid >> 6) + k] = acc[k];
        }
    }
    __syncthreads();
    if (want && tid == 0) {
#pragma unroll
        for (int k = 0; k < N; ++k) acc[k] = 0.0;
        for (int w = 0; w < (nt >> 6); ++w) {
#pragma unroll
            for (int k = 0; k < N; ++k) acc[k] += red[N * w + k];
        }
    }
}

// threads of a column workgroup: GEN_E elements each, whole waves, at least 256
inline int st_col_threads(int py) {
    const int n = py * st_cw(py);
    int nt = ((n + GEN_E - 1) / GEN_E + 63) / 64 * 64;
    if (nt < 256) nt = 256;
    return nt;
}

// the launch of column workgroups over fields of Py x Px: one workgroup per column group of every (position, mode)
struct StColGeom {
    int cw;            // adjacent columns per workgroup
    int ncg;           // column groups of a field
    int threads;
    size_t lds;        // dynamic LDS bytes: the [Py][cw] group and W_Py^j
};
inline StColGeom st_col_geom(int Py, int Px) {
    StColGeom c;
    const int cw = st_cw(Py);
    c.cw = cw; c.ncg = (Px + cw - 1) / cw; c.threads = st_col_threads(Py);
    c.lds = ((size_t)Py * cw + Py) * sizeof(float2);
    return c;
}

// lets a column kernel take the LDS of the largest group (each translation unit does this once for its own kernels)
template <class Kernel> inline hipError_t st_col_raise_lds(Kernel kernel) {
    return hipFuncSetAttribute(reinterpret_cast<const void*>(kernel), hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024 - 256);
}

}  // namespace adm
