// The column workgroups of the streamed multislice path, defined once for the translation units that launch them
// (adm_ms_streamed.hip, adm_ms_exitshift.hip, adm_ms_probeshift.hip, adm_ms_multidist.hip): how many adjacent columns a workgroup takes, its threads and
// its LDS (st_col_geom, the one place where the launch geometry is computed), the kernels' prologue (st_col_begin), LDS context and
// load / store / transform helpers, fftfreq, the phase of a sub-pixel shift, the fp64 workgroup sum of the gradient partials, and
// the launch line (st_col_launch, st_col_raise_lds_once).
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

// the start of a column kernel: which (position, mode) field -- or whatever the launch counts in its place -- and which first
// column this workgroup takes, and its LDS context (the fan kernels and the exit-shift kernel write these lines out: they say why)
struct StColWg { int bm, c0; };
__device__ __forceinline__ StColWg st_col_begin(GenCtx& g, cf* lds, const MsParams& p) {
    const int cw = st_cw(p.gen_py), ncg = (p.gen_px + cw - 1) / cw;
    StColWg w;
    w.bm = blockIdx.x / ncg; w.c0 = (blockIdx.x - w.bm * ncg) * cw;
    st_col_ctx(g, lds, p, w.c0, cw);
    return w;
}

// fftfreq(n)[i] * n
__device__ __forceinline__ int st_freq_index(int i, int n) { return i <= (n - 1) / 2 ? i : i - n; }
// fftfreq(n, 1)[i], one rounding (fftfreq_f of adm_multislice.hip)
__device__ __forceinline__ float st_freq(int i, int n) { return (float)((double)st_freq_index(i, n) / (double)n); }

// Phi = exp(-2 PI i (fx s_x + fy s_y)) at spectral element (y, x) for the offset s = (s_y, s_x), of the exit-wave shifts
// (adm_ms_exitshift.hip) and the probe shifts (adm_ms_probeshift.hip).  The argument is formed in fp64 from the integer frequency
// index, reduced to one turn, then sin / cos in fp32 (the scheme of st_fresnel_table_kernel), for two reasons:
//   * per-angle alignment exists to recover offsets of tens of pixels: the argument then reaches hundreds of radians (2000 rad at
//     640 px and an offset beyond the field), where an fp32 argument -- as the reference and shift_phases (adm_multislice.hip) form
//     it -- is 1e-4 rad off and the prediction 2.3e-5 from the fp64 model (640 x 12, tests/test_gpu_value_domain.py);
//   * at probe shifts of 2.5 px it reaches only 16 rad, where fp32 resolves 1e-6, yet that rounding alone puts dL/ds of an exit-wave
//     detector 3.4e-4 from the fp64 model, because the terms of that sum cancel to a thousandth of their size; what is left, 8e-5
//     in that case, is the fp32 rounding of the shifts themselves.
__device__ __forceinline__ cf st_shift_phase(int y, int py, int x, int px, float2 s) {
    const double fy = (double)st_freq_index(y, py) / (double)py, fx = (double)st_freq_index(x, px) / (double)px;
    double arg = -2.0 * 3.14159265359 * (fx * (double)s.y + fy * (double)s.x);
    const double two_pi = 6.283185307179586476925287;
    arg -= two_pi * rint(arg / two_pi);
    float sn, cs;
    sincos_fast((float)arg, sn, cs);
    return make_float2(cs, sn);
}

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

// lets a column kernel take the LDS of the largest group
template <class Kernel> inline hipError_t st_col_raise_lds(Kernel kernel) {
    return hipFuncSetAttribute(reinterpret_cast<const void*>(kernel), hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024 - 256);
}
// ... for every kernel a launcher may start, the first time it is called: `done` is the launcher's own function-local static
template <class... Kernels> inline hipError_t st_col_raise_lds_once(bool& done, Kernels... kernels) {
    hipError_t e = hipSuccess;
    if (!done) {
        ((e = e == hipSuccess ? st_col_raise_lds(kernels) : e), ...);
        done = e == hipSuccess;
    }
    return e;
}

// the launch of a column kernel over `groups` fields (positions * modes, as a rule): groups * cg.ncg workgroups
template <class Kernel, class... Args>
inline hipError_t st_col_launch(Kernel kernel, const StColGeom& cg, int groups, hipStream_t st, const Args&... args) {
    hipLaunchKernelGGL(kernel, dim3((unsigned)(groups * cg.ncg)), dim3((unsigned)cg.threads), cg.lds, st, args...);
    return hipGetLastError();
}

}  // namespace adm
