// Device helpers of the any-size multislice kernels: the run-time-radix line transform passes over an LDS field, the slice
// modulation and the block sum.  Shared by adm_ms_generic.hip (one workgroup per position, the whole field in LDS) and
// adm_ms_streamed.hip (line groups of fields kept in global memory).  Device-only, gfx950.
#pragma once
#include <hip/hip_runtime.h>
#include "adm_common.h"
#include "adm_fft.h"
#include "adm_ms_math.h"

namespace adm {

constexpr int GEN_E = 16;         // field elements per thread (Py*Px <= GEN_E * 1024)

struct GenCtx {
    cf* fld;            // LDS [Py*Px]
    const cf* twx;      // LDS W_Px^j
    const cf* twy;      // LDS W_Py^j
    int Py, Px, n, ne, tid, nt;
};

// one Stockham pass of radix R over every line of the field along x (ALONG_Y: along y); v = this thread's outputs
template <bool ALONG_Y, bool INV, int E = GEN_E>
__device__ __forceinline__ void gen_pass(const GenCtx& g, int R, int Ns, cf (&v)[E]) {
    const int N = ALONG_Y ? g.Py : g.Px;
    const cf* tw = ALONG_Y ? g.twy : g.twx;
    const int m = N / R;
    const int NsR = Ns * R;
    const int tstep = N / NsR;
#pragma unroll
    for (int j = 0; j < E; ++j) {
        const int i = g.tid + j * g.nt;
        if (j < g.ne && i < g.n) {
            const int y = i / g.Px, x = i - y * g.Px;
            const int o = ALONG_Y ? y : x;
            const int k = o % Ns, t = (o / Ns) % R, bq = o / NsR;
            const int jb = bq * Ns + k;
            const int base = (k * tstep + t * m) % N;
            const cf* src = ALONG_Y ? g.fld + (size_t)jb * g.Px + x : g.fld + (size_t)y * g.Px + jb;
            const int sstride = ALONG_Y ? m * g.Px : m;
            cf acc = make_float2(0.f, 0.f);
            int e = 0;
            for (int u = 0; u < R; ++u) {
                const cf a = src[(size_t)u * sstride];
                const cf w = tw[e];
                acc = INV ? cadd(acc, cmulc(a, w)) : cadd(acc, cmul(a, w));
                e += base;
                if (e >= N) e -= N;
            }
            v[j] = acc;
        }
    }
    __syncthreads();
#pragma unroll
    for (int j = 0; j < E; ++j) {
        const int i = g.tid + j * g.nt;
        if (j < g.ne && i < g.n) g.fld[i] = v[j];
    }
    __syncthreads();
}

// unnormalised 2-D transform of the LDS field, in place, natural order (INV: conjugate twiddles)
template <bool INV> __device__ __forceinline__ void gen_fft2(const GenCtx& g, const MsParams& p, cf (&v)[GEN_E]) {
    int Ns = 1;
    for (int s = 0; s < p.gen_nrx; ++s) { gen_pass<false, INV>(g, p.gen_rx[s], Ns, v); Ns *= p.gen_rx[s]; }
    Ns = 1;
    for (int s = 0; s < p.gen_nry; ++s) { gen_pass<true, INV>(g, p.gen_ry[s], Ns, v); Ns *= p.gen_ry[s]; }
}

// field <- IFFT2( H * FFT2(field) ) (CONJ: conj(H)); hs = H / (Py*Px), one rounding per element, natural order, global memory
template <bool CONJ> __device__ __forceinline__ void gen_convolve(const GenCtx& g, const MsParams& p, const float2* __restrict__ hs, cf (&v)[GEN_E]) {
    gen_fft2<false>(g, p, v);
#pragma unroll
    for (int j = 0; j < GEN_E; ++j) {
        const int i = g.tid + j * g.nt;
        if (j < g.ne && i < g.n) g.fld[i] = cmul_t<CONJ>(g.fld[i], hs[i]);
    }
    __syncthreads();
    gen_fft2<true>(g, p, v);
}

__device__ __forceinline__ cf gen_modulator(float2 db, float k1, float sigma) {
    const float e = exp_fast(-k1 * db.y);
    float sn, cs;
    sincos_fast(-sigma * k1 * db.x, sn, cs);
    return make_float2(e * cs, e * sn);
}

// (delta, beta) -- or (re, im) -- of modulation step `step` at tile pixel i (sum over the bin's slices)
__device__ __forceinline__ float2 gen_slice(const MsParams& p, const float2* __restrict__ tile, size_t slice_stride, int step, size_t pix_off) {
    const int s_lo = step * p.binning, s_hi = min(s_lo + p.binning, p.Z);
    float2 acc = make_float2(0.f, 0.f);
    for (int s = s_lo; s < s_hi; ++s) {
        const float2 q = tile[(size_t)s * slice_stride + pix_off];
        acc.x += q.x;
        acc.y += q.y;
    }
    return acc;
}

__device__ __forceinline__ float gen_block_sum(float val, float* red, int tid, int nt) {
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) val += __shfl_down(val, off, 64);
    __syncthreads();
    if ((tid & 63) == 0) red[tid >> 6] = val;
    __syncthreads();
    float s = 0.f;
    if (tid == 0) for (int w = 0; w < (nt >> 6); ++w) s += red[w];
    return s;          // valid on thread 0
}

}  // namespace adm
