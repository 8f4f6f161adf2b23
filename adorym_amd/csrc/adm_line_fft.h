// The line machinery of the holography kernels, stated once: Stockham passes in LDS, line_sync, LineGeo, the block-cooperative
// transposed store, the LDS twiddle copy, line_fft, the sums over a line's threads, mul_rounded, and what a launcher needs of them
// (blocks_for, ADM_LINE_SIZES).  adm_holo.hip, adm_holo_ctf.hip and adm_ctf_invert.hip include it and pull namespace linefft into
// their own; tests/test_ctfinv_coverage.py holds the layout (those three users, one definition of each piece), and the coverage
// tests of the three files read the launch arithmetic here.  The host setup that goes with it (twiddle tables, the frequency mesh,
// the accepted sides) is adm_line_host.h.  Kernel header, gfx950; blocks of 256 threads.
#pragma once
#include "adm_fft.h"

// the line lengths every line kernel is instantiated for: the powers of two that line_side_ok (adm_line_host.h) accepts
#define ADM_LINE_SIZES(X) X(16) X(32) X(64) X(128) X(256) X(512) X(1024) X(2048)

namespace adm {
namespace linefft {

// ---------------------------------------------------------------------------------------------------------------
// batched row FFT with transposed store
// ---------------------------------------------------------------------------------------------------------------
template <int N, int NS, int R, bool INV, int TPR>
__device__ __forceinline__ void stockham_pass(const cf* __restrict__ src, cf* __restrict__ dst, const float2* __restrict__ tw, int t) {
    constexpr int NB = N / R;                 // butterflies per row
    constexpr int TWS = N / (NS * R);         // twiddle table stride
    for (int j = t; j < NB; j += TPR) {
        const int k = j % NS;
        cf v[R];
#pragma unroll
        for (int q = 0; q < R; ++q) {
            v[q] = src[j + q * NB];
            if (NS > 1 && q > 0) {
                const cf w = tw[q * k * TWS];
                v[q] = INV ? cmulc(v[q], w) : cmul(v[q], w);
            }
        }
        Dft<R, INV>::run(v);
        const int j0 = (j / NS) * NS * R + k;
#pragma unroll
        for (int q = 0; q < R; ++q) dst[j0 + q * NS] = v[q];
    }
}

// The TPR threads of a line are one wave or part of one when TPR <= 64 (lines of up to 512 points): LDS operations of a wave
// execute in order, so ordering the compiler is all a line-local exchange needs -- no workgroup barrier between the passes of a
// transform, the four lines of a block run at their own pace.  Longer lines span two or four waves and keep the barrier.
template <int TPR> __device__ __forceinline__ void line_sync() {
    if (TPR <= 64) {
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
        __builtin_amdgcn_wave_barrier();
        __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
    } else {
        __syncthreads();
    }
}

template <int N, int NS, bool INV, int TPR> struct Passes {
    static __device__ __forceinline__ int run(cf* a, cf* b, const float2* tw, int t) {
        constexpr int REM = N / NS;
        constexpr int R = REM >= 8 ? 8 : REM;
        stockham_pass<N, NS, R, INV, TPR>(a, b, tw, t);
        line_sync<TPR>();
        return 1 + Passes<N, NS * R, INV, TPR>::run(b, a, tw, t);
    }
};
template <int N, bool INV, int TPR> struct Passes<N, N, INV, TPR> {
    static __device__ __forceinline__ int run(cf*, cf*, const float2*, int) { return 0; }
};

// Every stage of the kernels is "lines of length N through LDS": a block of 256 threads works on LPB = 256 / (N / 8) lines at once,
// N / 8 threads per line.
template <int N> struct LineGeo {
    static constexpr int TPR = N / 8;             // threads per line
    static constexpr int LPB = 256 / TPR;         // lines per block
    // pitch of a line's LDS buffer: N + 32 / min(LPB, 32) elements, so that the block-wide transposed read of
    // store_lines_transposed (a half wave = min(LPB, 32) lines x 32 / min(LPB, 32) consecutive points) touches 32 different
    // 8-byte bank pairs
    static constexpr int LP = N + (LPB > 1 ? 32 / (LPB < 32 ? LPB : 32) : 0);
};

// blocks of a launch over `lines` lines
template <int N> static int blocks_for(int lines) { return (lines + LineGeo<N>::LPB - 1) / LineGeo<N>::LPB; }

// The x and y stages of a 2-D transform hand their results over transposed.  A line's own threads would store its points 8 bytes
// at a time, pitch * 8 bytes apart: one L2 write transaction per point (1 M of them per K2 / K3 launch of adm_holo.hip at
// 512 x 512 x 4 -- the store-ablated build of round 6 is 15 us of 76 faster).  Instead the block stores its LPB adjacent lines
// together: thread e writes point e / LPB of line e % LPB, so LPB consecutive lanes fill LPB * 8 contiguous bytes (32 B at N = 512:
// a quarter of the transactions).  `base`: LDS address of line 0's result (all lines of a block finish in the same buffer);
// at(r, c): destination of point r of line c.
template <int N, typename At> __device__ __forceinline__ void store_lines_transposed(const cf* base, int n_lines, At at) {
    using LG = LineGeo<N>;
    __syncthreads();                               // every line of the block is complete
    for (int e = threadIdx.x; e < N * LG::LPB; e += 256) {
        const int c = e % LG::LPB, r = e / LG::LPB;
        if (c < n_lines) *at(r, c) = base[c * LG::LP + r];
    }
}
// The passes read 7 twiddles per butterfly: from an LDS copy of the table (N <= 1024; the caller's next barrier orders the copy
// before the first pass), from global memory otherwise (the line buffers of N = 2048 leave no room).
template <int N> struct TwLds {
    static constexpr bool USE = (N <= 1024);
    static constexpr int SIZE = USE ? N : 1;
};
template <int N> __device__ __forceinline__ const float2* stage_twiddles(float2* lds, const float2* __restrict__ tw) {
    if (!TwLds<N>::USE) return tw;
    for (int j = threadIdx.x; j < N; j += 256) lds[j] = tw[j];
    return lds;
}
// transform the line in `a` (filled, block synchronised); returns the buffer that holds the result (block synchronised)
template <int N, bool INV> __device__ __forceinline__ cf* line_fft(cf* a, cf* b, const float2* __restrict__ tw, int t) {
    const int np = Passes<N, 1, INV, LineGeo<N>::TPR>::run(a, b, tw, t);
    return (np & 1) ? b : a;
}

// a * b rounded on its own: with contraction off the product cannot merge with a following addition into one fused multiply-add,
// so that `old + mul_rounded(a, b)` adds the very float an overwriting launch stores (accumulated = seeded + overwritten, bit for bit)
__device__ __forceinline__ float mul_rounded(float a, float b) {
#pragma clang fp contract(off)
    return a * b;
}

// sum of v over the TPR threads of a line group (TPR a power of two <= 256); every thread of the block calls it.  A line of up to
// 64 threads is (part of) one wave: a fixed shuffle tree, no LDS, no workgroup barrier (the lines of a block stay independent);
// longer lines go through red (256 entries of LDS, free again when the call returns).  Either way the order of the additions is
// fixed: bit-reproducible.  T: float, or double where the terms cancel.
template <int TPR, typename T> __device__ __forceinline__ T line_sum(T v, T* red) {
    if (TPR <= 64) {
#pragma unroll
        for (int s = TPR / 2; s > 0; s >>= 1) v += __shfl_xor(v, s, 64);
        return v;
    }
    const int tid = threadIdx.x;
    red[tid] = v;
    __syncthreads();
#pragma unroll
    for (int s = TPR / 2; s > 0; s >>= 1) {
        if ((tid % TPR) < s) red[tid] += red[tid + s];
        __syncthreads();
    }
    const T r = red[tid - tid % TPR];
    __syncthreads();
    return r;
}

// the same for Q quantities at once (one set of barriers); red: [Q][256]
template <int TPR, int Q> __device__ __forceinline__ void line_sums(float (&v)[Q], float (*red)[256]) {
    if (TPR <= 64) {
#pragma unroll
        for (int q = 0; q < Q; ++q) {
#pragma unroll
            for (int s = TPR / 2; s > 0; s >>= 1) v[q] += __shfl_xor(v[q], s, 64);
        }
        return;
    }
    const int tid = threadIdx.x;
#pragma unroll
    for (int q = 0; q < Q; ++q) red[q][tid] = v[q];
    __syncthreads();
#pragma unroll
    for (int s = TPR / 2; s > 0; s >>= 1) {
        if ((tid % TPR) < s) {
#pragma unroll
            for (int q = 0; q < Q; ++q) red[q][tid] += red[q][tid + s];
        }
        __syncthreads();
    }
#pragma unroll
    for (int q = 0; q < Q; ++q) v[q] = red[q][tid - tid % TPR];
    __syncthreads();
}

}  // namespace linefft
}  // namespace adm
