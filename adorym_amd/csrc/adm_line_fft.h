// The line machinery of the holography kernels as a header: Stockham passes in LDS, LineGeo, line_sync, the block-cooperative
// transposed store and the LDS twiddle copy.  adm_ctf_invert.hip is the only file that includes it: adm_holo.hip and
// adm_holo_ctf.hip keep their own copies of the same set, because tests/test_holo_matrix_coverage.py and
// tests/test_ctf_coverage.py pin the text of those two files.  Device-only, gfx950; blocks of 256 threads.
#pragma once
#include "adm_fft.h"

namespace adm {
namespace linefft {

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

// lines of up to 64 threads are (part of) one wave: ordering the compiler is all a line-local exchange needs
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

template <int N> struct LineGeo {
    static constexpr int TPR = N / 8;             // threads per line
    static constexpr int LPB = 256 / TPR;         // lines per block
    static constexpr int LP = N + (LPB > 1 ? 32 / (LPB < 32 ? LPB : 32) : 0);      // LDS pitch of a line (bank spread of the transposed read)
};

// the block stores its LPB adjacent lines together: thread e writes point e / LPB of line e % LPB
template <int N, typename At> __device__ __forceinline__ void store_lines_transposed(const cf* base, int n_lines, At at) {
    using LG = LineGeo<N>;
    __syncthreads();                               // every line of the block is complete
    for (int e = threadIdx.x; e < N * LG::LPB; e += 256) {
        const int c = e % LG::LPB, r = e / LG::LPB;
        if (c < n_lines) *at(r, c) = base[c * LG::LP + r];
    }
}
template <int N> struct TwLds {
    static constexpr bool USE = (N <= 1024);
    static constexpr int SIZE = USE ? N : 1;
};
template <int N> __device__ __forceinline__ const float2* stage_twiddles(float2* lds, const float2* __restrict__ tw) {
    if (!TwLds<N>::USE) return tw;
    for (int j = threadIdx.x; j < N; j += 256) lds[j] = tw[j];
    return lds;
}
// transform the line in `a` (filled, block synchronised); returns the buffer that holds the result
template <int N, bool INV> __device__ __forceinline__ cf* line_fft(cf* a, cf* b, const float2* __restrict__ tw, int t) {
    const int np = Passes<N, 1, INV, LineGeo<N>::TPR>::run(a, b, tw, t);
    return (np & 1) ? b : a;
}

}  // namespace linefft
}  // namespace adm
