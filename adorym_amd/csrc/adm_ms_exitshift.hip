// Per-angle projection alignment on streamed plans (adm_plan_set_exit_shift): the field behind the last slice is Fourier-shifted
// by a sub-pixel offset s = (s_y, s_x) of its own per position before the free-space step to the detector
// (adorym/propagate.py:260-261, util.py:380-397: realign_image_fourier),
//   Psi_det = IFFT2( Phi * H_free * FFT2(Psi_S) ),   Phi[ky,kx] = exp(-2 PI i (fx s_x + fy s_y)),   f = fftfreq(n, 1),
// with H_free = 1 for an exit-wave detector.  The shift and the propagation are ONE transform pair: the two kernels below stand
// in the place of st_col_conv_kernel<false / true> at the detector step of ms_streamed_launch (adm_ms_streamed.hip), same launch
// geometry -- one workgroup per (position, mode, column group).
//
// Adjoint, with G the field the detector kernel hands back, a = FFT2(G) (unnormalised) and kept = Phi H_free FFT2(Psi_S) / (Py*Px)
// of the forward sweep:
//   back into the slice loop:   IFFT2( conj(Phi H_free) a )
//   dL/ds_y = 2 PI sum_k fy_k Im( conj(a_k) kept_k ),   dL/ds_x the same with fx_k
// Products in fp32, sums in fp64 (per thread, wave shuffle, the waves in order), ONE pair of partials per workgroup;
// es_reduce_kernel gathers the partials of every offset entry in a fixed order and adds them to the caller's buffer.  No atomics.
//
// st_cw, st_col_threads and the column helpers are restated from adm_ms_streamed.hip (tests/test_prj_offset_coverage.py holds the
// copies to the originals).
#include <hip/hip_runtime.h>
#include "adm_host.h"
#include "adm_fft.h"
#include "adm_ms_math.h"
#include "adm_ms_gen.h"

namespace adm {

constexpr int ES_COL_NT = 512;                 // most threads of a column workgroup (GEN_E elements each)
__host__ __device__ __forceinline__ int es_cw(int py) { return py <= ES_COL_NT * GEN_E / 8 ? 8 : 4; }

template <bool INV> __device__ __forceinline__ void es_col_fft(const GenCtx& g, const MsParams& p, cf (&v)[GEN_E]) {
    int Ns = 1;
    for (int s = 0; s < p.gen_nry; ++s) { gen_pass<true, INV>(g, p.gen_ry[s], Ns, v); Ns *= p.gen_ry[s]; }
}

// LDS of a column workgroup: the [Py][cw] group, then W_Py^j
__device__ __forceinline__ void es_col_ctx(GenCtx& g, cf* lds, const MsParams& p, int c0, int cw) {
    g.Py = p.gen_py; g.Px = min(cw, p.gen_px - c0); g.n = g.Py * g.Px;
    g.tid = threadIdx.x; g.nt = blockDim.x;
    g.ne = (g.n + g.nt - 1) / g.nt;
    g.fld = lds;
    cf* twy = lds + (size_t)g.Py * cw;
    for (int i = g.tid; i < g.Py; i += g.nt) twy[i] = p.gen_twid_y[i];
    g.twx = nullptr; g.twy = twy;
}
__device__ __forceinline__ void es_col_load(const GenCtx& g, const float2* f, int Px, int c0) {
    for (int i = g.tid; i < g.n; i += g.nt) {
        const int y = i / g.Px;
        g.fld[i] = f[(size_t)y * Px + c0 + (i - y * g.Px)];
    }
}
__device__ __forceinline__ void es_col_store(const GenCtx& g, float2* f, int Px, int c0) {
    for (int i = g.tid; i < g.n; i += g.nt) {
        const int y = i / g.Px;
        f[(size_t)y * Px + c0 + (i - y * g.Px)] = g.fld[i];
    }
}

// fftfreq(n)[i] * n
__device__ __forceinline__ int es_freq_index(int i, int n) { return i <= (n - 1) / 2 ? i : i - n; }
// fftfreq(n, 1)[i], one rounding (fftfreq_f of adm_multislice.hip)
__device__ __forceinline__ float es_freq(int i, int n) { return (float)((double)es_freq_index(i, n) / (double)n); }

// Phi at (fy, fx) for the offset s = (s_y, s_x): the argument in fp32, contraction off, as shift_phases (adm_multislice.hip)
__device__ __forceinline__ cf es_phase(float fy, float fx, float2 s) {
#pragma clang fp contract(off)
    const float m2pi = (float)(-2.0 * 3.14159265359);
    const float arg = m2pi * (fx * s.y + fy * s.x);
    float sn, cs;
    sincos_fast(arg, sn, cs);
    return make_float2(cs, sn);
}

// field <- column IFFT( Phi_b * H * column FFT(field) ) for one (position, mode, column group); hs = H / (Py*Px), or nullptr:
// H = 1.  Forward: keeps the multiplied spectrum when q.keep.  Adjoint (CONJ): conj(Phi_b H), and this workgroup's share of
// dL/ds when q.part.
template <bool CONJ> __global__ __launch_bounds__(ES_COL_NT) void es_col_conv_kernel(MsParams p, float2* __restrict__ fld,
                                                                                      const float2* __restrict__ hs, StExitShift q) {
    extern __shared__ cf es_lds[];
    __shared__ double redd[2 * (ES_COL_NT / 64)];
    const int Py = p.gen_py, Px = p.gen_px, cw = es_cw(Py), ncg = (Px + cw - 1) / cw;
    const int bm = blockIdx.x / ncg, c0 = (blockIdx.x - bm * ncg) * cw;
    const int b = bm / p.n_modes;
    GenCtx g;
    es_col_ctx(g, es_lds, p, c0, cw);
    const size_t row = (size_t)Py * Px;
    float2* f = fld + (size_t)bm * row;
    float2* keep = q.keep ? q.keep + (size_t)bm * row : nullptr;
    const float2 s = q.shifts[q.index ? q.index[b] : b];
    const float inv = (float)(1.0 / ((double)Py * (double)Px));
    es_col_load(g, f, Px, c0);
    __syncthreads();
    cf v[GEN_E];
    es_col_fft<false>(g, p, v);
    const bool sums = CONJ && q.part != nullptr;
    double accy = 0.0, accx = 0.0;
#pragma unroll
    for (int j = 0; j < GEN_E; ++j) {
        const int i = g.tid + j * g.nt;
        if (j < g.ne && i < g.n) {
            const int y = i / g.Px, x = c0 + (i - y * g.Px);
            const size_t k = (size_t)y * Px + x;
            const float fy = es_freq(y, Py), fx = es_freq(x, Px);
            const cf ph = es_phase(fy, fx, s);
            const cf a = g.fld[i];
            if (CONJ) {
                if (sums) {
                    const cf w = keep[k];
                    const float im = a.x * w.y - a.y * w.x;
                    accy += (double)(fy * im);
                    accx += (double)(fx * im);
                }
                g.fld[i] = cmulc(hs ? cmulc(a, hs[k]) : cscale(a, inv), ph);
            } else {
                const cf w = cmul(hs ? cmul(a, hs[k]) : cscale(a, inv), ph);
                if (keep) keep[k] = w;
                g.fld[i] = w;
            }
        }
    }
    if (sums) {
#pragma unroll
        for (int off = 32; off > 0; off >>= 1) {
            accy += __shfl_down(accy, off, 64);
            accx += __shfl_down(accx, off, 64);
        }
        if ((g.tid & 63) == 0) { redd[2 * (g.tid >> 6)] = accy; redd[2 * (g.tid >> 6) + 1] = accx; }
    }
    __syncthreads();
    if (sums && g.tid == 0) {
        double sy = 0.0, sx = 0.0;
        for (int w = 0; w < (g.nt >> 6); ++w) { sy += redd[2 * w]; sx += redd[2 * w + 1]; }
        q.part[2 * (size_t)blockIdx.x] = sy;
        q.part[2 * (size_t)blockIdx.x + 1] = sx;
    }
    es_col_fft<true>(g, p, v);
    es_col_store(g, f, Px, c0);
}

// grad_shifts[e] += 2 PI * (the partials of every position that uses entry e: ascending position, then mode, then column group).
// One workgroup per position; the first position of an entry gathers for it, the others leave.  per = n_modes * column groups.
__global__ __launch_bounds__(256) void es_reduce_kernel(const double* __restrict__ part, int batch, int per, const int* __restrict__ index,
                                                        float* grad_shifts) {
    __shared__ double red[2 * 256];
    __shared__ int later;
    const int b = blockIdx.x, t = threadIdx.x;
    const int e = index ? index[b] : b;
    if (t == 0) later = 0;
    __syncthreads();
    if (index) {
        int seen = 0;
        for (int c = t; c < b; c += 256) seen |= (index[c] == e);
        if (seen) later = 1;           // (every writer stores the same value)
    }
    __syncthreads();
    if (later) return;
    double ay = 0.0, ax = 0.0;
    for (int c = b; c < batch; ++c) {
        if (c != b && (!index || index[c] != e)) continue;
        const double* pc = part + 2 * (size_t)c * per;
        for (int i = t; i < per; i += 256) { ay += pc[2 * i]; ax += pc[2 * i + 1]; }
    }
    red[2 * t] = ay; red[2 * t + 1] = ax;
    __syncthreads();
    for (int h = 128; h > 0; h >>= 1) {
        if (t < h) { red[2 * t] += red[2 * (t + h)]; red[2 * t + 1] += red[2 * (t + h) + 1]; }
        __syncthreads();
    }
    if (t < 2) {
        const double two_pi = 2.0 * 3.14159265359;
        grad_shifts[2 * (size_t)e + t] += (float)(two_pi * red[t]);
    }
}

static int es_col_threads(int py) {
    const int n = py * es_cw(py);
    int nt = ((n + GEN_E - 1) / GEN_E + 63) / 64 * 64;
    if (nt < 256) nt = 256;
    return nt;
}

hipError_t ms_exitshift_col_launch(const MsParams& p, int batch, float2* fld, const float2* hs, bool conj, const StExitShiftLaunch& xs,
                                   hipStream_t st) {
    const int Py = p.gen_py, Px = p.gen_px, cw = es_cw(Py), ncg = (Px + cw - 1) / cw;
    const size_t clds = ((size_t)Py * cw + Py) * sizeof(float2);
    static bool attr_set = false;
    if (!attr_set) {
        const int lim = 160 * 1024 - 256;
        hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void*>(es_col_conv_kernel<false>), hipFuncAttributeMaxDynamicSharedMemorySize, lim);
        if (e == hipSuccess) e = hipFuncSetAttribute(reinterpret_cast<const void*>(es_col_conv_kernel<true>), hipFuncAttributeMaxDynamicSharedMemorySize, lim);
        if (e != hipSuccess) return e;
        attr_set = true;
    }
    const bool sums = p.want_grad && xs.grad_shifts;
    StExitShift q;
    q.shifts = (const float2*)xs.shifts; q.index = xs.index;
    q.keep = sums ? xs.keep : nullptr;
    q.part = sums ? xs.part : nullptr;
    const dim3 grid((unsigned)(batch * p.n_modes * ncg)), block((unsigned)es_col_threads(Py));
    if (conj) hipLaunchKernelGGL(es_col_conv_kernel<true>, grid, block, clds, st, p, fld, hs, q);
    else hipLaunchKernelGGL(es_col_conv_kernel<false>, grid, block, clds, st, p, fld, hs, q);
    return hipGetLastError();
}

hipError_t ms_exitshift_reduce_launch(const MsParams& p, int batch, const StExitShiftLaunch& xs, hipStream_t st) {
    const int cw = es_cw(p.gen_py), ncg = (p.gen_px + cw - 1) / cw;
    hipLaunchKernelGGL(es_reduce_kernel, dim3((unsigned)batch), dim3(256), 0, st, xs.part, batch, p.n_modes * ncg, xs.index, xs.grad_shifts);
    return hipGetLastError();
}

}  // namespace adm
