// Sub-pixel probe positions on streamed plans (adm_plan_set_probe_shift): position b illuminates with the probe modes
// Fourier-shifted by an offset s = (s_y, s_x) of its own (adorym/util.py:380-397: realign_image_fourier),
//   probe_b,m = IFFT2( Phi_b * FFT2(probe_m) ),   Phi_b[ky,kx] = exp(-2 PI i (fx s_x + fy s_y)),   f = fftfreq(n, 1),
// the model of adm_probe_shift (adm_multislice.hip); the phase argument is formed in fp64 here (ps_phase).  The LDS kernels
// materialise one probe set per position; here the fields live in global memory, so the shift is part of the sweep of ms_streamed_launch
// (adm_ms_streamed.hip), which calls the launchers at the end of this file.  Launches of one minibatch, beside the sweep's own:
//   in front   st_row_kernel (batch = 1, from the probe, row FFT) -> phat;  ps_colfft_kernel: column FFT of phat
//              (Phat_m = FFT2(probe_m), unnormalised, ONCE per launch, shared by all positions)
//              ps_col_kernel<false> per (position, mode, column group): Phat_m Phi_b / (Py*Px), column IFFT -> the field buffer;
//              the sweep's first row launch then starts with the row IFFT and reads the field buffer instead of the probe
//   behind     the sweep's last row launch ends with a row FFT and writes the field buffer instead of the slots; then
//              ps_col_kernel<true>: column FFT -> a = FFT2(G), the dL/ds sums, * conj(Phi_b) / (Py*Px), column IFFT
//              st_row_kernel (transforms only, row IFFT) -> the position's probe-gradient slots (probe_grad_reduce sums them)
//              ps_reduce_kernel: the partials of every entry added into grad_shifts
// Adjoint, with G the field the sweep hands back and a = FFT2(G):
//   dL/dprobe_m += IFFT2( conj(Phi_b) a )
//   dL/ds_y = 2 PI sum_k fy_k Im( conj(a_k) Phi_b,k Phat_m,k / (Py*Px) ),   dL/ds_x the same with fx_k
// The per-position spectrum is not kept: the adjoint recomputes Phi_b Phat_m / (Py*Px) with the forward launch's expression.
// Products in fp32, sums in fp64 (per thread, wave shuffle, the waves in order), ONE pair of partials per workgroup;
// ps_reduce_kernel gathers the partials of every entry in a fixed order and adds them to the caller's buffer.  No atomics.
//
// ps_cw, ps_col_threads and the column helpers are restated from adm_ms_streamed.hip (tests/test_probe_shift_coverage.py holds
// the copies to the originals).
#include <hip/hip_runtime.h>
#include "adm_host.h"
#include "adm_fft.h"
#include "adm_ms_math.h"
#include "adm_ms_gen.h"

namespace adm {

constexpr int PS_COL_NT = 512;                 // most threads of a column workgroup (GEN_E elements each)
__host__ __device__ __forceinline__ int ps_cw(int py) { return py <= PS_COL_NT * GEN_E / 8 ? 8 : 4; }

template <bool INV> __device__ __forceinline__ void ps_col_fft(const GenCtx& g, const MsParams& p, cf (&v)[GEN_E]) {
    int Ns = 1;
    for (int s = 0; s < p.gen_nry; ++s) { gen_pass<true, INV>(g, p.gen_ry[s], Ns, v); Ns *= p.gen_ry[s]; }
}

// LDS of a column workgroup: the [Py][cw] group, then W_Py^j
__device__ __forceinline__ void ps_col_ctx(GenCtx& g, cf* lds, const MsParams& p, int c0, int cw) {
    g.Py = p.gen_py; g.Px = min(cw, p.gen_px - c0); g.n = g.Py * g.Px;
    g.tid = threadIdx.x; g.nt = blockDim.x;
    g.ne = (g.n + g.nt - 1) / g.nt;
    g.fld = lds;
    cf* twy = lds + (size_t)g.Py * cw;
    for (int i = g.tid; i < g.Py; i += g.nt) twy[i] = p.gen_twid_y[i];
    g.twx = nullptr; g.twy = twy;
}
__device__ __forceinline__ void ps_col_load(const GenCtx& g, const float2* f, int Px, int c0) {
    for (int i = g.tid; i < g.n; i += g.nt) {
        const int y = i / g.Px;
        g.fld[i] = f[(size_t)y * Px + c0 + (i - y * g.Px)];
    }
}
__device__ __forceinline__ void ps_col_store(const GenCtx& g, float2* f, int Px, int c0) {
    for (int i = g.tid; i < g.n; i += g.nt) {
        const int y = i / g.Px;
        f[(size_t)y * Px + c0 + (i - y * g.Px)] = g.fld[i];
    }
}

// fftfreq(n)[i] * n
__device__ __forceinline__ int ps_freq_index(int i, int n) { return i <= (n - 1) / 2 ? i : i - n; }
// fftfreq(n, 1)[i], one rounding (fftfreq_f of adm_multislice.hip)
__device__ __forceinline__ float ps_freq(int i, int n) { return (float)((double)ps_freq_index(i, n) / (double)n); }

// Phi at spectral element (y, x) for the offset s = (s_y, s_x).  The argument -2 PI (fx s_x + fy s_y) reaches 16 rad at shifts of
// 2.5 px, where fp32 resolves 1e-6: formed in fp32 (as shift_phases of adm_multislice.hip forms it) that rounding alone puts
// dL/ds of an exit-wave detector 3.4e-4 from the fp64 model, because the terms of that sum cancel to a thousandth of their size.
// So: the argument in fp64, reduced to one turn, then sin / cos in fp32 (the scheme of st_sparse_table_kernel); what is left,
// 8e-5 in that case, is the fp32 rounding of the shifts themselves.
__device__ __forceinline__ cf ps_phase(int y, int py, int x, int px, float2 s) {
    const double fy = (double)ps_freq_index(y, py) / (double)py, fx = (double)ps_freq_index(x, px) / (double)px;
    double arg = -2.0 * 3.14159265359 * (fx * (double)s.y + fy * (double)s.x);
    const double two_pi = 6.283185307179586476925287;
    arg -= two_pi * rint(arg / two_pi);
    float sn, cs;
    sincos_fast((float)arg, sn, cs);
    return make_float2(cs, sn);
}

// phat <- column FFT(phat) for one (mode, column group): the second half of Phat_m = FFT2(probe_m)
__global__ __launch_bounds__(PS_COL_NT) void ps_colfft_kernel(MsParams p, float2* __restrict__ phat) {
    extern __shared__ cf ps_lds[];
    const int Px = p.gen_px, cw = ps_cw(p.gen_py), ncg = (Px + cw - 1) / cw;
    const int m = blockIdx.x / ncg, c0 = (blockIdx.x - m * ncg) * cw;
    GenCtx g;
    ps_col_ctx(g, ps_lds, p, c0, cw);
    float2* f = phat + (size_t)m * p.gen_py * Px;
    ps_col_load(g, f, Px, c0);
    __syncthreads();
    cf v[GEN_E];
    ps_col_fft<false>(g, p, v);
    ps_col_store(g, f, Px, c0);
}

// One (position, mode, column group).  Forward: field <- column IFFT( Phi_b Phat_m / (Py*Px) ).  Adjoint (CONJ):
// field <- column IFFT( conj(Phi_b) column FFT(field) / (Py*Px) ), and this workgroup's share of dL/ds when q.part.
// (4 waves per SIMD asked for: without the hint the adjoint instantiation takes 129 VGPRs and one wave less)
template <bool CONJ> __global__ __launch_bounds__(PS_COL_NT, 4) void ps_col_kernel(MsParams p, float2* __restrict__ fld, StProbeShift q) {
    extern __shared__ cf ps_lds[];
    __shared__ double redd[2 * (PS_COL_NT / 64)];
    const int Py = p.gen_py, Px = p.gen_px, cw = ps_cw(Py), ncg = (Px + cw - 1) / cw;
    const int bm = blockIdx.x / ncg, c0 = (blockIdx.x - bm * ncg) * cw;
    const int b = bm / p.n_modes, m = bm - b * p.n_modes;
    GenCtx g;
    ps_col_ctx(g, ps_lds, p, c0, cw);
    const size_t row = (size_t)Py * Px;
    float2* f = fld + (size_t)bm * row;
    const float2* ph_m = q.phat + (size_t)m * row;
    const float2 s = q.shifts[q.index ? q.index[b] : b];
    const float inv = (float)(1.0 / ((double)Py * (double)Px));
    ps_col_load(g, CONJ ? f : ph_m, Px, c0);
    __syncthreads();
    cf v[GEN_E];
    if (CONJ) ps_col_fft<false>(g, p, v);
    const bool sums = CONJ && q.part != nullptr;
    double accy = 0.0, accx = 0.0;
#pragma unroll
    for (int j = 0; j < GEN_E; ++j) {
        const int i = g.tid + j * g.nt;
        if (j < g.ne && i < g.n) {
            const int y = i / g.Px, x = c0 + (i - y * g.Px);
            const float fy = ps_freq(y, Py), fx = ps_freq(x, Px);
            const cf ph = ps_phase(y, Py, x, Px, s);
            const cf a = g.fld[i];
            if (CONJ) {
                if (sums) {
                    const cf w = cscale(cmul(ph_m[(size_t)y * Px + x], ph), inv);      // the forward launch's spectrum, recomputed
                    const float im = a.x * w.y - a.y * w.x;
                    accy += (double)(fy * im);
                    accx += (double)(fx * im);
                }
                g.fld[i] = cscale(cmulc(a, ph), inv);
            } else {
                g.fld[i] = cscale(cmul(a, ph), inv);
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
    ps_col_fft<true>(g, p, v);
    ps_col_store(g, f, Px, c0);
}

// grad_shifts[e] += 2 PI * (the partials of every position that uses entry e: ascending position, then mode, then column group).
// One workgroup per position; the first position of an entry gathers for it, the others leave.  per = n_modes * column groups.
// (es_reduce_kernel of adm_ms_exitshift.hip, restated.)
__global__ __launch_bounds__(256) void ps_reduce_kernel(const double* __restrict__ part, int batch, int per, const int* __restrict__ index,
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

static int ps_col_threads(int py) {
    const int n = py * ps_cw(py);
    int nt = ((n + GEN_E - 1) / GEN_E + 63) / 64 * 64;
    if (nt < 256) nt = 256;
    return nt;
}

static hipError_t ms_probeshift_attr() {
    static bool attr_set = false;
    if (attr_set) return hipSuccess;
    const int lim = 160 * 1024 - 256;
    hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void*>(ps_colfft_kernel), hipFuncAttributeMaxDynamicSharedMemorySize, lim);
    if (e == hipSuccess) e = hipFuncSetAttribute(reinterpret_cast<const void*>(ps_col_kernel<false>), hipFuncAttributeMaxDynamicSharedMemorySize, lim);
    if (e == hipSuccess) e = hipFuncSetAttribute(reinterpret_cast<const void*>(ps_col_kernel<true>), hipFuncAttributeMaxDynamicSharedMemorySize, lim);
    if (e == hipSuccess) attr_set = true;
    return e;
}

// phat <- column FFT(phat): [M][Py][Px], the row FFT of the probe modes already in it
hipError_t ms_probeshift_spectrum_launch(const MsParams& p, float2* phat, hipStream_t st) {
    const int Py = p.gen_py, Px = p.gen_px, cw = ps_cw(Py), ncg = (Px + cw - 1) / cw;
    const size_t clds = ((size_t)Py * cw + Py) * sizeof(float2);
    hipError_t e = ms_probeshift_attr();
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(ps_colfft_kernel, dim3((unsigned)(p.n_modes * ncg)), dim3((unsigned)ps_col_threads(Py)), clds, st, p, phat);
    return hipGetLastError();
}

hipError_t ms_probeshift_col_launch(const MsParams& p, int batch, float2* fld, bool conj, const StProbeShift& q, hipStream_t st) {
    const int Py = p.gen_py, Px = p.gen_px, cw = ps_cw(Py), ncg = (Px + cw - 1) / cw;
    const size_t clds = ((size_t)Py * cw + Py) * sizeof(float2);
    hipError_t e = ms_probeshift_attr();
    if (e != hipSuccess) return e;
    const dim3 grid((unsigned)(batch * p.n_modes * ncg)), block((unsigned)ps_col_threads(Py));
    if (conj) hipLaunchKernelGGL(ps_col_kernel<true>, grid, block, clds, st, p, fld, q);
    else hipLaunchKernelGGL(ps_col_kernel<false>, grid, block, clds, st, p, fld, q);
    return hipGetLastError();
}

hipError_t ms_probeshift_reduce_launch(const MsParams& p, int batch, const StProbeShift& q, float* grad_shifts, hipStream_t st) {
    const int cw = ps_cw(p.gen_py), ncg = (p.gen_px + cw - 1) / cw;
    hipLaunchKernelGGL(ps_reduce_kernel, dim3((unsigned)batch), dim3(256), 0, st, q.part, batch, p.n_modes * ncg, q.index, grad_shifts);
    return hipGetLastError();
}

}  // namespace adm
