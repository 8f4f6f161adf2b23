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
//              st_shift_reduce_kernel (adm_ms_streamed.hip): the partials of every entry added into grad_shifts
// Adjoint, with G the field the sweep hands back and a = FFT2(G):
//   dL/dprobe_m += IFFT2( conj(Phi_b) a )
//   dL/ds_y = 2 PI sum_k fy_k Im( conj(a_k) Phi_b,k Phat_m,k / (Py*Px) ),   dL/ds_x the same with fx_k
// The per-position spectrum is not kept: the adjoint recomputes Phi_b Phat_m / (Py*Px) with the forward launch's expression.
// Products in fp32, sums in fp64 (per thread, wave shuffle, the waves in order), ONE pair of partials per workgroup;
// st_shift_reduce_kernel gathers the partials of every entry in a fixed order and adds them to the caller's buffer.  No atomics.
// The column-workgroup helpers and the launch geometry: adm_ms_col.h.
#include <hip/hip_runtime.h>
#include "adm_host.h"
#include "adm_ms_col.h"

namespace adm {

// Phi at spectral element (y, x) for the offset s = (s_y, s_x).  The argument -2 PI (fx s_x + fy s_y) reaches 16 rad at shifts of
// 2.5 px, where fp32 resolves 1e-6: formed in fp32 (as shift_phases of adm_multislice.hip forms it) that rounding alone puts
// dL/ds of an exit-wave detector 3.4e-4 from the fp64 model, because the terms of that sum cancel to a thousandth of their size.
// So: the argument in fp64, reduced to one turn, then sin / cos in fp32 (the scheme of st_sparse_table_kernel); what is left,
// 8e-5 in that case, is the fp32 rounding of the shifts themselves.
__device__ __forceinline__ cf ps_phase(int y, int py, int x, int px, float2 s) {
    const double fy = (double)st_freq_index(y, py) / (double)py, fx = (double)st_freq_index(x, px) / (double)px;
    double arg = -2.0 * 3.14159265359 * (fx * (double)s.y + fy * (double)s.x);
    const double two_pi = 6.283185307179586476925287;
    arg -= two_pi * rint(arg / two_pi);
    float sn, cs;
    sincos_fast((float)arg, sn, cs);
    return make_float2(cs, sn);
}

// phat <- column FFT(phat) for one (mode, column group): the second half of Phat_m = FFT2(probe_m)
__global__ __launch_bounds__(ST_COL_NT) void ps_colfft_kernel(MsParams p, float2* __restrict__ phat) {
    extern __shared__ cf ps_lds[];
    const int Px = p.gen_px, cw = st_cw(p.gen_py), ncg = (Px + cw - 1) / cw;
    const int m = blockIdx.x / ncg, c0 = (blockIdx.x - m * ncg) * cw;
    GenCtx g;
    st_col_ctx(g, ps_lds, p, c0, cw);
    float2* f = phat + (size_t)m * p.gen_py * Px;
    st_col_load(g, f, Px, c0);
    __syncthreads();
    cf v[GEN_E];
    st_col_fft<false>(g, p, v);
    st_col_store(g, f, Px, c0);
}

// One (position, mode, column group).  Forward: field <- column IFFT( Phi_b Phat_m / (Py*Px) ).  Adjoint (CONJ):
// field <- column IFFT( conj(Phi_b) column FFT(field) / (Py*Px) ), and this workgroup's share of dL/ds when q.part.
// (4 waves per SIMD asked for: without the hint the adjoint instantiation takes 129 VGPRs and one wave less)
template <bool CONJ> __global__ __launch_bounds__(ST_COL_NT, 4) void ps_col_kernel(MsParams p, float2* __restrict__ fld, StProbeShift q) {
    extern __shared__ cf ps_lds[];
    __shared__ double redd[2 * (ST_COL_NT / 64)];
    const int Py = p.gen_py, Px = p.gen_px, cw = st_cw(Py), ncg = (Px + cw - 1) / cw;
    const int bm = blockIdx.x / ncg, c0 = (blockIdx.x - bm * ncg) * cw;
    const int b = bm / p.n_modes, m = bm - b * p.n_modes;
    GenCtx g;
    st_col_ctx(g, ps_lds, p, c0, cw);
    const size_t row = (size_t)Py * Px;
    float2* f = fld + (size_t)bm * row;
    const float2* ph_m = q.phat + (size_t)m * row;
    const float2 s = q.shifts[q.index ? q.index[b] : b];
    const float inv = (float)(1.0 / ((double)Py * (double)Px));
    st_col_load(g, CONJ ? f : ph_m, Px, c0);
    __syncthreads();
    cf v[GEN_E];
    if (CONJ) st_col_fft<false>(g, p, v);
    const bool sums = CONJ && q.part != nullptr;
    double acc[2] = {0.0, 0.0};     // dL/ds_y, dL/ds_x
#pragma unroll
    for (int j = 0; j < GEN_E; ++j) {
        const int i = g.tid + j * g.nt;
        if (j < g.ne && i < g.n) {
            const int y = i / g.Px, x = c0 + (i - y * g.Px);
            const float fy = st_freq(y, Py), fx = st_freq(x, Px);
            const cf ph = ps_phase(y, Py, x, Px, s);
            const cf a = g.fld[i];
            if (CONJ) {
                if (sums) {
                    const cf w = cscale(cmul(ph_m[(size_t)y * Px + x], ph), inv);      // the forward launch's spectrum, recomputed
                    const float im = a.x * w.y - a.y * w.x;
                    acc[0] += (double)(fy * im);
                    acc[1] += (double)(fx * im);
                }
                g.fld[i] = cscale(cmulc(a, ph), inv);
            } else {
                g.fld[i] = cscale(cmul(a, ph), inv);
            }
        }
    }
    st_block_sum_f64(acc, redd, g.tid, g.nt, sums);
    if (sums && g.tid == 0) {
        q.part[2 * (size_t)blockIdx.x] = acc[0];
        q.part[2 * (size_t)blockIdx.x + 1] = acc[1];
    }
    st_col_fft<true>(g, p, v);
    st_col_store(g, f, Px, c0);
}

static hipError_t ms_probeshift_attr() {
    static bool attr_set = false;
    if (attr_set) return hipSuccess;
    hipError_t e = st_col_raise_lds(ps_colfft_kernel);
    if (e == hipSuccess) e = st_col_raise_lds(ps_col_kernel<false>);
    if (e == hipSuccess) e = st_col_raise_lds(ps_col_kernel<true>);
    if (e == hipSuccess) attr_set = true;
    return e;
}

// phat <- column FFT(phat): [M][Py][Px], the row FFT of the probe modes already in it
hipError_t ms_probeshift_spectrum_launch(const MsParams& p, float2* phat, hipStream_t st) {
    const StColGeom cg = st_col_geom(p.gen_py, p.gen_px);
    hipError_t e = ms_probeshift_attr();
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(ps_colfft_kernel, dim3((unsigned)(p.n_modes * cg.ncg)), dim3((unsigned)cg.threads), cg.lds, st, p, phat);
    return hipGetLastError();
}

hipError_t ms_probeshift_col_launch(const MsParams& p, int batch, float2* fld, bool conj, const StProbeShift& q, hipStream_t st) {
    const StColGeom cg = st_col_geom(p.gen_py, p.gen_px);
    hipError_t e = ms_probeshift_attr();
    if (e != hipSuccess) return e;
    const dim3 grid((unsigned)(batch * p.n_modes * cg.ncg)), block((unsigned)cg.threads);
    if (conj) hipLaunchKernelGGL(ps_col_kernel<true>, grid, block, cg.lds, st, p, fld, q);
    else hipLaunchKernelGGL(ps_col_kernel<false>, grid, block, cg.lds, st, p, fld, q);
    return hipGetLastError();
}

}  // namespace adm
