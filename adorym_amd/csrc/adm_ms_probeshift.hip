// Sub-pixel probe positions on streamed plans (adm_plan_set_probe_shift): position b illuminates with the probe modes
// Fourier-shifted by an offset s = (s_y, s_x) of its own (adorym/util.py:380-397: realign_image_fourier),
//   probe_b,m = IFFT2( Phi_b * FFT2(probe_m) ),   Phi_b[ky,kx] = exp(-2 PI i (fx s_x + fy s_y)),   f = fftfreq(n, 1),
// the model of adm_probe_shift (adm_multislice.hip); the phase argument is formed in fp64 here (st_shift_phase, adm_ms_col.h).  The LDS kernels
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

// phat <- column FFT(phat) for one (mode, column group): the second half of Phat_m = FFT2(probe_m)
__global__ __launch_bounds__(ST_COL_NT) void ps_colfft_kernel(MsParams p, float2* __restrict__ phat) {
    extern __shared__ cf ps_lds[];
    const int Px = p.gen_px;
    GenCtx g;
    const auto [m, c0] = st_col_begin(g, ps_lds, p);      // (the launch counts modes)
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
    const int Py = p.gen_py, Px = p.gen_px;
    GenCtx g;
    const auto [bm, c0] = st_col_begin(g, ps_lds, p);
    const int b = bm / p.n_modes, m = bm - b * p.n_modes;
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
            const cf ph = st_shift_phase(y, Py, x, Px, s);
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

// phat <- column FFT(phat): [M][Py][Px], the row FFT of the probe modes already in it
hipError_t ms_probeshift_spectrum_launch(const MsParams& p, float2* phat, hipStream_t st) {
    const StColGeom cg = st_col_geom(p.gen_py, p.gen_px);
    static bool raised = false;
    hipError_t e = st_col_raise_lds_once(raised, ps_colfft_kernel);
    if (e != hipSuccess) return e;
    return st_col_launch(ps_colfft_kernel, cg, p.n_modes, st, p, phat);
}

hipError_t ms_probeshift_col_launch(const MsParams& p, int batch, float2* fld, bool conj, const StProbeShift& q, hipStream_t st) {
    const StColGeom cg = st_col_geom(p.gen_py, p.gen_px);
    static bool raised = false;
    hipError_t e = st_col_raise_lds_once(raised, ps_col_kernel<false>, ps_col_kernel<true>);
    if (e != hipSuccess) return e;
    return st_col_launch(conj ? ps_col_kernel<true> : ps_col_kernel<false>, cg, batch * p.n_modes, st, p, fld, q);
}

}  // namespace adm
