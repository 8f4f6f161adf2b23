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
// st_shift_reduce_kernel (adm_ms_streamed.hip) gathers the partials of every offset entry in a fixed order and adds them to the
// caller's buffer.  No atomics.  The column-workgroup helpers and the launch geometry: adm_ms_col.h.
#include <hip/hip_runtime.h>
#include "adm_host.h"
#include "adm_ms_col.h"

namespace adm {

// field <- column IFFT( Phi_b * H * column FFT(field) ) for one (position, mode, column group); hs = H / (Py*Px), or nullptr:
// H = 1.  Forward: keeps the multiplied spectrum when q.keep.  Adjoint (CONJ): conj(Phi_b H), and this workgroup's share of
// dL/ds when q.part.
template <bool CONJ> __global__ __launch_bounds__(ST_COL_NT) void es_col_conv_kernel(MsParams p, float2* __restrict__ fld,
                                                                                      const float2* __restrict__ hs, StExitShift q) {
    extern __shared__ cf es_lds[];
    __shared__ double redd[2 * (ST_COL_NT / 64)];
    // (st_col_begin written out, as in adm_ms_multidist.hip: behind the helper the prologue came out two instructions longer, and the
    // one-position launch with the shift gradient measured 0.03 - 0.09 % slower twice: profiles/col_refactor/timings.txt)
    const int Py = p.gen_py, Px = p.gen_px, cw = st_cw(Py), ncg = (Px + cw - 1) / cw;
    const int bm = blockIdx.x / ncg, c0 = (blockIdx.x - bm * ncg) * cw;
    const int b = bm / p.n_modes;
    GenCtx g;
    st_col_ctx(g, es_lds, p, c0, cw);
    const size_t row = (size_t)Py * Px;
    float2* f = fld + (size_t)bm * row;
    float2* keep = q.keep ? q.keep + (size_t)bm * row : nullptr;
    const float2 s = q.shifts[q.index ? q.index[b] : b];
    const float inv = (float)(1.0 / ((double)Py * (double)Px));
    st_col_load(g, f, Px, c0);
    __syncthreads();
    cf v[GEN_E];
    st_col_fft<false>(g, p, v);
    const bool sums = CONJ && q.part != nullptr;
    double acc[2] = {0.0, 0.0};     // dL/ds_y, dL/ds_x
#pragma unroll
    for (int j = 0; j < GEN_E; ++j) {
        const int i = g.tid + j * g.nt;
        if (j < g.ne && i < g.n) {
            const int y = i / g.Px, x = c0 + (i - y * g.Px);
            const size_t k = (size_t)y * Px + x;
            const float fy = st_freq(y, Py), fx = st_freq(x, Px);
            const cf ph = st_shift_phase(y, Py, x, Px, s);
            const cf a = g.fld[i];
            if (CONJ) {
                if (sums) {
                    const cf w = keep[k];
                    const float im = a.x * w.y - a.y * w.x;
                    acc[0] += (double)(fy * im);
                    acc[1] += (double)(fx * im);
                }
                g.fld[i] = cmulc(hs ? cmulc(a, hs[k]) : cscale(a, inv), ph);
            } else {
                const cf w = cmul(hs ? cmul(a, hs[k]) : cscale(a, inv), ph);
                if (keep) keep[k] = w;
                g.fld[i] = w;
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

hipError_t ms_exitshift_col_launch(const MsParams& p, int batch, float2* fld, const float2* hs, bool conj, const StExitShiftLaunch& xs,
                                   hipStream_t st) {
    const StColGeom cg = st_col_geom(p.gen_py, p.gen_px);
    static bool raised = false;
    hipError_t e = st_col_raise_lds_once(raised, es_col_conv_kernel<false>, es_col_conv_kernel<true>);
    if (e != hipSuccess) return e;
    const bool sums = p.want_grad && xs.grad_shifts;
    StExitShift q;
    q.shifts = (const float2*)xs.shifts; q.index = xs.index;
    q.keep = sums ? xs.keep : nullptr;
    q.part = sums ? xs.part : nullptr;
    return st_col_launch(conj ? es_col_conv_kernel<true> : es_col_conv_kernel<false>, cg, batch * p.n_modes, st, p, fld, hs, q);
}

}  // namespace adm
