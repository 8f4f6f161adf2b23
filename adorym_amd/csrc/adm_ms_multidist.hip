// Multi-distance detector step on streamed plans (adm_plan_set_detector_fanout): ONE field behind the last slice, Psi_S, is
// Fresnel-propagated to D detector planes (adorym/forward_model.py:971-1019: MultiDistModel.predict after the slice loop),
//   Psi_d = IFFT2( H_d * FFT2(Psi_S) ),   d = 0 .. D-1,
// so that the slice sweep runs once per position whatever D is.  The two kernels below stand in the place of
// st_col_conv_kernel<false / true> at the detector step of ms_streamed_launch (adm_ms_streamed.hip), same launch geometry -- one
// workgroup per (position, mode, column group) of the B*M sweep fields:
//   fan-out  md_fanout_kernel: column FFT of the group once, the spectrum kept in registers (a thread owns the same elements
//            before and after a transform); per d: * H_d / (Py*Px), column IFFT, stored into detector field (b, d, m).  The row
//            IFFT, st_det_kernel and the loss reduction then run over the B*D detector entries (entry b*D + d) as over positions.
//   fan-in   md_fanin_kernel: per d, ascending: column FFT of G_d's group (after the row FFT over the detector fields),
//            acc += conj(H_d / (Py*Px)) * spectrum per element in registers; then one column IFFT, stored into sweep field (b, m):
//            g_S = sum_d IFFT2( conj(H_d) FFT2(G_d) ).  A fixed order, no atomics.
// At D = 1 both do exactly st_col_conv_kernel's arithmetic.
//
// Detector distances as parameters (adm_plan_set_fanout_distances, adm_multislice_fwd_adj_fanout_dist): the reference's
// optimize_free_prop for a 3-D object (adorym/propagate.py:274-277, 556-568: fresnel_propagate_wrapped behind the slice loop,
// H_d = exp(i a d_d) with a = -sigma PI lambda (u^2 + v^2) per nm and d_d in nm).  The distances then live on the device:
//   table    st_fresnel_table_kernel (adm_ms_streamed.hip): hs[d][y][x] = exp(i a_yx d_d) / (Py*Px) from the float32 distances
//            (cm) as they sit in the caller's buffer, and ay[y] + ax[x] = a_yx.
//   fan-out  md_fanout_kernel<true>: the same arithmetic, and the column-transformed spectrum Psihat of every (position, mode)
//            field stored once (fan_keep section of the workspace).
//   fan-in   md_fanin_kernel<true>: the same products, the same ascending-d accumulation -- the object and probe gradients keep
//            their bits: it is the same loop body -- and per d, with Ghat_d the spectrum of G_d after its column transform,
//              dL/dd_d = - sum_k a_k Im( conj(Ghat_d,k) * Psihat_k * H_d,k / (Py*Px) )
//            over the workgroup's elements (products in fp32, sums in fp64): ONE partial per (d, workgroup).
//   reduce   st_dd_reduce_kernel (adm_ms_streamed.hip): the partials of a distance added in a fixed order,
//            grad_dists[d] += 1e7 * sum (per cm).  No atomics.
// The launchers pick the <true> instantiations when, and only when, StFanoutLaunch::grad_dists is set.  The helpers: adm_ms_col.h.
#include <hip/hip_runtime.h>
#include "adm_host.h"
#include "adm_ms_col.h"

namespace adm {

// GRAD: also keeps the spectrum of its group (r.keep)
template <bool GRAD> __global__ __launch_bounds__(ST_COL_NT) void md_fanout_kernel(MsParams p, const float2* __restrict__ fld, StFanout q, StDistGrad r) {
    extern __shared__ cf md_lds[];
    // (st_col_begin written out: behind the helper the scheduler orders the prologue of these two kernels differently, and the
    // instantiation without the gradient is held to the instruction stream it had before the gradient existed)
    const int Py = p.gen_py, Px = p.gen_px, cw = st_cw(Py), ncg = (Px + cw - 1) / cw;
    const int bm = blockIdx.x / ncg, c0 = (blockIdx.x - bm * ncg) * cw;
    const int b = bm / p.n_modes, m = bm - b * p.n_modes;
    GenCtx g;
    st_col_ctx(g, md_lds, p, c0, cw);
    const size_t row = (size_t)Py * Px;
    st_col_load(g, fld + (size_t)bm * row, Px, c0);
    __syncthreads();
    cf v[GEN_E], sp[GEN_E];
    st_col_fft<false>(g, p, v);
    float2* keep = GRAD ? r.keep + (size_t)bm * row : nullptr;
#pragma unroll
    for (int j = 0; j < GEN_E; ++j) {
        const int i = g.tid + j * g.nt;
        if (j < g.ne && i < g.n) {
            sp[j] = g.fld[i];
            if constexpr (GRAD) {
                const int y = i / g.Px;
                keep[(size_t)y * Px + c0 + (i - y * g.Px)] = sp[j];
            }
        }
    }
    for (int d = 0; d < q.n; ++d) {
        const float2* hs = q.hs + (size_t)d * row;
#pragma unroll
        for (int j = 0; j < GEN_E; ++j) {
            const int i = g.tid + j * g.nt;
            if (j < g.ne && i < g.n) {
                const int y = i / g.Px;
                g.fld[i] = cmul(sp[j], hs[(size_t)y * Px + c0 + (i - y * g.Px)]);
            }
        }
        __syncthreads();
        st_col_fft<true>(g, p, v);
        // (the store reads, and the next distance overwrites, this thread's own elements only)
        st_col_store(g, q.dfld + (((size_t)b * q.n + d) * p.n_modes + m) * row, Px, c0);
    }
}

// GRAD: also forms this workgroup's share of dL/dd_d, per d, before the conj(H_d) accumulate
template <bool GRAD> __global__ __launch_bounds__(ST_COL_NT) void md_fanin_kernel(MsParams p, float2* __restrict__ fld, StFanout q, StDistGrad r) {
    extern __shared__ cf md_lds[];
    const int Py = p.gen_py, Px = p.gen_px, cw = st_cw(Py), ncg = (Px + cw - 1) / cw;
    const int bm = blockIdx.x / ncg, c0 = (blockIdx.x - bm * ncg) * cw;
    const int b = bm / p.n_modes, m = bm - b * p.n_modes;
    GenCtx g;
    st_col_ctx(g, md_lds, p, c0, cw);
    const size_t row = (size_t)Py * Px;
    const float2* keep = GRAD ? r.keep + (size_t)bm * row : nullptr;
    cf v[GEN_E], acc[GEN_E];
#pragma unroll
    for (int j = 0; j < GEN_E; ++j) acc[j] = make_float2(0.f, 0.f);
    for (int d = 0; d < q.n; ++d) {
        const float2* hs = q.hs + (size_t)d * row;
        st_col_load(g, q.dfld + (((size_t)b * q.n + d) * p.n_modes + m) * row, Px, c0);
        __syncthreads();
        st_col_fft<false>(g, p, v);
        double dsum[1] = {0.0};
        if constexpr (GRAD) {
            // the gradient's pass over this thread's elements first, a loop of its own (rolled: beside the 16 accumulators of the
            // unrolled pass below its operands no longer fit the registers), then the accumulate as it stands without the gradient
#pragma unroll 1
            for (int i = g.tid; i < g.n; i += g.nt) {
                const int y = i / g.Px, x = c0 + (i - y * g.Px);
                const size_t k = (size_t)y * Px + x;
                const cf a = g.fld[i];
                const cf w = cmul(keep[k], hs[k]);
                dsum[0] += (double)((r.ay[y] + r.ax[x]) * (a.x * w.y - a.y * w.x));
            }
        }
#pragma unroll
        for (int j = 0; j < GEN_E; ++j) {
            const int i = g.tid + j * g.nt;
            if (j < g.ne && i < g.n) {
                const int y = i / g.Px;
                acc[j] = cadd(acc[j], cmulc(g.fld[i], hs[(size_t)y * Px + c0 + (i - y * g.Px)]));
            }
        }
        if constexpr (GRAD) {
            __shared__ double redd[ST_COL_NT / 64];      // (inside the discarded branch: no LDS without the gradient)
            // (the barrier inside also stands between this distance's reads of redd on thread 0 and the next distance's writes: those
            // come behind the barrier that follows the next load)
            st_block_sum_f64(dsum, redd, g.tid, g.nt, true);
            if (g.tid == 0) r.part[(size_t)d * gridDim.x + blockIdx.x] = -dsum[0];
        }
    }
#pragma unroll
    for (int j = 0; j < GEN_E; ++j) {
        const int i = g.tid + j * g.nt;
        if (j < g.ne && i < g.n) g.fld[i] = acc[j];
    }
    __syncthreads();
    st_col_fft<true>(g, p, v);
    st_col_store(g, fld + (size_t)bm * row, Px, c0);
}

static void md_args(const StFanoutLaunch& fo, StFanout& q, StDistGrad& r) {
    q.hs = fo.hs; q.dfld = fo.fld; q.n = fo.n;
    r.keep = fo.keep; r.part = fo.part; r.ay = fo.ay; r.ax = fo.ax;
}

hipError_t ms_multidist_fanout_launch(const MsParams& p, int batch, const float2* fld, const StFanoutLaunch& fo, hipStream_t st) {
    const StColGeom cg = st_col_geom(p.gen_py, p.gen_px);
    static bool raised = false;
    hipError_t e = st_col_raise_lds_once(raised, md_fanout_kernel<false>, md_fanout_kernel<true>);
    if (e != hipSuccess) return e;
    StFanout q;
    StDistGrad r;
    md_args(fo, q, r);
    return st_col_launch(fo.grad_dists ? md_fanout_kernel<true> : md_fanout_kernel<false>, cg, batch * p.n_modes, st, p, fld, q, r);
}

hipError_t ms_multidist_fanin_launch(const MsParams& p, int batch, float2* fld, const StFanoutLaunch& fo, hipStream_t st) {
    const StColGeom cg = st_col_geom(p.gen_py, p.gen_px);
    static bool raised = false;
    hipError_t e = st_col_raise_lds_once(raised, md_fanin_kernel<false>, md_fanin_kernel<true>);
    if (e != hipSuccess) return e;
    StFanout q;
    StDistGrad r;
    md_args(fo, q, r);
    return st_col_launch(fo.grad_dists ? md_fanin_kernel<true> : md_fanin_kernel<false>, cg, batch * p.n_modes, st, p, fld, q, r);
}

}  // namespace adm
