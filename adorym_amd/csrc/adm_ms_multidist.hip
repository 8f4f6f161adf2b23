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
// At D = 1 both do exactly st_col_conv_kernel's arithmetic.  (dL/dd_d = -sum_k a_k Im(conj(Ghat_d,k) kept_d,k): the twins of these
// kernels in adm_ms_distgrad.hip, to which the two launchers hand over when the gradient is requested.)  The helpers: adm_ms_col.h.
#include <hip/hip_runtime.h>
#include "adm_host.h"
#include "adm_ms_col.h"

namespace adm {

__global__ __launch_bounds__(ST_COL_NT) void md_fanout_kernel(MsParams p, const float2* __restrict__ fld, StFanout q) {
    extern __shared__ cf md_lds[];
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
#pragma unroll
    for (int j = 0; j < GEN_E; ++j) {
        const int i = g.tid + j * g.nt;
        if (j < g.ne && i < g.n) sp[j] = g.fld[i];
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

__global__ __launch_bounds__(ST_COL_NT) void md_fanin_kernel(MsParams p, float2* __restrict__ fld, StFanout q) {
    extern __shared__ cf md_lds[];
    const int Py = p.gen_py, Px = p.gen_px, cw = st_cw(Py), ncg = (Px + cw - 1) / cw;
    const int bm = blockIdx.x / ncg, c0 = (blockIdx.x - bm * ncg) * cw;
    const int b = bm / p.n_modes, m = bm - b * p.n_modes;
    GenCtx g;
    st_col_ctx(g, md_lds, p, c0, cw);
    const size_t row = (size_t)Py * Px;
    cf v[GEN_E], acc[GEN_E];
#pragma unroll
    for (int j = 0; j < GEN_E; ++j) acc[j] = make_float2(0.f, 0.f);
    for (int d = 0; d < q.n; ++d) {
        const float2* hs = q.hs + (size_t)d * row;
        st_col_load(g, q.dfld + (((size_t)b * q.n + d) * p.n_modes + m) * row, Px, c0);
        __syncthreads();
        st_col_fft<false>(g, p, v);
#pragma unroll
        for (int j = 0; j < GEN_E; ++j) {
            const int i = g.tid + j * g.nt;
            if (j < g.ne && i < g.n) {
                const int y = i / g.Px;
                acc[j] = cadd(acc[j], cmulc(g.fld[i], hs[(size_t)y * Px + c0 + (i - y * g.Px)]));
            }
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

static hipError_t md_raise_lds() {
    static bool attr_set = false;
    if (attr_set) return hipSuccess;
    hipError_t e = st_col_raise_lds(md_fanout_kernel);
    if (e == hipSuccess) e = st_col_raise_lds(md_fanin_kernel);
    attr_set = e == hipSuccess;
    return e;
}

hipError_t ms_multidist_fanout_launch(const MsParams& p, int batch, const float2* fld, const StFanoutLaunch& fo, hipStream_t st) {
    if (fo.grad_dists) return ms_distgrad_fanout_launch(p, batch, fld, fo, st);
    const StColGeom cg = st_col_geom(p.gen_py, p.gen_px);
    hipError_t e = md_raise_lds();
    if (e != hipSuccess) return e;
    StFanout q;
    q.hs = fo.hs; q.dfld = fo.fld; q.n = fo.n;
    hipLaunchKernelGGL(md_fanout_kernel, dim3((unsigned)(batch * p.n_modes * cg.ncg)), dim3((unsigned)cg.threads), cg.lds, st, p, fld, q);
    return hipGetLastError();
}

hipError_t ms_multidist_fanin_launch(const MsParams& p, int batch, float2* fld, const StFanoutLaunch& fo, hipStream_t st) {
    if (fo.grad_dists) return ms_distgrad_fanin_launch(p, batch, fld, fo, st);
    const StColGeom cg = st_col_geom(p.gen_py, p.gen_px);
    hipError_t e = md_raise_lds();
    if (e != hipSuccess) return e;
    StFanout q;
    q.hs = fo.hs; q.dfld = fo.fld; q.n = fo.n;
    hipLaunchKernelGGL(md_fanin_kernel, dim3((unsigned)(batch * p.n_modes * cg.ncg)), dim3((unsigned)cg.threads), cg.lds, st, p, fld, q);
    return hipGetLastError();
}

}  // namespace adm
