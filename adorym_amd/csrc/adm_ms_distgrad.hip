// Detector distances as parameters of the multi-distance detector step (adm_plan_set_fanout_distances,
// adm_multislice_fwd_adj_fanout_dist): the reference's optimize_free_prop for a 3-D object (adorym/propagate.py:274-277, 556-568:
// fresnel_propagate_wrapped behind the slice loop, H_d = exp(i a d_d) with a = -sigma PI lambda (u^2 + v^2) per nm and d_d in nm).
// The fan-out of adm_ms_multidist.hip with the distances living on the device:
//   table    dg_table_kernel: hs[d][y][x] = exp(i a_yx d_d) / (Py*Px) from the float32 distances (cm) as they sit in the caller's
//            buffer, and ay[y] + ax[x] = a_yx -- st_sparse_table_kernel's arithmetic (adm_ms_streamed.hip).
//   fan-out  dg_fanout_kernel: md_fanout_kernel's arithmetic, and the column-transformed spectrum Psihat of every (position, mode)
//            field stored once (fan_keep section of the workspace).
//   fan-in   dg_fanin_kernel: md_fanin_kernel's arithmetic (same products, same ascending-d accumulation: the object and probe
//            gradients keep their bits), and per d, with Ghat_d the spectrum of G_d after its column transform,
//              dL/dd_d = - sum_k a_k Im( conj(Ghat_d,k) * Psihat_k * H_d,k / (Py*Px) )
//            over the workgroup's elements (products in fp32, sums in fp64): ONE partial per (d, workgroup).
//   reduce   dg_reduce_kernel: the partials of a distance added in a fixed order, grad_dists[d] += 1e7 * sum (per cm).  No atomics.
// ms_multidist_fanout_launch / ms_multidist_fanin_launch (adm_ms_multidist.hip) hand a launch over to this file when, and only when,
// StFanoutLaunch::grad_dists is set.  The column-workgroup helpers: adm_ms_col.h.
#include <hip/hip_runtime.h>
#include "adm_host.h"
#include "adm_ms_col.h"

namespace adm {

// hs[d][y][x] = exp(i a_yx d_d) / (Py*Px): the phase in fp64, reduced to one turn, then sin / cos in fp32 and one rounding for the
// division.  ay[y] + ax[x] = a_yx for the gradient kernel (fp32).
__global__ __launch_bounds__(256) void dg_table_kernel(StDistGeom q, const float* __restrict__ dists_cm, float2* __restrict__ hs,
                                                        float* __restrict__ ay, float* __restrict__ ax) {
    const size_t row = (size_t)q.py * q.px, n = (size_t)q.n * row;
    const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
    const double c = -q.sigma * 3.14159265359 * q.lambda_nm;
    if (i < (size_t)q.py) { const double u = (double)st_freq_index((int)i, q.py) / q.py / q.voxel_nm_y; ay[i] = (float)(c * u * u); }
    if (i < (size_t)q.px) { const double v = (double)st_freq_index((int)i, q.px) / q.px / q.voxel_nm_x; ax[i] = (float)(c * v * v); }
    if (i >= n) return;
    const int d = (int)(i / row);
    const int y = (int)((i - (size_t)d * row) / q.px), x = (int)(i - (size_t)d * row - (size_t)y * q.px);
    const double u = (double)st_freq_index(y, q.py) / q.py / q.voxel_nm_y, v = (double)st_freq_index(x, q.px) / q.px / q.voxel_nm_x;
    const double d_nm = (double)dists_cm[d] * 1e7;
    double ph = c * (u * u + v * v) * d_nm;
    const double two_pi = 6.283185307179586476925287;
    ph -= two_pi * rint(ph / two_pi);
    float sn, cs;
    sincosf((float)ph, &sn, &cs);
    hs[i] = make_float2((float)((double)cs / (double)row), (float)((double)sn / (double)row));
}

// md_fanout_kernel that also keeps the spectrum of its group
__global__ __launch_bounds__(ST_COL_NT) void dg_fanout_kernel(MsParams p, const float2* __restrict__ fld, StFanout q, StDistGrad r) {
    extern __shared__ cf dg_lds[];
    const int Py = p.gen_py, Px = p.gen_px, cw = st_cw(Py), ncg = (Px + cw - 1) / cw;
    const int bm = blockIdx.x / ncg, c0 = (blockIdx.x - bm * ncg) * cw;
    const int b = bm / p.n_modes, m = bm - b * p.n_modes;
    GenCtx g;
    st_col_ctx(g, dg_lds, p, c0, cw);
    const size_t row = (size_t)Py * Px;
    st_col_load(g, fld + (size_t)bm * row, Px, c0);
    __syncthreads();
    cf v[GEN_E], sp[GEN_E];
    st_col_fft<false>(g, p, v);
    float2* keep = r.keep + (size_t)bm * row;
#pragma unroll
    for (int j = 0; j < GEN_E; ++j) {
        const int i = g.tid + j * g.nt;
        if (j < g.ne && i < g.n) {
            const int y = i / g.Px;
            sp[j] = g.fld[i];
            keep[(size_t)y * Px + c0 + (i - y * g.Px)] = sp[j];
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

// md_fanin_kernel that also forms this workgroup's share of dL/dd_d, per d, before the conj(H_d) accumulate
__global__ __launch_bounds__(ST_COL_NT) void dg_fanin_kernel(MsParams p, float2* __restrict__ fld, StFanout q, StDistGrad r) {
    extern __shared__ cf dg_lds[];
    __shared__ double redd[ST_COL_NT / 64];
    const int Py = p.gen_py, Px = p.gen_px, cw = st_cw(Py), ncg = (Px + cw - 1) / cw;
    const int bm = blockIdx.x / ncg, c0 = (blockIdx.x - bm * ncg) * cw;
    const int b = bm / p.n_modes, m = bm - b * p.n_modes;
    GenCtx g;
    st_col_ctx(g, dg_lds, p, c0, cw);
    const size_t row = (size_t)Py * Px;
    const float2* keep = r.keep + (size_t)bm * row;
    cf v[GEN_E], acc[GEN_E];
#pragma unroll
    for (int j = 0; j < GEN_E; ++j) acc[j] = make_float2(0.f, 0.f);
    for (int d = 0; d < q.n; ++d) {
        const float2* hs = q.hs + (size_t)d * row;
        st_col_load(g, q.dfld + (((size_t)b * q.n + d) * p.n_modes + m) * row, Px, c0);
        __syncthreads();
        st_col_fft<false>(g, p, v);
        // the gradient's pass over this thread's elements first, a loop of its own (rolled: beside the 16 accumulators of the
        // unrolled pass below its operands no longer fit the registers), then md_fanin_kernel's accumulate as it stands there
        double dsum[1] = {0.0};
#pragma unroll 1
        for (int i = g.tid; i < g.n; i += g.nt) {
            const int y = i / g.Px, x = c0 + (i - y * g.Px);
            const size_t k = (size_t)y * Px + x;
            const cf a = g.fld[i];
            const cf w = cmul(keep[k], hs[k]);
            dsum[0] += (double)((r.ay[y] + r.ax[x]) * (a.x * w.y - a.y * w.x));
        }
#pragma unroll
        for (int j = 0; j < GEN_E; ++j) {
            const int i = g.tid + j * g.nt;
            if (j < g.ne && i < g.n) {
                const int y = i / g.Px;
                acc[j] = cadd(acc[j], cmulc(g.fld[i], hs[(size_t)y * Px + c0 + (i - y * g.Px)]));
            }
        }
        // (the barrier inside also stands between this distance's reads of redd on thread 0 and the next distance's writes: those
        // come behind the barrier that follows the next load)
        st_block_sum_f64(dsum, redd, g.tid, g.nt, true);
        if (g.tid == 0) r.part[(size_t)d * gridDim.x + blockIdx.x] = -dsum[0];
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

// grad_dists[d] += 1e7 * (the npart partials of distance d added in a fixed order); one workgroup
__global__ __launch_bounds__(256) void dg_reduce_kernel(const double* __restrict__ part, int npart, int n_dists, float* grad_dists) {
    __shared__ double red[256];
    const int t = threadIdx.x;
    for (int d = 0; d < n_dists; ++d) {
        double a = 0.0;
        for (int i = t; i < npart; i += 256) a += part[(size_t)d * npart + i];
        red[t] = a;
        __syncthreads();
        for (int h = 128; h > 0; h >>= 1) {
            if (t < h) red[t] += red[t + h];
            __syncthreads();
        }
        if (t == 0) grad_dists[d] += (float)(1e7 * red[0]);
        __syncthreads();
    }
}

static hipError_t dg_raise_lds() {
    static bool attr_set = false;
    if (attr_set) return hipSuccess;
    hipError_t e = st_col_raise_lds(dg_fanout_kernel);
    if (e == hipSuccess) e = st_col_raise_lds(dg_fanin_kernel);
    attr_set = e == hipSuccess;
    return e;
}

hipError_t ms_distgrad_table_launch(const StDistGeom& q, const float* dists_cm, float2* hs, float* ay, float* ax, hipStream_t st) {
    size_t n = (size_t)q.n * q.py * q.px;
    hipLaunchKernelGGL(dg_table_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, st, q, dists_cm, hs, ay, ax);
    return hipGetLastError();
}

static void dg_args(const StFanoutLaunch& fo, StFanout& q, StDistGrad& r) {
    q.hs = fo.hs; q.dfld = fo.fld; q.n = fo.n;
    r.keep = fo.keep; r.part = fo.part; r.ay = fo.ay; r.ax = fo.ax;
}

hipError_t ms_distgrad_fanout_launch(const MsParams& p, int batch, const float2* fld, const StFanoutLaunch& fo, hipStream_t st) {
    const StColGeom cg = st_col_geom(p.gen_py, p.gen_px);
    hipError_t e = dg_raise_lds();
    if (e != hipSuccess) return e;
    StFanout q;
    StDistGrad r;
    dg_args(fo, q, r);
    hipLaunchKernelGGL(dg_fanout_kernel, dim3((unsigned)(batch * p.n_modes * cg.ncg)), dim3((unsigned)cg.threads), cg.lds, st, p, fld, q, r);
    return hipGetLastError();
}

hipError_t ms_distgrad_fanin_launch(const MsParams& p, int batch, float2* fld, const StFanoutLaunch& fo, hipStream_t st) {
    const StColGeom cg = st_col_geom(p.gen_py, p.gen_px);
    hipError_t e = dg_raise_lds();
    if (e != hipSuccess) return e;
    StFanout q;
    StDistGrad r;
    dg_args(fo, q, r);
    hipLaunchKernelGGL(dg_fanin_kernel, dim3((unsigned)(batch * p.n_modes * cg.ncg)), dim3((unsigned)cg.threads), cg.lds, st, p, fld, q, r);
    return hipGetLastError();
}

hipError_t ms_distgrad_sum_launch(const MsParams& p, int batch, const StFanoutLaunch& fo, hipStream_t st) {
    const StColGeom cg = st_col_geom(p.gen_py, p.gen_px);
    hipLaunchKernelGGL(dg_reduce_kernel, dim3(1), dim3(256), 0, st, (const double*)fo.part, batch * p.n_modes * cg.ncg, fo.n, fo.grad_dists);
    return hipGetLastError();
}

}  // namespace adm
