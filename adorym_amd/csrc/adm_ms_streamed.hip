// Multislice forward + loss + adjoint for probes of any size up to 2048 x 2048: the fields of all (position, mode) pairs live
// in global memory ([B][M][Py][Px] complex, a section of the workspace) and every 2-D transform is a ROW launch and a COLUMN
// launch over all of them, with the element-wise work fused into those launches.  Spread over the chip like that, a minibatch of
// 32 positions of 256 x 256 fills every CU, where the one-workgroup-per-position kernels (adm_multislice.hip,
// adm_ms_generic.hip) stop at 128 x 128 (the field must fit one workgroup's LDS).
//
// Mathematics: exactly ms_generic_kernel's (adm_ms_generic.hip), which is the specification -- the stash conventions, H / (Py*Px)
// rounded once per element, det_scale / det_inverse, the fftshift-ed detector indexing, loss_term / loss_term_nz, det_weight,
// pre_t, binning with a partial last bin, the three detector modes, tile gradients summed over the modes in ascending order, one
// probe-gradient slot per position.  A 2-D transform here is the row transform and then the column transform (the inverse:
// columns, then rows); the same line passes (gen_pass, run-time radix lists) as the generic kernel, so the roundings differ from
// it only in the order of the two axes.
//
// Launch sequence of one minibatch, S = n_steps (4 S launches, + 2 each way for a Fresnel detector; far field, S = 1: four):
//   forward   row(s):  [row IFFT of the previous convolution] * t_s -> stash, [row FFT of the next convolution / detector]
//             col:     column FFT, * H / (Py*Px), column IFFT                        (between the steps)
//             Fresnel detector: one more col (H_free) and a row launch with the row IFFT only
//   detector  det:     per (b, column group), all modes: column transform, intensity over the modes, loss terms, pred,
//                      dL/dPsi, per-group loss partials; then per mode the adjoint's first column transform
//             reduce:  loss_sum[b] = the group partials of b in a fixed order
//   adjoint   [Fresnel: a row launch with the row FFT, col with conj(H_free)]
//             row(s), s descending: [pending row transform], tile gradient of step s (+= over the modes, in the workgroup),
//                      * conj(t_s), then the row FFT of the next convolution -- or, at s = 0, the probe-gradient slot
//             col:     the conj(H) convolution between the steps
//   then probe_grad_reduce sums the slots (adm_api.hip).
// A plan with probe shifts (adm_plan_set_probe_shift) puts three launches in front of the sweep and up to three behind it
// (adm_ms_probeshift.hip lists them).  A plan with a detector fan-out (adm_plan_set_detector_fanout) replaces the Fresnel detector's
// two column launches and runs the detector step over D entries per position (adm_ms_multidist.hip; with the gradient w.r.t. the
// distances requested: one reduce launch at the end).
//
// Row launches: one workgroup per (position, group of whole rows), all modes in turn (the slice factors are loaded once and the
// tile gradient of the modes is summed in registers).  Column launches: one workgroup per (position, mode, 8 adjacent columns;
// 4 beyond Py = 1024): every row of the group is a 64-byte (32-byte) run.  Workspace rows (stash, tile gradients) are pixel-major [Py][Px] like the generic
// kernel's, so the cover lists and the overlap-add (TileGeom::pixel_major) serve both.  What a column workgroup is made of (st_cw,
// its threads and LDS, the load / store / transform helpers) is in adm_ms_col.h, shared with the two shift files and adm_ms_multidist.hip.
#include <hip/hip_runtime.h>
#include "adm_host.h"
#include "adm_ms_col.h"

namespace adm {

constexpr int ST_ROW_NT = 256;                 // threads of a row workgroup
constexpr int ST_ROW_E = 8;                    // elements per thread in a row workgroup
constexpr int ST_ROW_ELEMS = ST_ROW_NT * ST_ROW_E;   // whole rows, at most this many elements (one row of 2048 at the largest)
constexpr int ST_MAX_SIDE = 2048;
constexpr int ST_MAX_SLICES = 1024;         // most slices of a sparse plan (st_dd_reduce_kernel keeps one sum per gap in LDS)

// row transform passes of the line group in LDS (INV: conjugate twiddles)
template <bool INV, int E> __device__ __forceinline__ void st_row_fft(const GenCtx& g, const MsParams& p, cf (&v)[E]) {
    int Ns = 1;
    for (int s = 0; s < p.gen_nrx; ++s) { gen_pass<false, INV, E>(g, p.gen_rx[s], Ns, v); Ns *= p.gen_rx[s]; }
}
// dir: 0 none, 1 forward, 2 inverse
template <int E> __device__ __forceinline__ void st_row_dir(const GenCtx& g, const MsParams& p, int dir, cf (&v)[E]) {
    if (dir == 1) st_row_fft<false>(g, p, v);
    else if (dir == 2) st_row_fft<true>(g, p, v);
}
__device__ __forceinline__ void st_col_dir(const GenCtx& g, const MsParams& p, int dir, cf (&v)[GEN_E]) {
    if (dir == 1) st_col_fft<false>(g, p, v);
    else if (dir == 2) st_col_fft<true>(g, p, v);
}

struct StRow {
    int rows;          // rows per workgroup
    int step;          // modulation step (mode 1, 2)
    int mode;          // 0 transforms only, 1 forward (modulation, stash), 2 adjoint (tile gradient, conjugate modulation)
    int pre, post;     // row transform before / after the element-wise work: 0 none, 1 forward, 2 inverse
    int from_probe;    // read the probe modes instead of the field buffer (first forward step)
    int to_gprobe;     // write the position's probe-gradient slots instead of the field buffer (last adjoint step)
};

__global__ __launch_bounds__(ST_ROW_NT) void st_row_kernel(MsParams p, StRow r, float2* __restrict__ fld) {
    __shared__ cf lds[ST_ROW_ELEMS + ST_MAX_SIDE];
    const int Py = p.gen_py, Px = p.gen_px;
    const int ngr = (Py + r.rows - 1) / r.rows;
    const int b = blockIdx.x / ngr, r0 = (blockIdx.x - b * ngr) * r.rows;
    GenCtx g;
    g.Py = min(r.rows, Py - r0); g.Px = Px; g.n = g.Py * Px;
    g.tid = threadIdx.x; g.nt = ST_ROW_NT;
    g.ne = (g.n + g.nt - 1) / g.nt;
    g.fld = lds;
    cf* twx = lds + ST_ROW_ELEMS;
    for (int i = g.tid; i < Px; i += g.nt) twx[i] = p.twid[i];
    g.twx = twx; g.twy = nullptr;
    const int M = p.n_modes;
    const bool RI = p.real_imag != 0;
    const size_t row = (size_t)Py * Px, per = (size_t)p.n_steps * row, off0 = (size_t)r0 * Px;
    const int2 ps = p.pos[b];
    const size_t slice_stride = (size_t)p.Yp * p.Xp;
    const float2* tile = p.obj_rot + (size_t)(ps.x + p.pad_y0 + r0) * p.Xp + (ps.y + p.pad_x0);
    cf v[ST_ROW_E], tv[ST_ROW_E];
    float2 gacc[ST_ROW_E];
    const float sk1 = p.sigma * p.k1;
    for (int m = 0; m < M; ++m) {
        const float2* src = r.from_probe ? p.probe + (size_t)m * row : fld + ((size_t)b * M + m) * row;
        for (int i = g.tid; i < g.n; i += g.nt) lds[i] = src[off0 + i];
        __syncthreads();
        st_row_dir(g, p, r.pre, v);
        if (r.mode != 0) {
            float2* stash = p.stash + ((size_t)b * M + m) * per + (size_t)r.step * row + off0;
#pragma unroll
            for (int j = 0; j < ST_ROW_E; ++j) {
                const int i = g.tid + j * g.nt;
                if (j < g.ne && i < g.n) {
                    if (m == 0) {       // the slice factor of this pixel, kept for the other modes
                        const int y = i / Px;
                        const float2 db = gen_slice(p, tile, slice_stride, r.step, (size_t)y * p.Xp + (i - y * Px));
                        tv[j] = (RI || p.pre_t) ? db : gen_modulator(db, p.k1, p.sigma);
                    }
                    cf a = lds[i];
                    if (r.mode == 1) {
                        if (RI) {
                            if (p.want_grad) stash[i] = a;      // pre-modulation field
                            a = cmul(a, tv[j]);
                        } else {
                            a = cmul(a, tv[j]);
                            if (p.want_grad) stash[i] = a;      // post-modulation field
                        }
                    } else {
                        const cf psi = stash[i];
                        const float zr = a.x * psi.x + a.y * psi.y;
                        const float zi = a.x * psi.y - a.y * psi.x;
                        float2 gr = make_float2(RI ? zr : sk1 * zi, RI ? -zi : -p.k1 * zr);
                        if (m > 0) { gr.x += gacc[j].x; gr.y += gacc[j].y; }
                        gacc[j] = gr;
                        a = cmulc(a, tv[j]);
                    }
                    lds[i] = a;
                }
            }
            __syncthreads();
        }
        st_row_dir(g, p, r.post, v);
        float2* dst = fld + ((size_t)b * M + m) * row;
        if (r.to_gprobe) dst = p.grad_probe ? p.grad_probe + (size_t)b * p.gprobe_bstride + (size_t)m * row : nullptr;
        if (dst)
            for (int i = g.tid; i < g.n; i += g.nt) dst[off0 + i] = lds[i];
        __syncthreads();
    }
    if (r.mode == 2) {
        float2* gtile = p.gtile + (size_t)b * per + (size_t)r.step * row + off0;
#pragma unroll
        for (int j = 0; j < ST_ROW_E; ++j) {
            const int i = g.tid + j * g.nt;
            if (j < g.ne && i < g.n) gtile[i] = gacc[j];
        }
    }
}

// field <- column IFFT( H * column FFT(field) ) for one (position, mode, column group); hs = H / (Py*Px) (CONJ: conj)
template <bool CONJ> __global__ __launch_bounds__(ST_COL_NT) void st_col_conv_kernel(MsParams p, float2* __restrict__ fld, const float2* __restrict__ hs) {
    extern __shared__ cf st_lds[];
    const int Px = p.gen_px;
    GenCtx g;
    const auto [bm, c0] = st_col_begin(g, st_lds, p);
    float2* f = fld + (size_t)bm * p.gen_py * Px;
    st_col_load(g, f, Px, c0);
    __syncthreads();
    cf v[GEN_E];
    st_col_fft<false>(g, p, v);
#pragma unroll
    for (int j = 0; j < GEN_E; ++j) {
        const int i = g.tid + j * g.nt;
        if (j < g.ne && i < g.n) {
            const int y = i / g.Px;
            g.fld[i] = cmul_t<CONJ>(g.fld[i], hs[(size_t)y * Px + c0 + (i - y * g.Px)]);
        }
    }
    __syncthreads();
    st_col_fft<true>(g, p, v);
    st_col_store(g, f, Px, c0);
}

// detector plane of one (position, column group), all modes: column transform, loss, pred, dL/dPsi, adjoint column transform
__global__ __launch_bounds__(ST_COL_NT) void st_det_kernel(MsParams p, float2* __restrict__ fld, float* __restrict__ part) {
    extern __shared__ cf st_lds[];
    __shared__ float red[ST_COL_NT / 64];
    const int Py = p.gen_py, Px = p.gen_px, cw = st_cw(Py);
    GenCtx g;
    const StColWg wg = st_col_begin(g, st_lds, p);      // (one workgroup per position and column group: all modes)
    const int b = wg.bm, c0 = wg.c0;
    const int M = p.n_modes;
    const bool far = p.det_mode == ADM_DET_FARFIELD_;
    const int fwd_dir = far ? (p.det_inverse ? 2 : 1) : 0, adj_dir = far ? (p.det_inverse ? 1 : 2) : 0;
    const size_t row = (size_t)Py * Px;
    cf v[GEN_E];
    // per element: the intensity summed over the modes, then the factor g of dL/dPsi = g * Psi (LDS, behind the twiddles: in
    // registers the detector state spills)
    float* gf = reinterpret_cast<float*>(st_lds + (size_t)Py * cw + Py);
    auto gidx = [&](int i) { const int y = i / g.Px; return (size_t)y * Px + c0 + (i - y * g.Px); };
    for (int m = 0; m < M; ++m) {
        if (m > 0) __syncthreads();
        st_col_load(g, fld + ((size_t)b * M + m) * row, Px, c0);
        __syncthreads();
        st_col_dir(g, p, fwd_dir, v);
        if (M > 1) {
            float2* dq = p.det + ((size_t)b * M + m) * row;
#pragma unroll
            for (int j = 0; j < GEN_E; ++j) {
                const int i = g.tid + j * g.nt;
                if (j < g.ne && i < g.n) {
                    const cf psi = far ? cscale(g.fld[i], p.det_scale) : g.fld[i];
                    const float q = psi.x * psi.x + psi.y * psi.y;
                    gf[i] = m > 0 ? gf[i] + q : q;
                    dq[gidx(i)] = psi;
                }
            }
        }
    }
    float lsum = 0.f;
#pragma unroll
    for (int j = 0; j < GEN_E; ++j) {
        const int i = g.tid + j * g.nt;
        if (j < g.ne && i < g.n) {
            const int ky = i / g.Px, kx = c0 + (i - ky * g.Px);
            // far field: natural-order spectrum element (ky, kx) is the fftshifted detector pixel ((ky + Py/2) % Py, ...)
            const int my = far ? (ky + Py / 2) % Py : ky, mx = far ? (kx + Px / 2) % Px : kx;
            const size_t di = ((size_t)b * Py + my) * Px + mx;
            const bool drop = p.det_weight && p.det_weight[my * Px + mx] == 0.f;    // dropped, not weighted: the data there may be NaN
            float mag;
            if (M > 1) mag = sqrtf(gf[i]);
            else {
                const cf psi = far ? cscale(g.fld[i], p.det_scale) : g.fld[i];
                mag = sqrtf(psi.x * psi.x + psi.y * psi.y);
            }
            float gg;
            const float term = M > 1 ? loss_term_nz(mag, p.target[di], p, gg) : loss_term(mag, p.target[di], p, gg);
            lsum += drop ? 0.f : term;
            if (p.pred) p.pred[di] = mag;
            gf[i] = drop ? 0.f : gg;
        }
    }
    {
        const float s = gen_block_sum(lsum, red, g.tid, g.nt);
        if (g.tid == 0) part[blockIdx.x] = s;
    }
    if (!p.want_grad) return;
    for (int m = 0; m < M; ++m) {
        __syncthreads();
#pragma unroll
        for (int j = 0; j < GEN_E; ++j) {
            const int i = g.tid + j * g.nt;
            if (j < g.ne && i < g.n) {
                // Psi = scale * F(psi): the adjoint of (scale * F) applied to g * Psi is scale * F^H (g * scale * F psi)
                const cf psi = (M > 1) ? p.det[((size_t)b * M + m) * row + gidx(i)] : (far ? cscale(g.fld[i], p.det_scale) : g.fld[i]);
                g.fld[i] = cscale(psi, gf[i] * (far ? p.det_scale : 1.f));
            }
        }
        __syncthreads();
        st_col_dir(g, p, adj_dir, v);
        st_col_store(g, fld + ((size_t)b * M + m) * row, Px, c0);
    }
}

// ---------------------------------------------------------------------------------------------------------------------------
// Sparse multislice (adm_plan_set_slice_positions): the slices sit at arbitrary depths z_s, so convolution s has a transfer
// function of its own, H_s = exp(i a d_s) with d_s = (z_{s+1} - z_s) * 1e7 nm and a = -sigma PI lambda (u^2 + v^2) per nm.  The
// table hs[S-1][Py][Px] = H_s / (Py*Px) is built on the device from z as it lives there; the forward and adjoint sweeps are the
// launches above with hs + s*Py*Px.  When dL/dz is wanted, the column launches are the two kernels below instead: the forward
// one keeps H_s Psihat'_s / (Py*Px) (in LDS after the multiply), the adjoint one holds Ghat after its column transform and sums
//   dL/dd_s = - sum_k a_k Im( conj(Ghat_k) * kept_k )
// over its elements (products in fp32, sums in fp64), ONE partial per workgroup; st_dd_reduce_kernel adds the partials of a
// step in a fixed order and accumulates dL/dz_j = 1e7 (dL/dd_{j-1} - dL/dd_j) into the caller's buffer.  No atomics.

// hs[s][y][x] = exp(i a_yx d_s) / (Py*Px): the phase (hundreds of radians at 10 um gaps) in fp64, reduced to one turn, then
// sin / cos in fp32 and one rounding for the division.  ay[y] + ax[x] = a_yx for the gradient kernels (fp32).  d_s: the gap between
// slice positions s and s + 1 (q.gaps), or detector distance s of a fan-out whose distances are refined (adm_ms_multidist.hip).
__global__ __launch_bounds__(256) void st_fresnel_table_kernel(StFresnelGeom q, const float* __restrict__ src, float2* __restrict__ hs,
                                                                float* __restrict__ ay, float* __restrict__ ax) {
    const size_t row = (size_t)q.py * q.px, n = (size_t)q.n * row;
    const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
    const double c = -q.sigma * 3.14159265359 * q.lambda_nm;
    if (i < (size_t)q.py) { const double u = (double)st_freq_index((int)i, q.py) / q.py / q.voxel_nm_y; ay[i] = (float)(c * u * u); }
    if (i < (size_t)q.px) { const double v = (double)st_freq_index((int)i, q.px) / q.px / q.voxel_nm_x; ax[i] = (float)(c * v * v); }
    if (i >= n) return;
    const int s = (int)(i / row);
    const int y = (int)((i - (size_t)s * row) / q.px), x = (int)(i - (size_t)s * row - (size_t)y * q.px);
    const double u = (double)st_freq_index(y, q.py) / q.py / q.voxel_nm_y, v = (double)st_freq_index(x, q.px) / q.px / q.voxel_nm_x;
    const double d = q.gaps ? ((double)src[s + 1] - (double)src[s]) * 1e7 : (double)src[s] * 1e7;
    double ph = c * (u * u + v * v) * d;
    const double two_pi = 6.283185307179586476925287;
    ph -= two_pi * rint(ph / two_pi);
    float sn, cs;
    sincosf((float)ph, &sn, &cs);
    hs[i] = make_float2((float)((double)cs / (double)row), (float)((double)sn / (double)row));
}

// z <- z - z[0] (adorym/optimizers.py:1059)
__global__ __launch_bounds__(256) void st_sparse_anchor_kernel(float* z, int n) {
    const float z0 = z[0];
    __syncthreads();
    for (int i = threadIdx.x; i < n; i += 256) z[i] -= z0;
}

// st_col_conv_kernel for the convolution `step` of a sparse plan when dL/dz is wanted.  Forward: keeps the multiplied spectrum.
// Adjoint (CONJ): forms this workgroup's share of dL/dd_step before the multiply.
template <bool CONJ> __global__ __launch_bounds__(ST_COL_NT) void st_col_conv_sparse_kernel(MsParams p, float2* __restrict__ fld,
                                                                                             const float2* __restrict__ hs, StSparse q) {
    extern __shared__ cf st_lds[];
    __shared__ double redd[ST_COL_NT / 64];
    const int Px = p.gen_px;
    GenCtx g;
    const auto [bm, c0] = st_col_begin(g, st_lds, p);
    const size_t row = (size_t)p.gen_py * Px;
    float2* f = fld + (size_t)bm * row;
    float2* keep = q.keep + ((size_t)bm * q.n_conv + q.step) * row;
    st_col_load(g, f, Px, c0);
    __syncthreads();
    cf v[GEN_E];
    st_col_fft<false>(g, p, v);
    double acc[1] = {0.0};
#pragma unroll
    for (int j = 0; j < GEN_E; ++j) {
        const int i = g.tid + j * g.nt;
        if (j < g.ne && i < g.n) {
            const int y = i / g.Px, x = c0 + (i - y * g.Px);
            const size_t k = (size_t)y * Px + x;
            const cf a = g.fld[i];
            if (CONJ) {
                const cf w = keep[k];
                acc[0] += (double)((q.ay[y] + q.ax[x]) * (a.x * w.y - a.y * w.x));
                g.fld[i] = cmulc(a, hs[k]);
            } else {
                const cf w = cmul(a, hs[k]);
                keep[k] = w;
                g.fld[i] = w;
            }
        }
    }
    st_block_sum_f64(acc, redd, g.tid, g.nt, CONJ);
    if (CONJ && g.tid == 0) q.part[(size_t)q.step * gridDim.x + blockIdx.x] = -acc[0];
    st_col_fft<true>(g, p, v);
    st_col_store(g, f, Px, c0);
}

// dL/dd_s = the npart partials of step s added in a fixed order (one workgroup), s < n; then, per cm,
//   gaps != 0 (sparse plans, d_s the gap behind slice s):        out[j] += 1e7 * (dL/dd_{j-1} - dL/dd_j),  j <= n   (dL/dz)
//   gaps == 0 (fan-out, d_s detector distance s; n <= 64):       out[s] += 1e7 * dL/dd_s
__global__ __launch_bounds__(256) void st_dd_reduce_kernel(const double* __restrict__ part, int npart, int n, int gaps, float* out) {
    __shared__ double red[256];
    __shared__ double gd[ST_MAX_SLICES];
    const int t = threadIdx.x;
    for (int s = 0; s < n; ++s) {
        double a = 0.0;
        for (int i = t; i < npart; i += 256) a += part[(size_t)s * npart + i];
        red[t] = a;
        __syncthreads();
        for (int h = 128; h > 0; h >>= 1) {
            if (t < h) red[t] += red[t + h];
            __syncthreads();
        }
        if (t == 0) gd[s] = red[0];
        __syncthreads();
    }
    if (gaps) {
        for (int j = t; j <= n; j += 256) {
            const double d = (j > 0 ? gd[j - 1] : 0.0) - (j < n ? gd[j] : 0.0);
            out[j] += (float)(1e7 * d);
        }
    } else {
        for (int d = t; d < n; d += 256) out[d] += (float)(1e7 * gd[d]);
    }
}

// The dL/ds partials of the shift kernels (adm_ms_exitshift.hip, adm_ms_probeshift.hip; [B*M*column groups][2], index: the entry of
// position b, or nullptr: b):
// grad_shifts[e] += 2 PI * (the partials of every position that uses entry e: ascending position, then mode, then column group).
// One workgroup per position; the first position of an entry gathers for it, the others leave.  per = n_modes * column groups.
__global__ __launch_bounds__(256) void st_shift_reduce_kernel(const double* __restrict__ part, int batch, int per,
                                                              const int* __restrict__ index, float* grad_shifts) {
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

// loss_sum[b] = the column-group partials of position b, ascending (loss_sum may be host-mapped memory)
__global__ __launch_bounds__(256) void st_loss_reduce_kernel(const float* __restrict__ part, int ncg, int batch, float* loss_sum) {
    const int b = blockIdx.x * 256 + threadIdx.x;
    if (b >= batch) return;
    float s = 0.f;
    for (int c = 0; c < ncg; ++c) s += part[(size_t)b * ncg + c];
    loss_sum[b] = s;
}

bool ms_streamed_supported(int py, int px) { return py >= 1 && px >= 1 && py <= ST_MAX_SIDE && px <= ST_MAX_SIDE; }
int ms_streamed_col_groups(int py, int px) { return st_col_geom(py, px).ncg; }

hipError_t ms_fresnel_table_launch(const StFresnelGeom& q, const float* src_cm, float2* hs, float* ay, float* ax, hipStream_t st) {
    size_t n = (size_t)q.n * q.py * q.px;
    if (n < (size_t)(q.py > q.px ? q.py : q.px)) n = q.py > q.px ? q.py : q.px;      // (ay and ax are filled whatever n is)
    hipLaunchKernelGGL(st_fresnel_table_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, st, q, src_cm, hs, ay, ax);
    return hipGetLastError();
}
hipError_t ms_sparse_anchor_launch(float* z, int n, hipStream_t st) {
    hipLaunchKernelGGL(st_sparse_anchor_kernel, dim3(1), dim3(256), 0, st, z, n);
    return hipGetLastError();
}
int ms_sparse_max_slices() { return ST_MAX_SLICES; }

hipError_t ms_streamed_launch(const MsParams& p, int batch, float2* fld, float* part, hipStream_t st, const StSparseLaunch* sp,
                              const StExitShiftLaunch* xs, const StFanoutLaunch* fo, const StProbeShiftLaunch* ps) {
    const int Py = p.gen_py, Px = p.gen_px, S = p.n_steps, M = p.n_modes;
    if (!ms_streamed_supported(Py, Px)) return hipErrorInvalidValue;
    // exit-wave shifts (adm_ms_exitshift.hip): a far-field magnitude does not see them; an exit-wave detector takes the Fresnel
    // sequence with H = 1
    const bool far = p.det_mode == ADM_DET_FARFIELD_;
    if (far) xs = nullptr;
    const bool fresnel = p.det_mode == ADM_DET_FRESNEL_ || xs;
    const float2* hfree_s = p.det_mode == ADM_DET_FRESNEL_ ? p.gen_hfree_s : nullptr;
    int rows = ST_ROW_ELEMS / Px;
    if (rows < 1) rows = 1;
    if (rows > Py) rows = Py;
    const StColGeom cg = st_col_geom(Py, Px);
    const int ngr = (Py + rows - 1) / rows, ncg = cg.ncg;
    static bool raised = false;
    hipError_t e = st_col_raise_lds_once(raised, st_col_conv_kernel<false>, st_col_conv_kernel<true>, st_det_kernel,
                                         st_col_conv_sparse_kernel<false>, st_col_conv_sparse_kernel<true>);
    if (e != hipSuccess) return e;
    auto row = [&](int step, int mode, int pre, int post, int from_probe, int to_gprobe) {
        StRow r;
        r.rows = rows; r.step = step; r.mode = mode; r.pre = pre; r.post = post; r.from_probe = from_probe; r.to_gprobe = to_gprobe;
        hipLaunchKernelGGL(st_row_kernel, dim3(batch * ngr), dim3(ST_ROW_NT), 0, st, p, r, fld);
        return hipGetLastError();
    };
    auto col = [&](const float2* h, bool conj) {
        return st_col_launch(conj ? st_col_conv_kernel<true> : st_col_conv_kernel<false>, cg, batch * M, st, p, fld, h);
    };
    // convolution `step` of the slice loop: the plan's one H, or a sparse plan's H_step -- through the kernels that also keep the
    // spectrum / form the dL/dd partials when the slice-position gradient is wanted
    const size_t frow = (size_t)Py * Px;
    const bool zgrad = sp && sp->grad_z && p.want_grad && S > 1;
    auto conv = [&](int step, bool conj) {
        if (!sp) return col(p.gen_hs, conj);
        const float2* h = sp->hs + (size_t)step * frow;
        if (!zgrad) return col(h, conj);
        StSparse q;
        q.keep = sp->keep; q.part = sp->part; q.ay = sp->ay; q.ax = sp->ax; q.step = step; q.n_conv = S - 1;
        return st_col_launch(conj ? st_col_conv_sparse_kernel<true> : st_col_conv_sparse_kernel<false>, cg, batch * M, st, p, fld, h, q);
    };
    // detector fan-out (adm_ms_multidist.hip): the detector step sends every sweep field to fo->n planes; the row launches around
    // the detector kernel, that kernel and the loss reduction then run over the batch * fo->n detector entries
    MsParams pd = p;
    if (fo) { pd.pos = fo->pos; pd.det = fo->det; }
    auto det_row_only = [&](int pre) {
        StRow r;
        r.rows = rows; r.step = 0; r.mode = 0; r.pre = pre; r.post = 0; r.from_probe = 0; r.to_gprobe = 0;
        hipLaunchKernelGGL(st_row_kernel, dim3(batch * fo->n * ngr), dim3(ST_ROW_NT), 0, st, pd, r, fo->fld);
        return hipGetLastError();
    };
    // (p, batch, fld: the sweep's own, or -- with a fan-out -- the detector entries'; the names of the outer ones on purpose)
    StColGeom dg = cg;
    dg.lds += (size_t)Py * cg.cw * sizeof(float);      // (the detector kernel's per-element factor behind the twiddles)
    auto detect = [&](const MsParams& p, int batch, float2* fld) {
        hipError_t e = st_col_launch(st_det_kernel, dg, batch, st, p, fld, part);
        if (e != hipSuccess) return e;
        hipLaunchKernelGGL(st_loss_reduce_kernel, dim3((batch + 255) / 256), dim3(256), 0, st, part, ncg, batch, p.loss_sum);
        return hipGetLastError();
    };
    auto det_col = [&](bool conj) { return xs ? ms_exitshift_col_launch(p, batch, fld, hfree_s, conj, *xs, st) : col(hfree_s, conj); };
    // sub-pixel probe positions: Phat = FFT2(probe) once, then the fields of every (position, mode) up to their row IFFT, which
    // the first row launch of the sweep does in front of its modulation
    StProbeShift pq;
    if (ps) {
        pq.shifts = (const float2*)ps->shifts; pq.index = ps->index; pq.phat = ps->phat; pq.part = nullptr;
        StRow r;
        r.rows = rows; r.step = 0; r.mode = 0; r.pre = 0; r.post = 1; r.from_probe = 1; r.to_gprobe = 0;
        hipLaunchKernelGGL(st_row_kernel, dim3(ngr), dim3(ST_ROW_NT), 0, st, p, r, ps->phat);
        if ((e = hipGetLastError()) != hipSuccess) return e;
        if ((e = ms_probeshift_spectrum_launch(p, ps->phat, st)) != hipSuccess) return e;
        if ((e = ms_probeshift_col_launch(p, batch, fld, false, pq, st)) != hipSuccess) return e;
    }
    // ---------------- forward ----------------
    const int det_row = far ? (p.det_inverse ? 2 : 1) : (fresnel ? 1 : 0);     // the row transform that starts the detector propagation
    for (int s = 0; s < S && e == hipSuccess; ++s) {
        e = row(s, 1, s > 0 || ps ? 2 : 0, s < S - 1 ? 1 : det_row, s == 0 && !ps, 0);
        if (e == hipSuccess && s < S - 1) e = conv(s, false);
    }
    if (e == hipSuccess && fresnel) {
        e = fo ? ms_multidist_fanout_launch(p, batch, fld, *fo, st) : det_col(false);
        if (e == hipSuccess) e = fo ? det_row_only(2) : row(0, 0, 2, 0, 0, 0);
    }
    if (e != hipSuccess) return e;
    // ---------------- detector, loss ----------------
    e = fo ? detect(pd, batch * fo->n, fo->fld) : detect(p, batch, fld);
    if (e != hipSuccess || !p.want_grad) return e;
    // ---------------- adjoint ----------------
    if (fresnel) {
        e = fo ? det_row_only(1) : row(0, 0, 1, 0, 0, 0);
        if (e == hipSuccess) e = fo ? ms_multidist_fanin_launch(p, batch, fld, *fo, st) : det_col(true);
    }
    const int adj_row = far ? (p.det_inverse ? 1 : 2) : (fresnel ? 2 : 0);
    // (probe shifts: the last row launch ends with the row FFT of the shift's adjoint and leaves the field in the buffer)
    const bool ps_adj = ps && (p.grad_probe || ps->grad_shifts);
    for (int s = S - 1; s >= 0 && e == hipSuccess; --s) {
        e = row(s, 2, s == S - 1 ? adj_row : 2, s > 0 || ps_adj ? 1 : 0, 0, s == 0 && !ps_adj);
        if (e == hipSuccess && s > 0) e = conv(s - 1, true);
    }
    if (e == hipSuccess && ps_adj) {
        pq.part = ps->grad_shifts ? ps->part : nullptr;
        e = ms_probeshift_col_launch(p, batch, fld, true, pq, st);
        if (e == hipSuccess && p.grad_probe) e = row(0, 0, 2, 0, 0, 1);
        if (e == hipSuccess && ps->grad_shifts) {
            hipLaunchKernelGGL(st_shift_reduce_kernel, dim3(batch), dim3(256), 0, st, ps->part, batch, M * ncg, ps->index, ps->grad_shifts);
            e = hipGetLastError();
        }
    }
    if (e == hipSuccess && zgrad) {
        hipLaunchKernelGGL(st_dd_reduce_kernel, dim3(1), dim3(256), 0, st, sp->part, batch * M * ncg, S - 1, 1, sp->grad_z);
        e = hipGetLastError();
    }
    if (e == hipSuccess && fo && fo->grad_dists) {
        hipLaunchKernelGGL(st_dd_reduce_kernel, dim3(1), dim3(256), 0, st, fo->part, batch * M * ncg, fo->n, 0, fo->grad_dists);
        e = hipGetLastError();
    }
    if (e == hipSuccess && xs && xs->grad_shifts) {
        hipLaunchKernelGGL(st_shift_reduce_kernel, dim3(batch), dim3(256), 0, st, xs->part, batch, M * ncg, xs->index, xs->grad_shifts);
        e = hipGetLastError();
    }
    return e;
}

}  // namespace adm
