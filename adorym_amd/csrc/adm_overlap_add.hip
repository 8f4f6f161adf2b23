// Overlap-add of the per-position tile gradients into the rotated-frame gradient: cover lists per pixel, then a gather.
#include <hip/hip_runtime.h>
#include "adm_host.h"
#include "adm_ms_math.h"

namespace adm {
// --------------------------------------------------------------------------------------------
// Overlap-add of the per-position tile gradients written by the multislice kernel (adjoint of the
// tile gather, adorym/forward_model.py:313-331).  Tiles overlap, so this is a gather per rotated-frame
// pixel over the positions that cover it: deterministic, no atomics.
//   cover_build_kernel : per padded pixel (y, x) the list of (position, element) sources
//   tile_accumulate_kernel : grad_rot[s][y][x] = sum of the sources, for every slice
// gtile layout per position: [step] rows of R1 x NT elements, element (k, tid) at ws_elem_offset() (adm_ms_math.h), with
// pixel (row, col) -> k = col / R2, tid = (row / LPW) * 64 + (row % LPW) * G + col % R2 (the multislice kernel's
// thread-native order).
// --------------------------------------------------------------------------------------------

struct TileGeom {
    int Yp, Xp, pad_y0, pad_x0, Py, Px, R1, R2, G, LPW, NT, n_steps, binning, Z;
    int pixel_major;      // rows written by the generic kernel: [Py][Px]; else the tuned kernels' thread-native order
    int row_elems;        // float2 elements of one row (one modulation step of one position)
    int row0, nrows;      // padded-row window touched by the batch
    int add_lo, add_hi;   // padded rows [add_lo, add_hi) already hold an earlier part of the same batch: accumulate there
};

// positions [b0, B) of the batch enter the lists (b0 > 0: one pass of a batch whose coverage exceeds ADM_MAXCOVER, see
// adm_tile_grad_accumulate_range)
__global__ __launch_bounds__(256) void cover_build_kernel(const int2* __restrict__ pos, int b0, int B, TileGeom g,
                                                          unsigned* __restrict__ cover, int* __restrict__ overflow) {
    // The positions are read 256 at a time, and only those whose tile reaches this block's 32 x 8 pixels go on -- in position
    // order (ballot + prefix count per wave) -- to the per-pixel loop: a pixel used to walk ALL positions of the batch, one
    // dependent load each (15 us per 64 positions whatever the number of pixels; 29 us for the 200 entries of a tiled
    // multi-distance launch, longer than the multislice kernel beside it).
    __shared__ int2 sp[256];
    __shared__ int sb[256];
    __shared__ int wcnt[4];
    const int x = blockIdx.x * 32 + (threadIdx.x & 31);
    const int r = blockIdx.y * 8 + (threadIdx.x >> 5);
    const bool live = x < g.Xp && r < g.nrows;
    const int y = g.row0 + r;
    const int bx_lo = blockIdx.x * 32, by_lo = g.row0 + blockIdx.y * 8;         // the block's pixels: [bx_lo, +32) x [by_lo, +8)
    // structure-of-arrays: entry c of pixel (r, x) at cover[(c * nrows + r) * Xp + x], so that the lanes of a wave
    // (consecutive x) read consecutive words
    const size_t cplane = (size_t)g.nrows * g.Xp;
    unsigned* out = cover + (size_t)(live ? r : 0) * g.Xp + (live ? x : 0);
    int cnt = 0;
    const unsigned per_pos = (unsigned)g.n_steps * g.row_elems;
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    for (int c0 = b0; c0 < B; c0 += 256) {
        const int b = c0 + (int)threadIdx.x;
        int2 p = make_int2(0, 0);
        bool hit = false;
        if (b < B) {
            p = pos[b];
            const int ty = p.x + g.pad_y0, tx = p.y + g.pad_x0;                   // the tile's first padded row / column
            hit = ty < by_lo + 8 && ty + g.Py > by_lo && tx < bx_lo + 32 && tx + g.Px > bx_lo;
        }
        const unsigned long long m = __ballot(hit);
        __syncthreads();                                                          // (the previous chunk's candidates are consumed)
        if (lane == 0) wcnt[wave] = __popcll(m);
        __syncthreads();
        int off = 0, n = 0;
#pragma unroll
        for (int w = 0; w < 4; ++w) { if (w < wave) off += wcnt[w]; n += wcnt[w]; }
        if (hit) {
            const int k = off + __popcll(m & ((1ull << lane) - 1ull));
            sp[k] = p;
            sb[k] = b;
        }
        __syncthreads();
        if (!live) continue;
        for (int j = 0; j < n; ++j) {
            const int2 q = sp[j];
            const int row = y - (q.x + g.pad_y0), col = x - (q.y + g.pad_x0);
            if (row >= 0 && row < g.Py && col >= 0 && col < g.Px) {
                if (cnt < ADM_MAXCOVER) {
                    unsigned off_e;
                    if (g.pixel_major) off_e = (unsigned)(row * g.Px + col);
                    else {
                        const int tid = (row / g.LPW) * 64 + (row % g.LPW) * g.G + col % g.R2;
                        off_e = adm::ws_elem_offset(g.R1, g.NT, col / g.R2, tid);
                    }
                    out[(size_t)(1 + cnt) * cplane] = (unsigned)sb[j] * per_pos + off_e;
                }
                ++cnt;
            }
        }
    }
    if (!live) return;
    if (cnt > ADM_MAXCOVER) { atomicExch(overflow, 1); cnt = ADM_MAXCOVER; }
    out[0] = (unsigned)cnt;
}

// One thread owns one padded pixel and TA_STEPS consecutive modulation steps: for every covering tile it issues TA_STEPS
// independent 8-B loads (stride = one step of that tile) before touching the accumulators (TA_CU > 1: of TA_CU tiles at a
// time).  With the XCD-aware grid below the kernel is bound by how much of a fetched line its neighbours still find in
// their L2, so FEWER steps per block are better: 256 positions take 0.76 / 0.87 / 1.01 ms at TA_STEPS 2 / 4 / 8 (round 1,
// blockIdx = (x, y, z): 0.97 at 4, the best of 2/4/8/16 then); TA_CU 2-8 and an x loop inside the block change nothing.
#ifndef TA_STEPS
#define TA_STEPS 2
#endif
#ifndef TA_CU
#define TA_CU 1
#endif
// the work of one block of tile_accumulate_kernel: step chunk zc, pixel block `rem` (x fastest)
__device__ __forceinline__ void ta_block(const float2* __restrict__ gtile, const unsigned* __restrict__ cover, float2* __restrict__ grad_rot,
                                         const TileGeom& g, int zc, int rem) {
    const int nbx = (g.Xp + 31) / 32;
    const int x = (rem % nbx) * 32 + (threadIdx.x & 31);
    const int r = (rem / nbx) * 8 + (threadIdx.x >> 5);
    if (x >= g.Xp || r >= g.nrows) return;
    const size_t cplane = (size_t)g.nrows * g.Xp;
    const unsigned* cv = cover + (size_t)r * g.Xp + x;
    const int cnt = (int)cv[0];
    const size_t step_stride = (size_t)g.row_elems;
    const size_t slice_stride = (size_t)g.Yp * g.Xp;
    float2* out = grad_rot + (size_t)(g.row0 + r) * g.Xp + x;
    const bool add = (g.row0 + r >= g.add_lo) && (g.row0 + r < g.add_hi);
    const int st0 = zc * TA_STEPS;
    const int nst = min(TA_STEPS, g.n_steps - st0);
    float2 acc[TA_STEPS];
#pragma unroll
    for (int i = 0; i < TA_STEPS; ++i) acc[i] = make_float2(0.f, 0.f);
    if (nst == TA_STEPS) {
        int c = 0;
        for (; c + TA_CU <= cnt; c += TA_CU) {         // TA_CU tiles x TA_STEPS steps in flight; added in list order
            float2 v[TA_CU][TA_STEPS];
#pragma unroll
            for (int u = 0; u < TA_CU; ++u) {
                const float2* src = gtile + (size_t)cv[(size_t)(1 + c + u) * cplane] + (size_t)st0 * step_stride;
#pragma unroll
                for (int i = 0; i < TA_STEPS; ++i) v[u][i] = src[(size_t)i * step_stride];
            }
#pragma unroll
            for (int u = 0; u < TA_CU; ++u)
#pragma unroll
                for (int i = 0; i < TA_STEPS; ++i) { acc[i].x += v[u][i].x; acc[i].y += v[u][i].y; }
        }
        for (; c < cnt; ++c) {
            const float2* src = gtile + (size_t)cv[(size_t)(1 + c) * cplane] + (size_t)st0 * step_stride;
            float2 v[TA_STEPS];
#pragma unroll
            for (int i = 0; i < TA_STEPS; ++i) v[i] = src[(size_t)i * step_stride];
#pragma unroll
            for (int i = 0; i < TA_STEPS; ++i) { acc[i].x += v[i].x; acc[i].y += v[i].y; }
        }
    } else if (nst == 1) {
        // one step left (every thin object: 2-D ptychography, sub-tiles of holograms): the loop over the covering tiles is all
        // there is -- four list entries and their four values in flight at a time, added in list order (same bits as one by one)
        int c = 0;
        for (; c + 4 <= cnt; c += 4) {
            unsigned e[4];
            float2 v[4];
#pragma unroll
            for (int u = 0; u < 4; ++u) e[u] = cv[(size_t)(1 + c + u) * cplane];
#pragma unroll
            for (int u = 0; u < 4; ++u) v[u] = gtile[(size_t)e[u] + (size_t)st0 * step_stride];
#pragma unroll
            for (int u = 0; u < 4; ++u) { acc[0].x += v[u].x; acc[0].y += v[u].y; }
        }
        for (; c < cnt; ++c) {
            const float2 v = gtile[(size_t)cv[(size_t)(1 + c) * cplane] + (size_t)st0 * step_stride];
            acc[0].x += v.x; acc[0].y += v.y;
        }
    } else {
        for (int c = 0; c < cnt; ++c) {
            const float2* src = gtile + (size_t)cv[(size_t)(1 + c) * cplane] + (size_t)st0 * step_stride;
#pragma unroll
            for (int i = 0; i < TA_STEPS; ++i)
                if (i < nst) { const float2 v = src[(size_t)i * step_stride]; acc[i].x += v.x; acc[i].y += v.y; }
        }
    }
#pragma unroll
    for (int i = 0; i < TA_STEPS; ++i) {
        if (i < nst) {
            const int st = st0 + i;
            const int s_lo = st * g.binning, s_hi = min(s_lo + g.binning, g.Z);
            for (int sl = s_lo; sl < s_hi; ++sl) {
                float2 v = acc[i];
                if (add) { const float2 o = out[(size_t)sl * slice_stride]; v.x += o.x; v.y += o.y; }
                out[(size_t)sl * slice_stride] = v;
            }
        }
    }
}

__global__ __launch_bounds__(256) void tile_accumulate_kernel(const float2* __restrict__ gtile, const unsigned* __restrict__ cover,
                                                              float2* __restrict__ grad_rot, TileGeom g) {
    // 1-D grid, XCD-aware: blocks are dealt round-robin over the 8 XCDs, and the 72-144-byte runs a block reads from a
    // tile row straddle 128-byte lines that its x / y neighbours read too.  XCD k takes the step chunks k, k + 8, ... and
    // ALL pixel blocks of each, x fastest, so that neighbours share an L2 (with blockIdx = (x, y, z) every straddled
    // line was fetched from HBM by two or three XCDs; FETCH_SIZE -12 %, time -10 % from the mapping alone).
    const int nbx = (g.Xp + 31) / 32, nby = (g.nrows + 7) / 8;
    const int idx = blockIdx.x >> 3;
    const int zc = (blockIdx.x & 7) + 8 * (idx / (nbx * nby));
    if (zc * TA_STEPS >= g.n_steps) return;
    ta_block(gtile, cover, grad_rot, g, zc, idx % (nbx * nby));
}
}  // namespace adm
using namespace adm;

extern "C" int adm_tile_grad_accumulate(adm_plan* plan, void* workspace, size_t workspace_bytes, const int32_t* pos, int batch,
                                       const int32_t* pos_host, float* grad_rot) {
    return adm_tile_grad_accumulate_part(plan, workspace, workspace_bytes, pos, batch, pos_host, grad_rot, 0, 0, 0);
}

// Geometry of the overlap-add of one (part of a) batch; shared by the cover build and the accumulate so that both see the
// same window.  Returns 0 or a negative status.
static int tile_geom(adm_plan* plan, int batch, const int32_t* pos_host, int win_y_lo, int win_y_hi, int add, TileGeom& g) {
    const adm_plan_desc& d = plan->d;
    const int N = d.probe_x;
    g.Yp = plan->Yp; g.Xp = plan->Xp; g.pad_y0 = d.pad_y0; g.pad_x0 = d.pad_x0; g.Py = d.probe_y; g.Px = d.probe_x;
    g.pixel_major = plan->generic ? 1 : 0;
    g.row_elems = (int)ms_row_elems(plan);
    g.R1 = g.R2 = g.G = g.LPW = 1; g.NT = 64;
    if (!plan->generic) { g.R1 = ms_r1_for(N); g.R2 = ms_r2_for(N); g.G = g.R1 > g.R2 ? g.R1 : g.R2; g.LPW = 64 / g.G; g.NT = ms_threads_for(N); }
    g.n_steps = plan->n_steps; g.binning = d.binning; g.Z = d.obj_z;
    int ymin = pos_host[0], ymax = pos_host[0];
    for (int b = 1; b < batch; ++b) { ymin = pos_host[2 * b] < ymin ? pos_host[2 * b] : ymin; ymax = pos_host[2 * b] > ymax ? pos_host[2 * b] : ymax; }
    g.row0 = ymin + d.pad_y0;
    g.nrows = ymax - ymin + d.probe_y;
    g.add_lo = g.add_hi = 0;
    if (add) {                      // accumulate into this part's own rows (an earlier part wrote the whole batch window)
        g.add_lo = g.row0;
        g.add_hi = g.row0 + g.nrows;
    } else if (win_y_hi > win_y_lo) {   // first part: write the whole batch window (zeros where no tile of this part reaches)
        if (win_y_lo + d.pad_y0 > g.row0 || win_y_hi + d.pad_y0 < g.row0 + g.nrows)
            return fail(ADM_ERR_INVALID, "adm_tile_grad_accumulate_part: the window must contain the part's own rows");
        g.row0 = win_y_lo + d.pad_y0;
        g.nrows = win_y_hi - win_y_lo;
    }
    if (g.row0 < 0 || g.row0 + g.nrows > g.Yp) return fail(ADM_ERR_INVALID, "adm_tile_grad_accumulate: a position lies outside the padded frame");
    const size_t per = (size_t)plan->n_steps * g.row_elems;
    if ((size_t)batch * per >= 0xFFFFFFFFull) return fail(ADM_ERR_UNSUPPORTED, "adm_tile_grad_accumulate: batch too large for 32-bit tile offsets");
    return ADM_OK;
}

// what adm_tile_cover_build has built and nobody has used yet (a workspace holds one set of lists: a new build for the same
// workspace replaces its entry)
// (the key includes a fingerprint of the positions THEMSELVES: the device position buffer is reused from minibatch to minibatch, so
// its address says nothing about its contents)
static unsigned long long pos_fingerprint(const int32_t* pos_host, int batch) {
    unsigned long long h = 1469598103934665603ull;                     // FNV-1a over the (y, x) pairs
    for (int i = 0; i < 2 * batch; ++i) { h ^= (unsigned)pos_host[i]; h *= 1099511628211ull; }
    return h;
}
static void cover_key_put(adm_plan* plan, const void* ws, const void* pos, const int32_t* pos_host, int batch, const TileGeom& g) {
    int slot = 0;
    for (int i = 0; i < 4; ++i) {
        if (plan->cover_keys[i].ws == ws) { slot = i; break; }
        if (!plan->cover_keys[i].ws) slot = i;
    }
    plan->cover_keys[slot] = {ws, pos, batch, g.row0, g.nrows, pos_fingerprint(pos_host, batch)};
}
static bool cover_key_take(adm_plan* plan, const void* ws, const void* pos, const int32_t* pos_host, int batch, const TileGeom& g) {
    for (int i = 0; i < 4; ++i) {
        adm_plan::CoverKey& k = plan->cover_keys[i];
        if (k.ws == ws) {
            const bool ok = k.pos == pos && k.batch == batch && k.row0 == g.row0 && k.nrows == g.nrows && k.fp == pos_fingerprint(pos_host, batch);
            k.ws = nullptr;
            return ok;
        }
    }
    return false;
}

static int cover_build(adm_plan* plan, void* workspace, const int32_t* pos, int batch, const TileGeom& g, int b_lo = 0, int b_hi = -1) {
    if (b_hi < 0) b_hi = batch;
    char* ws = (char*)workspace;
    const WsLayout w = ws_layout(plan, batch);
    unsigned* cover = (unsigned*)(ws + w.cover);
    int* overflow = (int*)(ws + w.overflow);
    hipStream_t st = plan->ctx->stream;
    // (a batch of at most ADM_MAXCOVER positions cannot overflow a cover list: no flag to reset, one launch less per minibatch)
    if (b_hi - b_lo > ADM_MAXCOVER) ADM_HIP(hipMemsetAsync(overflow, 0, sizeof(int), st));
    dim3 grid((g.Xp + 31) / 32, (g.nrows + 7) / 8, 1);
    hipLaunchKernelGGL(cover_build_kernel, grid, dim3(256), 0, st, (const int2*)pos, b_lo, b_hi, g, cover, overflow);
    ADM_HIP(hipGetLastError());
    return ADM_OK;
}

// grad_rot rows of g (+)= the tile gradients in the workspace, gathered through its cover lists
static int tile_accumulate(adm_plan* plan, void* workspace, int batch, const TileGeom& g, float* grad_rot) {
    char* ws = (char*)workspace;
    const WsLayout w = ws_layout(plan, batch);
    dim3 grid((g.Xp + 31) / 32, (g.nrows + 7) / 8, 1);
    const unsigned nz8 = ((plan->n_steps + TA_STEPS - 1) / TA_STEPS + 7) / 8;      // step chunks per XCD
    hipLaunchKernelGGL(tile_accumulate_kernel, dim3(8u * nz8 * grid.x * grid.y), dim3(256), 0, plan->ctx->stream,
                       (const float2*)(ws + w.gtile), (const unsigned*)(ws + w.cover), (float2*)grad_rot, g);
    ADM_HIP(hipGetLastError());
    return ADM_OK;
}

// The cover lists depend on the positions only, not on the tile gradients: building them EARLY -- on the side stream, beside the
// multislice launch -- takes a launch and its dependency gap off the chain that follows the kernel.  The plan remembers what
// was built (workspace, positions, batch, window); the next adm_tile_grad_accumulate[_part] with the same arguments skips its
// own build.  The caller orders the two (adm_ctx_join before the accumulate when the build was queued on the side stream).
extern "C" int adm_tile_cover_build(adm_plan* plan, void* workspace, size_t workspace_bytes, const int32_t* pos, int batch,
                                    const int32_t* pos_host, int win_y_lo, int win_y_hi, int add) {
    if (!plan || !workspace || !pos || !pos_host) return fail(ADM_ERR_INVALID, "adm_tile_cover_build: null argument");
    if (batch <= 0) return fail(ADM_ERR_INVALID, "adm_tile_cover_build: batch must be positive");
    if (workspace_bytes < adm_plan_workspace_bytes(plan, batch)) return fail(ADM_ERR_INVALID, "adm_tile_cover_build: workspace too small");
    TileGeom g;
    int rc = tile_geom(plan, batch, pos_host, win_y_lo, win_y_hi, add, g);
    if (rc) return rc;
    rc = cover_build(plan, workspace, pos, batch, g);
    if (rc) return rc;
    cover_key_put(plan, workspace, pos, pos_host, batch, g);
    return ADM_OK;
}

extern "C" int adm_tile_grad_accumulate_part(adm_plan* plan, void* workspace, size_t workspace_bytes, const int32_t* pos, int batch,
                                            const int32_t* pos_host, float* grad_rot, int win_y_lo, int win_y_hi, int add) {
    if (!plan || !workspace || !pos || !pos_host || !grad_rot) return fail(ADM_ERR_INVALID, "adm_tile_grad_accumulate: null argument");
    if (batch <= 0) return fail(ADM_ERR_INVALID, "adm_tile_grad_accumulate: batch must be positive");
    if (workspace_bytes < adm_plan_workspace_bytes(plan, batch)) return fail(ADM_ERR_INVALID, "adm_tile_grad_accumulate: workspace too small");
    TileGeom g;
    int rc = tile_geom(plan, batch, pos_host, win_y_lo, win_y_hi, add, g);
    if (rc) return rc;
    const bool prebuilt = cover_key_take(plan, workspace, pos, pos_host, batch, g);     // one use: the position buffer may be rewritten later
    if (!prebuilt) {
        rc = cover_build(plan, workspace, pos, batch, g);
        if (rc) return rc;
    }
    return tile_accumulate(plan, workspace, batch, g, grad_rot);
}

// A batch in which a pixel is covered by more than ADM_MAXCOVER tiles (dense 2-D scans taken as ONE minibatch,
// demos/2d_ptychography_w_probe_optimization.py: 2704 positions 5 pixels apart under a 72 x 72 probe): the overlap-add runs in
// passes over position ranges [b_lo, b_hi) of at most ADM_MAXCOVER positions each -- a range cannot overflow a list --, the first
// writing the batch's rows, the others adding to them.  Sums in position order, deterministic like the one-pass form.
extern "C" int adm_tile_grad_accumulate_range(adm_plan* plan, void* workspace, size_t workspace_bytes, const int32_t* pos, int batch,
                                             const int32_t* pos_host, float* grad_rot, int b_lo, int b_hi, int add) {
    if (!plan || !workspace || !pos || !pos_host || !grad_rot) return fail(ADM_ERR_INVALID, "adm_tile_grad_accumulate_range: null argument");
    if (batch <= 0 || b_lo < 0 || b_hi <= b_lo || b_hi > batch) return fail(ADM_ERR_INVALID, "adm_tile_grad_accumulate_range: bad range");
    if (b_hi - b_lo > ADM_MAXCOVER) return fail(ADM_ERR_INVALID, "adm_tile_grad_accumulate_range: at most 64 positions per pass");
    if (workspace_bytes < adm_plan_workspace_bytes(plan, batch)) return fail(ADM_ERR_INVALID, "adm_tile_grad_accumulate_range: workspace too small");
    TileGeom g, gb;
    int rc = tile_geom(plan, batch, pos_host, 0, 0, 0, gb);        // the window of the WHOLE batch
    if (rc) return rc;
    (void)cover_key_take(plan, workspace, pos, pos_host, batch, gb); // lists built ahead for the one-pass form are void now
    if (!add) {
        // first pass: the batch's rows start from zero, every pass then ADDS inside the rows its own positions reach (a pass over
        // the whole batch window cost the same whatever the range covered: 43 passes x 276 rows for the 2704-position demo)
        hipStream_t st0 = plan->ctx->stream;
        const size_t slice = (size_t)gb.Yp * gb.Xp;
        ADM_HIP(hipMemset2DAsync(grad_rot + 2 * (size_t)gb.row0 * gb.Xp, slice * sizeof(float2), 0, (size_t)gb.nrows * gb.Xp * sizeof(float2),
                                 (size_t)plan->d.obj_z, st0));
    }
    rc = tile_geom(plan, b_hi - b_lo, pos_host + 2 * (size_t)b_lo, 0, 0, 1, g);      // this range's own rows, accumulated
    if (rc) return rc;
    if ((size_t)batch * plan->n_steps * g.row_elems >= 0xFFFFFFFFull)
        return fail(ADM_ERR_UNSUPPORTED, "adm_tile_grad_accumulate_range: batch too large for 32-bit tile offsets");
    rc = cover_build(plan, workspace, pos, batch, g, b_lo, b_hi);
    if (rc) return rc;
    return tile_accumulate(plan, workspace, batch, g, grad_rot);
}

extern "C" int adm_tile_grad_status(adm_plan* plan, void* workspace, size_t workspace_bytes, int batch, int* overflow_host) {
    if (!plan || !workspace || !overflow_host) return fail(ADM_ERR_INVALID, "adm_tile_grad_status: null argument");
    if (batch <= 0 || workspace_bytes < adm_plan_workspace_bytes(plan, batch)) return fail(ADM_ERR_INVALID, "adm_tile_grad_status: bad workspace");
    if (batch <= ADM_MAXCOVER) {        // cannot overflow; the flag is not maintained for such batches
        *overflow_host = 0;
        return ADM_OK;
    }
    return adm_d2h(plan->ctx, overflow_host, (char*)workspace + ws_layout(plan, batch).overflow, sizeof(int));
}
