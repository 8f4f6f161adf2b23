// Rotation about axis 0 (R2): gather, adjoint (atomic, CSR gather, LDS-staged), stacked forms, the slice-transmission cache.
#include <hip/hip_runtime.h>
#include <hip/hip_fp16.h>
#include "adm_host.h"
#include "adm_ms_math.h"
#include "adm_rot_bilin.h"

namespace adm {
// --------------------------------------------------------------------------------------------
// Rotation about axis 0.  Reference: apply_rotation -> w.grid_sample (adorym/util.py:536-552,
// adorym/wrappers.py:1105-1147), torch grid_sampler bilinear / border / align_corners=False.
// One thread owns one rotated-frame (x', z') and loops over the y planes, so the coordinate
// pipeline (fp16 table -> fp64 normalise -> fp32 un-normalise -> clamp -> weights) runs once per
// thread.  A 16x16 (x', z') patch per block keeps the source footprint compact for any angle;
// writes are 128-B row segments of the slice-major [Z][Yp][Xp][2] layout.
// --------------------------------------------------------------------------------------------
// trans != nullptr: the slice transmission of every gathered voxel is stored beside it (same layout), so that the
// multislice kernel multiplies with a loaded number instead of evaluating exp / sincos per covering position and sweep.
__global__ __launch_bounds__(256) void rotate_fwd_kernel(const float2* __restrict__ obj, const uint16_t* __restrict__ coords,
                                                         float2* __restrict__ rot, float2* __restrict__ trans, float k1, float sigma,
                                                         RotGeom g, int y_lo, int y_hi, int y_chunk) {
    const int xr = blockIdx.x * 16 + (threadIdx.x & 15);
    const int zr = blockIdx.y * 16 + (threadIdx.x >> 4);
    if (xr >= g.X || zr >= g.Z) return;
    const Bilin b = make_bilin(coords, xr, zr, g.X, g.Z);
    const int ya = y_lo + blockIdx.z * y_chunk;
    const int yb = min(ya + y_chunk, y_hi);
    const size_t plane = (size_t)g.X * g.Z;
    for (int y = ya; y < yb; ++y) {
        const float2* o = obj + (size_t)y * plane;
        const float2 v00 = o[b.i00], v01 = o[b.i01], v10 = o[b.i10], v11 = o[b.i11];
        float2 r;
        r.x = v00.x * b.w00 + v01.x * b.w01 + v10.x * b.w10 + v11.x * b.w11;
        r.y = v00.y * b.w00 + v01.y * b.w01 + v10.y * b.w10 + v11.y * b.w11;
        const size_t o_rot = ((size_t)zr * g.Yp + g.pad_y0 + y) * g.Xp + g.pad_x0 + xr;
        if (rot) rot[o_rot] = r;
        if (trans) trans[o_rot] = slice_transmission(r, k1, sigma);
    }
}

// R objects stacked along y, block r (planes [r * Yb, (r + 1) * Yb) of the stacked rotated frame) gathered with ITS angle's table
// from the ONE real object (adorym_amd.AngleBatch: the 16 angles of a config-2 update): one launch instead of R launches of a
// few blocks each.  Same arithmetic per voxel as rotate_fwd_kernel.
__global__ __launch_bounds__(256) void rotate_fwd_stack_kernel(const float2* __restrict__ obj, const uint16_t* const* __restrict__ tables,
                                                               int Yb, float2* __restrict__ rot, float2* __restrict__ trans, float k1,
                                                               float sigma, RotGeom g, int y_chunk) {
    const int xr = blockIdx.x * 16 + (threadIdx.x & 15);
    const int zr = blockIdx.y * 16 + (threadIdx.x >> 4);
    if (xr >= g.X || zr >= g.Z) return;
    const int ya = blockIdx.z * y_chunk;                 // (y_chunk divides Yb: a block never straddles two angles)
    const int r = ya / Yb;
    const Bilin b = make_bilin(tables[r], xr, zr, g.X, g.Z);
    const int yb = min(ya + y_chunk, g.Y);
    const size_t plane = (size_t)g.X * g.Z;
    for (int y = ya; y < yb; ++y) {
        const float2* o = obj + (size_t)(y - r * Yb) * plane;
        const float2 v00 = o[b.i00], v01 = o[b.i01], v10 = o[b.i10], v11 = o[b.i11];
        float2 q;
        q.x = v00.x * b.w00 + v01.x * b.w01 + v10.x * b.w10 + v11.x * b.w11;
        q.y = v00.y * b.w00 + v01.y * b.w01 + v10.y * b.w10 + v11.y * b.w11;
        const size_t o_rot = ((size_t)zr * g.Yp + g.pad_y0 + y) * g.Xp + g.pad_x0 + xr;
        if (rot) rot[o_rot] = q;
        if (trans) trans[o_rot] = slice_transmission(q, k1, sigma);
    }
}

// No rotation (coords == nullptr) on a thin object -- the 2-D modes, Z = 1: the general kernels above would keep one thread in
// sixteen busy (their 16 x 16 patches span (x', z')).  One thread per voxel, z fastest like the object: the same numbers (weights
// 1, 0, 0, 0), 13-14 us -> a plain copy's time on the config-1 shape.
__global__ __launch_bounds__(256) void identity_fwd_kernel(const float2* __restrict__ obj, float2* __restrict__ rot, float2* __restrict__ trans,
                                                           float k1, float sigma, RotGeom g, int y_lo, int y_hi) {
    const size_t n = (size_t)(y_hi - y_lo) * g.X * g.Z;
    for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (size_t)gridDim.x * blockDim.x) {
        const int z = (int)(i % g.Z);
        const size_t yx = i / g.Z;
        const int x = (int)(yx % g.X), y = y_lo + (int)(yx / g.X);
        const float2 r = obj[((size_t)y * g.X + x) * g.Z + z];
        const size_t o_rot = ((size_t)z * g.Yp + g.pad_y0 + y) * g.Xp + g.pad_x0 + x;
        if (rot) rot[o_rot] = r;
        if (trans) trans[o_rot] = slice_transmission(r, k1, sigma);
    }
}
__global__ __launch_bounds__(256) void identity_adj_kernel(const float2* __restrict__ grot, float2* __restrict__ gobj, RotGeom g, int y_lo,
                                                           int y_hi) {
    const size_t n = (size_t)(y_hi - y_lo) * g.X * g.Z;
    for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (size_t)gridDim.x * blockDim.x) {
        const int z = (int)(i % g.Z);
        const size_t yx = i / g.Z;
        const int x = (int)(yx % g.X), y = y_lo + (int)(yx / g.X);
        const float2 v = grot[((size_t)z * g.Yp + g.pad_y0 + y) * g.Xp + g.pad_x0 + x];
        float2* o = gobj + ((size_t)y * g.X + x) * g.Z + z;
        float2 c = *o;
        c.x += v.x;
        c.y += v.y;
        *o = c;
    }
}

// slice transmissions of rows [row_lo, row_hi) of every slice of a rotated-frame buffer (pads included): the cache's
// initial fill (obj_rot == nullptr: vacuum, 1 + 0i) and adm_transmission_refresh
__global__ __launch_bounds__(256) void transmission_kernel(const float2* __restrict__ rot, float2* __restrict__ trans, float k1,
                                                           float sigma, int Z, int Yp, int Xp, int row_lo, int row_hi) {
    const size_t per = (size_t)(row_hi - row_lo) * Xp;
    const size_t n = per * Z;
    for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (size_t)gridDim.x * blockDim.x) {
        const size_t z = i / per, r = i - z * per;
        const size_t o = (z * Yp + row_lo) * Xp + r;
        trans[o] = rot ? slice_transmission(rot[o], k1, sigma) : make_float2(1.f, 0.f);
    }
}

__global__ __launch_bounds__(256) void rotate_adj_kernel(const float2* __restrict__ grot, const uint16_t* __restrict__ coords,
                                                         float* __restrict__ gobj, RotGeom g, int y_lo, int y_hi, int y_chunk) {
    const int xr = blockIdx.x * 16 + (threadIdx.x & 15);
    const int zr = blockIdx.y * 16 + (threadIdx.x >> 4);
    if (xr >= g.X || zr >= g.Z) return;
    const Bilin b = make_bilin(coords, xr, zr, g.X, g.Z);
    const int ya = y_lo + blockIdx.z * y_chunk;
    const int yb = min(ya + y_chunk, y_hi);
    const size_t plane = (size_t)g.X * g.Z;
    for (int y = ya; y < yb; ++y) {
        const float2 v = grot[((size_t)zr * g.Yp + g.pad_y0 + y) * g.Xp + g.pad_x0 + xr];
        float* o = gobj + 2 * (size_t)y * plane;
        if (b.w00 != 0.f) { atomicAdd(o + 2 * b.i00, v.x * b.w00); atomicAdd(o + 2 * b.i00 + 1, v.y * b.w00); }
        if (b.w01 != 0.f) { atomicAdd(o + 2 * b.i01, v.x * b.w01); atomicAdd(o + 2 * b.i01 + 1, v.y * b.w01); }
        if (b.w10 != 0.f) { atomicAdd(o + 2 * b.i10, v.x * b.w10); atomicAdd(o + 2 * b.i10 + 1, v.y * b.w10); }
        if (b.w11 != 0.f) { atomicAdd(o + 2 * b.i11, v.x * b.w11); atomicAdd(o + 2 * b.i11 + 1, v.y * b.w11); }
    }
}

// Rotation adjoint as a GATHER (deterministic, no atomics): the transpose of the bilinear sampling
// operator is prebuilt per angle as a CSR matrix over object-plane voxels (host: adorym_amd/util.py
// build_rotation_adjoint_csr, same fp32 coordinate pipeline as make_bilin).  One thread owns one object
// voxel column (x, z) -- consecutive threads are consecutive z, the fastest object axis, so the
// read-modify-write of grad_obj is coalesced -- and walks the y planes four at a time.
// A block owns a 16 x 16 patch of object-plane voxels and four y planes.  ALONG_X = false: lanes run along z (the
// fastest object axis): gobj accesses are coalesced, and so are the gathers from grad_rot when |sin(theta)| is large
// (a step in z is then a step in x').  ALONG_X = true (|cos| > |sin|): lanes run along x so that the gathered
// rotated-frame voxels are consecutive in x' (the fastest axis of [Z][Yp][Xp]); the patch is then transposed through
// LDS so that the read-modify-write of gobj is still issued along z.
template <bool ALONG_X>
__global__ __launch_bounds__(256) void rotate_adj_csr_kernel(const float2* __restrict__ grot, const int* __restrict__ ptr,
                                                             const int* __restrict__ src, const float* __restrict__ wgt,
                                                             float2* __restrict__ gobj, RotGeom g, int y_lo, int y_hi) {
    __shared__ float2 tile[4][16][17];
    const int lx = ALONG_X ? (threadIdx.x & 15) : (threadIdx.x >> 4);
    const int lz = ALONG_X ? (threadIdx.x >> 4) : (threadIdx.x & 15);
    const int x = blockIdx.x * 16 + lx, z = blockIdx.y * 16 + lz;
    const bool ok = (x < g.X) && (z < g.Z);
    const int t = ok ? x * g.Z + z : 0;
    const int beg = ok ? ptr[t] : 0, end = ok ? ptr[t + 1] : 0;
    const int y0 = y_lo + blockIdx.z * 4;
    const int ny = min(4, y_hi - y0);
    const size_t plane = (size_t)g.X * g.Z;
    float2 a[4];
#pragma unroll
    for (int i = 0; i < 4; ++i) a[i] = make_float2(0.f, 0.f);
    const size_t row = (size_t)(g.pad_y0 + y0) * g.Xp;
    if (ny == 4) {
        for (int j = beg; j < end; ++j) {
            const float w = wgt[j];
            const float2* q = grot + (size_t)src[j] + row;
            const float2 v0 = q[0], v1 = q[g.Xp], v2 = q[2 * (size_t)g.Xp], v3 = q[3 * (size_t)g.Xp];
            a[0].x += w * v0.x; a[0].y += w * v0.y;
            a[1].x += w * v1.x; a[1].y += w * v1.y;
            a[2].x += w * v2.x; a[2].y += w * v2.y;
            a[3].x += w * v3.x; a[3].y += w * v3.y;
        }
    } else {
        for (int j = beg; j < end; ++j) {
            const float w = wgt[j];
            const float2* q = grot + (size_t)src[j] + row;
#pragma unroll
            for (int i = 0; i < 4; ++i)
                if (i < ny) { const float2 v = q[(size_t)i * g.Xp]; a[i].x += w * v.x; a[i].y += w * v.y; }
        }
    }
    int wx = lx, wz = lz;
    if (ALONG_X) {
#pragma unroll
        for (int i = 0; i < 4; ++i) tile[i][lx][lz] = a[i];
        __syncthreads();
        wx = threadIdx.x >> 4; wz = threadIdx.x & 15;          // now lanes run along z
#pragma unroll
        for (int i = 0; i < 4; ++i) a[i] = tile[i][wx][wz];
    }
    const int ox = blockIdx.x * 16 + wx, oz = blockIdx.y * 16 + wz;
    if (ox < g.X && oz < g.Z) {
        float2* o = gobj + (size_t)y0 * plane + (size_t)ox * g.Z + oz;
#pragma unroll
        for (int i = 0; i < 4; ++i)
            if (i < ny) { float2 c = o[(size_t)i * plane]; c.x += a[i].x; c.y += a[i].y; o[(size_t)i * plane] = c; }
    }
}

// LDS-staged variant of the CSR rotation adjoint: the sources of a 16 x 16 patch of object-plane voxels lie in a
// (x', z') bounding box of at most ~27 x 27 rotated-frame voxels (host-computed per patch and angle).  The box rows are
// loaded contiguously along x' into LDS for four y planes, and the bilinear-transpose gather then runs out of LDS -- the
// memory access pattern no longer depends on the angle (the direct gather is 10x slower at 45 degrees than at 0).
// lsrc[j] = (z' - box.z0) * box.w + (x' - box.x0) of CSR entry j.
#define ADM_STAGE_MAX 1024          // float2 elements per plane in LDS when four planes are staged at once
// The staged kernels are bound by memory latency, not by the bytes they move: a block's work is a chain of dependent round trips
// (tables -> box -> CSR entries -> gradient), so each link issues all of its loads before it uses the first.
// Planes [0, NPL) of a box go to stage[p * pitch + rem], rem = z * bw + x inside the box: RB elements x NPL planes are loaded
// (one division per element, serving its NPL planes) before the first LDS store.  Nothing is branched around, or the compiler
// sinks the loads to their stores, one wait each: a plane at or past `nvalid` is staged as a copy of the last valid one (its
// sums are formed and never stored), and a thread past the box's end loads and stores the box's last element once more.
template <int NPL, int RB>
__device__ __forceinline__ void stage_box(float2* __restrict__ stage, const float2* __restrict__ box0, int Xp, size_t slice, int bw, int per,
                                          int pitch, int nvalid) {
    for (int r0 = threadIdx.x; r0 < per; r0 += 256 * RB) {
        float2 v[RB][NPL];
#pragma unroll
        for (int b = 0; b < RB; ++b) {
            const int rem = min(r0 + 256 * b, per - 1);
            const int zz = rem / bw, xx = rem - zz * bw;
            const float2* q = box0 + (size_t)zz * slice + xx;
#pragma unroll
            for (int p = 0; p < NPL; ++p) v[b][p] = q[(size_t)min(p, nvalid - 1) * Xp];
        }
#pragma unroll
        for (int b = 0; b < RB; ++b) {
            const int rem = min(r0 + 256 * b, per - 1);
#pragma unroll
            for (int p = 0; p < NPL; ++p) stage[p * pitch + rem] = v[b][p];
        }
    }
}

// weights and LDS offsets of entries [j, j + 8) of a CSR row that ends at `end`: sixteen loads in flight (entries past the end repeat
// the last one and are left out by gather_row; an empty row reads entry 0)
__device__ __forceinline__ void load_row8(const float* __restrict__ wgt, const unsigned short* __restrict__ lsrc, int j, int end, float* w,
                                          int* q) {
#pragma unroll
    for (int u = 0; u < 8; ++u) {
        const int jj = max(min(j + u, end - 1), 0);
        w[u] = wgt[jj];
        q[u] = lsrc[jj];
    }
}

// a[i] = fma(w, v, a[i]) for four entries of which the first n exist, planes [0, ny) (ny is uniform).  An entry that does not exist
// leaves a[i] as it is: a zero weight in its place would turn a sum of -0 into +0.  Its LDS read is made all the same: the empty asm
// statements pin all sixteen reads ahead of the first select, where the compiler would otherwise sink each read to its own branch
// and wait there.  It reads stage[threadIdx.x], whatever that holds (on a small box LDS this block never wrote: intended, the
// select drops the value), and not the row's last offset once more: near the axes a row
// has one or two entries and a wave's offsets lie a box row apart, so every repeated read would queue on the same few LDS banks
// (0 rad, 256^3: 55 us per launch against 41 with four reads per entry that exists); consecutive lanes share no bank.
__device__ __forceinline__ void gather4(const float2* __restrict__ stage, float2* a, const float* w, const int* q, int n, int ny) {
    float2 v[4][4];
#pragma unroll
    for (int u = 0; u < 4; ++u) {
#pragma unroll
        for (int i = 0; i < 4; ++i)
            if (i < ny) v[u][i] = stage[i * ADM_STAGE_MAX + ((u < n) ? q[u] : (int)threadIdx.x)];
    }
#pragma unroll
    for (int u = 0; u < 4; ++u) {
#pragma unroll
        for (int i = 0; i < 4; ++i)
            if (i < ny) asm volatile("" ::"v"(v[u][i].x), "v"(v[u][i].y));
    }
#pragma unroll
    for (int u = 0; u < 4; ++u) {
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            if (i < ny) {
                const float ax = __builtin_fmaf(w[u], v[u][i].x, a[i].x), ay = __builtin_fmaf(w[u], v[u][i].y, a[i].y);
                a[i].x = (u < n) ? ax : a[i].x;
                a[i].y = (u < n) ? ay : a[i].y;
            }
        }
    }
}

// the bilinear-transpose gather of one voxel out of a staged interior box: every entry of its CSR row [beg, end) in CSR order, from
// zero, one fused multiply-add each.  w, q: load_row8 of (beg, end), issued by the caller ahead of the staging so that a row of up
// to eight entries (all but the rim's) costs no round trip of its own
__device__ __forceinline__ void gather_row(const float2* __restrict__ stage, const float* __restrict__ wgt,
                                           const unsigned short* __restrict__ lsrc, int beg, int end, float* w, int* q, float2* a, int ny) {
    int j = beg;
    while (j < end) {
        gather4(stage, a, w, q, end - j, ny);
        if (j + 4 < end) gather4(stage, a, w + 4, q + 4, end - j - 4, ny);
        j += 8;
        if (j < end) load_row8(wgt, lsrc, j, end, w, q);
    }
}

// weights and LDS offsets of entries [j, j + 4) of a rim voxel's CSR row that ends at `end`; an entry past the end repeats the last
// one (an empty row reads entry 0).  No branch and no select here: either would be where the compiler waits for the load
__device__ __forceinline__ void rim_next4(const float* __restrict__ wgt, const unsigned short* __restrict__ lsrc, int j, int end, float* w,
                                          int* q) {
#pragma unroll
    for (int u = 0; u < 4; ++u) {
        const int jj = max(min(j + u, end - 1), 0);
        w[u] = wgt[jj];
        q[u] = lsrc[jj];
    }
}

// The staged adjoint's blocks are a 1-D grid walked in dispatch order, and a rim patch's block is a chain several times as long as an interior
// one's: the launch ends one such chain after the last rim block STARTS.  Rim patches are border patches of the nx x nz patch grid
// (clamping folds the frame's corner onto the object's edge), so the border ring goes first: slots [0, ring) are the ring, the
// rest the inside, row by row.  A pure function of the patch grid: nothing per angle, nothing stored.
__host__ __device__ inline int patch_ring_size(int nx, int nz) { return (nx > 2 && nz > 2) ? 2 * nx + 2 * (nz - 2) : nx * nz; }
__host__ __device__ inline void ring_patch(int i, int nx, int nz, int& px, int& pz) {      // slot i < ring -> (px, pz)
    if (nx <= 2 || nz <= 2) {                                    // all border
        pz = i / nx;
        px = i - pz * nx;
    } else if (i < 2 * nx) {                                     // rows z = 0 and z = nz - 1
        pz = (i < nx) ? 0 : nz - 1;
        px = (i < nx) ? i : i - nx;
    } else {                                                     // the two columns between them
        pz = 1 + ((i - 2 * nx) >> 1);
        px = ((i - 2 * nx) & 1) ? nx - 1 : 0;
    }
}
__host__ __device__ inline int patch_of_slot(int i, int nx, int nz) {      // -> pz * nx + px
    const int ring = patch_ring_size(nx, nz);
    int px, pz;
    if (i < ring) {
        ring_patch(i, nx, nz, px, pz);
    } else {
        pz = 1 + (i - ring) / (nx - 2);
        px = 1 + (i - ring) % (nx - 2);
    }
    return pz * nx + px;
}

// Grid (1-D): every ring patch has ADM_RING_SPLIT blocks per group of four planes, every other patch one.  Ring blocks first --
// plane group slowest, then the part, then the ring slot -- then the inside.  What a ring block does is known once its box is read
// (the angle's table): part h of a rim patch takes its share of the group's planes, so that no block chains more than that share
// of the patch's passes; any other ring patch does all four planes in part 0, and its other parts return at once.  (A rim box on
// a patch that is not on the ring would be walked by its one block, pass after pass.)
#ifndef ADM_RING_SPLIT
#define ADM_RING_SPLIT 2
#endif
static_assert(ADM_RING_SPLIT == 1 || ADM_RING_SPLIT == 2 || ADM_RING_SPLIT == 4, "a ring patch's blocks share a group of four planes");
__global__ __launch_bounds__(256) void rotate_adj_staged_kernel(const float2* __restrict__ grot, const int* __restrict__ ptr,
                                                                const int* __restrict__ src, const unsigned short* __restrict__ lsrc,
                                                                const float* __restrict__ wgt,
                                                                const int4* __restrict__ boxes, float2* __restrict__ gobj, RotGeom g,
                                                                int y_lo, int y_hi) {
    __shared__ float2 stage[4 * ADM_STAGE_MAX];
    const int nx = (g.X + 15) >> 4, nz = (g.Z + 15) >> 4, ngrp = (y_hi - y_lo + 3) >> 2;
    const int nring = patch_ring_size(nx, nz);
    int bi = blockIdx.x, slot, half = 0;
    const bool ring = bi < ADM_RING_SPLIT * nring * ngrp;
    if (ring) {
        slot = bi % nring;
        bi /= nring;
        half = bi % ADM_RING_SPLIT;
        bi /= ADM_RING_SPLIT;
    } else {
        bi -= ADM_RING_SPLIT * nring * ngrp;
        const int nin = nx * nz - nring;
        slot = nring + bi % nin;
        bi /= nin;
    }
    const int patch = patch_of_slot(slot, nx, nz);
    const int pz = patch / nx, px = patch - pz * nx;
    const int4 box = boxes[patch];      // (x0, z0, w, h)
    const int y0 = y_lo + bi * 4;
    const int ny = min(4, y_hi - y0);
    const int bw = box.z, bh = box.w, per = bw * bh;
    const size_t slice = (size_t)g.Yp * g.Xp;
    const size_t plane = (size_t)g.X * g.Z;
    const int lx = threadIdx.x >> 4, lz = threadIdx.x & 15;          // lanes along z, the fastest object axis
    const int x = px * 16 + lx, z = pz * 16 + lz;
    const bool ok = (x < g.X) && (z < g.Z);
    const int t = ok ? x * g.Z + z : 0;
    const int beg = ok ? ptr[t] : 0, end = ok ? ptr[t + 1] : 0;
    float2* o = gobj + (size_t)y0 * plane + (size_t)x * g.Z + z;
    // planes [pa, pb) of the group are this block's if the patch is a rim patch
    const bool rim = per > ADM_STAGE_MAX;
    const int pa = half * (4 / ADM_RING_SPLIT), pb = ring ? min(ny, pa + 4 / ADM_RING_SPLIT) : ny;
    if (half && (!rim || pa >= ny)) return;
    if (bw == 0) {
        // no usable box (only for objects much larger than 256^3): gather from global memory
        if (!ok) return;
        const size_t row = (size_t)(g.pad_y0 + y0) * g.Xp;
        float2 a[4];
#pragma unroll
        for (int i = 0; i < 4; ++i) a[i] = make_float2(0.f, 0.f);
        for (int j = beg; j < end; ++j) {
            const float w = wgt[j];
            const float2* q = grot + (size_t)src[j] + row;
#pragma unroll
            for (int i = 0; i < 4; ++i)
                if (i < ny) { const float2 v = q[(size_t)i * g.Xp]; a[i].x += w * v.x; a[i].y += w * v.y; }
        }
#pragma unroll
        for (int i = 0; i < 4; ++i)
            if (i < ny) { float2 c = o[(size_t)i * plane]; c.x += a[i].x; c.y += a[i].y; o[(size_t)i * plane] = c; }
        return;
    }
    const float2* oc = gobj + (size_t)y0 * plane + t;
    const float2* box0 = grot + (size_t)box.y * slice + (size_t)(g.pad_y0 + y0) * g.Xp + g.pad_x0 + box.x;
    if (per <= ADM_STAGE_MAX) {
        // interior patch: the boxes of four y planes fit at once.  The four read-modify-write targets and the first eight entries
        // of the voxel's CSR row travel together with the box: nothing below waits for a load that could have been issued here (a
        // thread outside the object, or a plane past ny, reads a valid address and drops it)
        float2 c[4];
#pragma unroll
        for (int i = 0; i < 4; ++i) c[i] = oc[(size_t)min(i, ny - 1) * plane];
        float w[8];
        int q[8];
        load_row8(wgt, lsrc, beg, end, w, q);
        stage_box<4, 2>(stage, box0, g.Xp, slice, bw, per, ADM_STAGE_MAX, ny);
        __syncthreads();
        if (!ok) return;
        float2 a[4];
#pragma unroll
        for (int i = 0; i < 4; ++i) a[i] = make_float2(0.f, 0.f);
        gather_row(stage, wgt, lsrc, beg, end, w, q, a, 4);
#pragma unroll
        for (int i = 0; i < 4; ++i)
            if (i < ny) { c[i].x += a[i].x; c[i].y += a[i].y; o[(size_t)i * plane] = c[i]; }
        return;
    }
    // rim patch (border clamping folds a corner of the rotated frame onto it: box of up to 4096 voxels): one or two planes
    // per pass over the CSR entries, whatever fits the 32 KB stage.  The row (up to ~115 entries) is walked through a ring of
    // sixteen entries: the first sixteen travel with the box, and every four slots are reloaded with the entries sixteen further on
    // as soon as their LDS gathers are issued, ahead of their multiply-adds -- sixteen entries' loads stay in flight behind the
    // gathers, where a batch of eight used to be loaded, waited for and used before the next was asked for.  The pass's two
    // read-modify-write targets are asked for behind the barrier and arrive during the walk.
    const int npp = (2 * per <= 4 * ADM_STAGE_MAX) ? 2 : 1;
    for (int p0 = pa; p0 < pb; p0 += npp) {
        float w[16];
        int q[16];
        int b0 = beg;       // opaque per pass: hoisted out of this loop, the first sixteen entries would hold 32 registers across the walk
        asm volatile("" : "+v"(b0));
#pragma unroll
        for (int u0 = 0; u0 < 16; u0 += 4) rim_next4(wgt, lsrc, b0 + u0, end, w + u0, q + u0);
        if (npp == 2) stage_box<2, 4>(stage, box0 + (size_t)p0 * g.Xp, g.Xp, slice, bw, per, per, pb - p0);
        else stage_box<1, 8>(stage, box0 + (size_t)p0 * g.Xp, g.Xp, slice, bw, per, per, 1);
        __syncthreads();
        if (ok) {
            const bool two = (npp == 2) && (p0 + 1 < pb);
            float2 c0 = oc[(size_t)p0 * plane], c1 = oc[(size_t)(two ? p0 + 1 : p0) * plane];
            float2 acc0 = make_float2(0.f, 0.f), acc1 = make_float2(0.f, 0.f);
            const int second = (npp == 2) ? per : 0;
            for (int j = beg; j < end; j += 16) {
#pragma unroll
                for (int u0 = 0; u0 < 16; u0 += 4) {
                    float2 v0[4], v1[4];
                    float wc[4];
#pragma unroll
                    for (int u = 0; u < 4; ++u) {
                        v0[u] = stage[q[u0 + u]];
                        v1[u] = stage[q[u0 + u] + second];
                        wc[u] = (j + u0 + u < end) ? w[u0 + u] : 0.f;      // past the row's end: a zero weight on its last entry
                    }
                    rim_next4(wgt, lsrc, j + 16 + u0, end, w + u0, q + u0);
#pragma unroll
                    for (int u = 0; u < 4; ++u) {
                        acc0.x += wc[u] * v0[u].x; acc0.y += wc[u] * v0[u].y;
                        acc1.x += wc[u] * v1[u].x; acc1.y += wc[u] * v1[u].y;
                    }
                    __builtin_amdgcn_sched_barrier(0);      // one group of four at a time: merged, the groups' gathers want 200 registers
                }
            }
            c0.x += acc0.x; c0.y += acc0.y;
            o[(size_t)p0 * plane] = c0;
            if (two) { c1.x += acc1.x; c1.y += acc1.y; o[(size_t)(p0 + 1) * plane] = c1; }
        }
        __syncthreads();
    }
}

// The staged adjoint for R objects stacked along y (adorym_amd.AngleBatch): block r of the stacked gradient image is back-rotated with
// ITS angle's CSR and all R contributions are added, r ascending, to the ONE real gradient -- c = g; c += a_0; c += a_1; ... ; g = c:
// the additions R sequential launches of rotate_adj_staged_kernel would make, in the same order, in one launch (16 launches of
// 6 - 12 us each per config-2 update).  Same three cases per (patch, angle) as above, written without early exits so that every
// thread reaches the barriers that separate one angle's use of the LDS stage from the next.
struct AdjTables { const int* ptr; const int* src; const unsigned short* lsrc; const float* wgt; const int4* boxes; };
// `part` != nullptr: the angles run in PARALLEL -- blockIdx.z = (angle, plane group), the block leaves its angle's term a_r in
// part[r][y][x][z] and stack_sum_kernel forms c = g; c += a_0; c += a_1; ... afterwards (the same additions in the same order: same
// bits); a block walking all R angles one after the other is a chain of R stage-fill / barrier / gather rounds (86 us for 16
// angles of a 64^3 object against 20 + 8).
__global__ __launch_bounds__(256) void rotate_adj_staged_stack_kernel(const float2* __restrict__ grot, const AdjTables* __restrict__ tabs,
                                                                      int R, int Yb, float2* __restrict__ gobj, RotGeom g, int npl,
                                                                      float2* __restrict__ part) {
    __shared__ float2 stage[4 * ADM_STAGE_MAX];
    const int nzg = (Yb + npl - 1) / npl;                // plane groups
    const int zg = part ? (int)blockIdx.z % nzg : (int)blockIdx.z;
    const int r_lo = part ? (int)blockIdx.z / nzg : 0, r_hi = part ? r_lo + 1 : R;
    const int y0 = zg * npl;                             // first plane (of the REAL object, Yb planes) of this block: npl = 1, 2 or 4 planes
    const int ny = min(npl, Yb - y0);
    const size_t slice = (size_t)g.Yp * g.Xp;
    const size_t plane = (size_t)g.X * g.Z;
    const int lx = threadIdx.x >> 4, lz = threadIdx.x & 15;
    const int x = blockIdx.x * 16 + lx, z = blockIdx.y * 16 + lz;
    const bool ok = (x < g.X) && (z < g.Z);
    const int t = ok ? x * g.Z + z : 0;
    float2* o = (part ? part + (size_t)r_lo * Yb * plane : gobj) + (size_t)y0 * plane + (size_t)x * g.Z + z;
    float2 c[4];
#pragma unroll
    for (int i = 0; i < 4; ++i) c[i] = make_float2(0.f, 0.f);
    if (!part) {
        // all four loads in flight at once: a thread outside the object, or a plane past ny, reads a valid address and drops it
        const float2* oc = gobj + (size_t)y0 * plane + t;
        float2 l[4];
#pragma unroll
        for (int i = 0; i < 4; ++i) l[i] = oc[(size_t)min(i, ny - 1) * plane];
#pragma unroll
        for (int i = 0; i < 4; ++i)
            if (ok && i < ny) c[i] = l[i];
    }
    for (int r = r_lo; r < r_hi; ++r) {
        const AdjTables T = tabs[r];
        const int4 box = T.boxes[blockIdx.y * gridDim.x + blockIdx.x];      // (x0, z0, w, h)
        const int ys = r * Yb + y0;                     // the same planes in block r of the stacked image
        const int bw = box.z, bh = box.w, per = bw * bh;
        const int beg = ok ? T.ptr[t] : 0, end = ok ? T.ptr[t + 1] : 0;
        const float2* box0 = grot + (size_t)box.y * slice + (size_t)(g.pad_y0 + ys) * g.Xp + g.pad_x0 + box.x;
        if (bw == 0) {
            const size_t row = (size_t)(g.pad_y0 + ys) * g.Xp;
            float2 a[4];
#pragma unroll
            for (int i = 0; i < 4; ++i) a[i] = make_float2(0.f, 0.f);
            for (int j = beg; j < end; ++j) {
                const float w = T.wgt[j];
                const float2* q = grot + (size_t)T.src[j] + row;
#pragma unroll
                for (int i = 0; i < 4; ++i)
                    if (i < ny) { const float2 v = q[(size_t)i * g.Xp]; a[i].x += w * v.x; a[i].y += w * v.y; }
            }
#pragma unroll
            for (int i = 0; i < 4; ++i) { c[i].x += a[i].x; c[i].y += a[i].y; }
        } else if (per <= ADM_STAGE_MAX) {
            float w[8];
            int q[8];
            load_row8(T.wgt, T.lsrc, beg, end, w, q);                       // ahead of the staging: see rotate_adj_staged_kernel
            if (npl == 4) stage_box<4, 2>(stage, box0, g.Xp, slice, bw, per, ADM_STAGE_MAX, ny);
            else if (npl == 2) stage_box<2, 4>(stage, box0, g.Xp, slice, bw, per, ADM_STAGE_MAX, ny);
            else stage_box<1, 8>(stage, box0, g.Xp, slice, bw, per, ADM_STAGE_MAX, 1);
            __syncthreads();
            float2 a[4];
#pragma unroll
            for (int i = 0; i < 4; ++i) a[i] = make_float2(0.f, 0.f);
            gather_row(stage, T.wgt, T.lsrc, beg, end, w, q, a, ny);
#pragma unroll
            for (int i = 0; i < 4; ++i) { c[i].x += a[i].x; c[i].y += a[i].y; }
        } else {
            const int npp = (npl >= 2 && 2 * per <= 4 * ADM_STAGE_MAX) ? 2 : 1;
            for (int p0 = 0; p0 < ny; p0 += npp) {
                if (npp == 2) stage_box<2, 4>(stage, box0 + (size_t)p0 * g.Xp, g.Xp, slice, bw, per, per, ny - p0);
                else stage_box<1, 8>(stage, box0 + (size_t)p0 * g.Xp, g.Xp, slice, bw, per, per, 1);
                __syncthreads();
                float2 acc0 = make_float2(0.f, 0.f), acc1 = make_float2(0.f, 0.f);
                const int second = (npp == 2) ? per : 0;
                for (int j = beg; j < end; j += 8) {
                    float w[8];
                    int q[8];
#pragma unroll
                    for (int u = 0; u < 8; ++u) {
                        const int jj = min(j + u, end - 1);
                        w[u] = (j + u < end) ? T.wgt[jj] : 0.f;
                        q[u] = T.lsrc[jj];
                    }
#pragma unroll
                    for (int u = 0; u < 8; ++u) {
                        const float2 v0 = stage[q[u]];
                        const float2 v1 = stage[q[u] + second];
                        acc0.x += w[u] * v0.x; acc0.y += w[u] * v0.y;
                        acc1.x += w[u] * v1.x; acc1.y += w[u] * v1.y;
                    }
                }
                // (p0 is uniform: the static indices below keep c[] in registers)
#pragma unroll
                for (int i = 0; i < 4; ++i) {
                    if (i == p0) { c[i].x += acc0.x; c[i].y += acc0.y; }
                    if (npp == 2 && i == p0 + 1) { c[i].x += acc1.x; c[i].y += acc1.y; }
                }
                __syncthreads();
            }
        }
        __syncthreads();                                 // the next angle refills the stage
    }
    if (ok) {
#pragma unroll
        for (int i = 0; i < 4; ++i)
            if (i < ny) o[(size_t)i * plane] = c[i];
    }
}
}  // namespace adm
using namespace adm;

extern "C" int adm_rotate_fwd(adm_plan* plan, const float* obj, const uint16_t* coords, float* obj_rot, int y_lo, int y_hi) {
    if (!plan || !obj || !obj_rot) return fail(ADM_ERR_INVALID, "adm_rotate_fwd: null argument");
    const adm_plan_desc& d = plan->d;
    if (y_lo < 0 || y_hi > d.obj_y || y_lo > y_hi) return fail(ADM_ERR_INVALID, "adm_rotate_fwd: bad y range");
    if (y_lo == y_hi) return ADM_OK;
    RotGeom g{d.obj_y, d.obj_x, d.obj_z, plan->Yp, plan->Xp, d.pad_y0, d.pad_x0};
    // y planes per block: 32 (the (x', z') sampling weights are decoded once per block and reused) -- unless that leaves the chip
    // empty: a 64^3 object has 16 patches x 2 chunks = 32 blocks that each walk 32 planes one dependent gather after the other
    // (17 us per launch, 16 launches per config-2 update); then fewer planes per block, down to one
    int y_chunk = 32;
    const int n_patch = ((d.obj_x + 15) / 16) * ((d.obj_z + 15) / 16);
    while (y_chunk > 1 && n_patch * ((y_hi - y_lo + y_chunk - 1) / y_chunk) < 512) y_chunk >>= 1;
    dim3 grid((d.obj_x + 15) / 16, (d.obj_z + 15) / 16, (y_hi - y_lo + y_chunk - 1) / y_chunk);
    // cache mode 2: only the transmissions are written (half the stores); obj_rot then merely names the image the cache holds
    float2* rot_out = (plan->trans_dev && plan->trans_only) ? (float2*)nullptr : (float2*)obj_rot;
    if (!coords && d.obj_z < 16)
        hipLaunchKernelGGL(identity_fwd_kernel, dim3(stream_grid((size_t)(y_hi - y_lo) * d.obj_x * d.obj_z)), dim3(256), 0, plan->ctx->stream,
                           (const float2*)obj, rot_out, plan->trans_dev, d.k1, (float)d.sign_convention, g, y_lo, y_hi);
    else
        hipLaunchKernelGGL(rotate_fwd_kernel, grid, dim3(256), 0, plan->ctx->stream, (const float2*)obj, coords, rot_out, plan->trans_dev,
                           d.k1, (float)d.sign_convention, g, y_lo, y_hi, y_chunk);
    ADM_HIP(hipGetLastError());
    if (plan->trans_dev) plan->trans_src = obj_rot;
    return ADM_OK;
}

extern "C" int adm_rotate_fwd_stack(adm_plan* plan, const float* obj, const void* tables_dev, int n_tables, float* obj_rot) {
    if (!plan || !obj || !tables_dev || !obj_rot) return fail(ADM_ERR_INVALID, "adm_rotate_fwd_stack: null argument");
    const adm_plan_desc& d = plan->d;
    if (n_tables < 1 || d.obj_y % n_tables) return fail(ADM_ERR_INVALID, "adm_rotate_fwd_stack: the plan's y extent is not n_tables blocks");
    const int Yb = d.obj_y / n_tables;
    RotGeom g{d.obj_y, d.obj_x, d.obj_z, plan->Yp, plan->Xp, d.pad_y0, d.pad_x0};
    int y_chunk = 32;
    while (y_chunk > 1 && Yb % y_chunk) y_chunk >>= 1;
    const int n_patch = ((d.obj_x + 15) / 16) * ((d.obj_z + 15) / 16);
    while (y_chunk > 1 && n_patch * (d.obj_y / y_chunk) < 512) y_chunk >>= 1;
    dim3 grid((d.obj_x + 15) / 16, (d.obj_z + 15) / 16, d.obj_y / y_chunk);
    float2* rot_out = (plan->trans_dev && plan->trans_only) ? (float2*)nullptr : (float2*)obj_rot;
    hipLaunchKernelGGL(rotate_fwd_stack_kernel, grid, dim3(256), 0, plan->ctx->stream, (const float2*)obj,
                       (const uint16_t* const*)tables_dev, Yb, rot_out, plan->trans_dev, d.k1, (float)d.sign_convention, g, y_chunk);
    ADM_HIP(hipGetLastError());
    if (plan->trans_dev) plan->trans_src = obj_rot;
    return ADM_OK;
}

static int transmission_fill(adm_plan* plan, const float* obj_rot, int row_lo, int row_hi) {
    const adm_plan_desc& d = plan->d;
    const size_t n = (size_t)(row_hi - row_lo) * plan->Xp * d.obj_z;
    hipLaunchKernelGGL(transmission_kernel, dim3((unsigned)std::min<size_t>((n + 255) / 256, 8192)), dim3(256), 0, plan->ctx->stream,
                       (const float2*)obj_rot, plan->trans_dev, d.k1, (float)d.sign_convention, d.obj_z, plan->Yp, plan->Xp, row_lo,
                       row_hi);
    ADM_HIP(hipGetLastError());
    return ADM_OK;
}

extern "C" int adm_plan_set_transmission_cache(adm_plan* plan, int on) {
    if (!plan) return fail(ADM_ERR_INVALID, "adm_plan_set_transmission_cache: null plan");
    const adm_plan_desc& d = plan->d;
    if (!on) {
        if (plan->trans_dev) {
            ADM_HIP(hipStreamSynchronize(plan->ctx->main_stream));
            ADM_HIP(hipFree(plan->trans_dev));
        }
        plan->trans_dev = nullptr;
        plan->trans_src = nullptr;
        plan->trans_only = false;
        return ADM_OK;
    }
    if (d.unknown_type != 0 || d.binning != 1)      // (validated first: a refused call leaves the plan as it was)
        return fail(ADM_ERR_UNSUPPORTED, "adm_plan_set_transmission_cache: needs unknown_type delta_beta and binning 1");
    if (!plan->trans_dev) {
        float2* t = nullptr;
        ADM_HIP(hipMalloc((void**)&t, (size_t)d.obj_z * plan->Yp * plan->Xp * sizeof(float2)));
        plan->trans_dev = t;
        plan->trans_src = nullptr;
        const int rc = transmission_fill(plan, nullptr, 0, plan->Yp);      // vacuum everywhere: the pads keep it forever
        if (rc) {
            (void)hipFree(t);
            plan->trans_dev = nullptr;
            plan->trans_only = false;
            return rc;
        }
    }
    plan->trans_only = (on == 2);
    return ADM_OK;
}

extern "C" int adm_transmission_refresh(adm_plan* plan, const float* obj_rot, int y_lo, int y_hi) {
    if (!plan || !obj_rot) return fail(ADM_ERR_INVALID, "adm_transmission_refresh: null argument");
    if (!plan->trans_dev) return fail(ADM_ERR_INVALID, "adm_transmission_refresh: the plan has no transmission cache");
    const adm_plan_desc& d = plan->d;
    if (y_lo < 0 || y_hi > d.obj_y || y_lo > y_hi) return fail(ADM_ERR_INVALID, "adm_transmission_refresh: bad y range");
    plan->trans_src = obj_rot;
    if (y_lo == y_hi) return ADM_OK;
    return transmission_fill(plan, obj_rot, d.pad_y0 + y_lo, d.pad_y0 + y_hi);
}

extern "C" int adm_rotate_adj(adm_plan* plan, const float* grad_rot, const uint16_t* coords, float* grad_obj, int y_lo, int y_hi) {
    if (!plan || !grad_rot || !grad_obj) return fail(ADM_ERR_INVALID, "adm_rotate_adj: null argument");
    const adm_plan_desc& d = plan->d;
    if (y_lo < 0 || y_hi > d.obj_y || y_lo > y_hi) return fail(ADM_ERR_INVALID, "adm_rotate_adj: bad y range");
    if (y_lo == y_hi) return ADM_OK;
    RotGeom g{d.obj_y, d.obj_x, d.obj_z, plan->Yp, plan->Xp, d.pad_y0, d.pad_x0};
    const int y_chunk = 32;
    dim3 grid((d.obj_x + 15) / 16, (d.obj_z + 15) / 16, (y_hi - y_lo + y_chunk - 1) / y_chunk);
    if (!coords && d.obj_z < 16)
        hipLaunchKernelGGL(identity_adj_kernel, dim3(stream_grid((size_t)(y_hi - y_lo) * d.obj_x * d.obj_z)), dim3(256), 0, plan->ctx->stream,
                           (const float2*)grad_rot, (float2*)grad_obj, g, y_lo, y_hi);
    else
        hipLaunchKernelGGL(rotate_adj_kernel, grid, dim3(256), 0, plan->ctx->stream, (const float2*)grad_rot, coords, grad_obj, g, y_lo,
                           y_hi, y_chunk);
    ADM_HIP(hipGetLastError());
    return ADM_OK;
}

extern "C" int adm_rotate_adj_csr(adm_plan* plan, const float* grad_rot, const int32_t* csr_ptr, const int32_t* csr_src,
                                  const float* csr_w, float* grad_obj, int y_lo, int y_hi, int lanes_along_x) {
    if (!plan || !grad_rot || !csr_ptr || !csr_src || !csr_w || !grad_obj) return fail(ADM_ERR_INVALID, "adm_rotate_adj_csr: null argument");
    const adm_plan_desc& d = plan->d;
    if (y_lo < 0 || y_hi > d.obj_y || y_lo > y_hi) return fail(ADM_ERR_INVALID, "adm_rotate_adj_csr: bad y range");
    if (y_lo == y_hi) return ADM_OK;
    RotGeom g{d.obj_y, d.obj_x, d.obj_z, plan->Yp, plan->Xp, d.pad_y0, d.pad_x0};
    dim3 grid((d.obj_x + 15) / 16, (d.obj_z + 15) / 16, (y_hi - y_lo + 3) / 4);
    if (lanes_along_x)
        hipLaunchKernelGGL(rotate_adj_csr_kernel<true>, grid, dim3(256), 0, plan->ctx->stream, (const float2*)grad_rot, csr_ptr, csr_src,
                           csr_w, (float2*)grad_obj, g, y_lo, y_hi);
    else
        hipLaunchKernelGGL(rotate_adj_csr_kernel<false>, grid, dim3(256), 0, plan->ctx->stream, (const float2*)grad_rot, csr_ptr, csr_src,
                           csr_w, (float2*)grad_obj, g, y_lo, y_hi);
    ADM_HIP(hipGetLastError());
    return ADM_OK;
}

extern "C" int adm_rotate_adj_staged(adm_plan* plan, const float* grad_rot, const int32_t* csr_ptr, const int32_t* csr_src,
                                     const uint16_t* csr_lsrc, const float* csr_w, const int32_t* boxes, float* grad_obj, int y_lo,
                                     int y_hi) {
    if (!plan || !grad_rot || !csr_ptr || !csr_src || !csr_lsrc || !csr_w || !boxes || !grad_obj)
        return fail(ADM_ERR_INVALID, "adm_rotate_adj_staged: null argument");
    const adm_plan_desc& d = plan->d;
    if (y_lo < 0 || y_hi > d.obj_y || y_lo > y_hi) return fail(ADM_ERR_INVALID, "adm_rotate_adj_staged: bad y range");
    if (y_lo == y_hi) return ADM_OK;
    RotGeom g{d.obj_y, d.obj_x, d.obj_z, plan->Yp, plan->Xp, d.pad_y0, d.pad_x0};
    // one block per (patch, group of four planes), ADM_RING_SPLIT for the patches of the border ring: see rotate_adj_staged_kernel
    const int nx = (d.obj_x + 15) / 16, nz = (d.obj_z + 15) / 16;
    const size_t blocks = ((size_t)nx * nz + (ADM_RING_SPLIT - 1) * patch_ring_size(nx, nz)) * ((y_hi - y_lo + 3) / 4);
    if (blocks > 0x7fffffffu) return fail(ADM_ERR_UNSUPPORTED, "adm_rotate_adj_staged: more than 2^31 blocks");
    hipLaunchKernelGGL(rotate_adj_staged_kernel, dim3((unsigned)blocks), dim3(256), 0, plan->ctx->stream, (const float2*)grad_rot, csr_ptr,
                       csr_src, (const unsigned short*)csr_lsrc, csr_w, (const int4*)boxes, (float2*)grad_obj, g, y_lo, y_hi);
    ADM_HIP(hipGetLastError());
    return ADM_OK;
}

extern "C" int adm_patch_order(int nx, int nz, int32_t* order) {
    if (nx < 1 || nz < 1 || !order) return fail(ADM_ERR_INVALID, "adm_patch_order: bad argument");
    for (int i = 0; i < nx * nz; ++i) order[i] = patch_of_slot(i, nx, nz);
    return patch_ring_size(nx, nz);
}

#ifndef ADM_STACK_MIN_BLOCKS
#define ADM_STACK_MIN_BLOCKS 2048
#endif
// g[i] = ((g[i] + a_0[i]) + a_1[i]) + ... : the terms of the R angles in angle order
__global__ __launch_bounds__(256) void stack_sum_kernel(const float2* __restrict__ part, int R, size_t n, float2* __restrict__ gobj) {
    const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    float2 c = gobj[i];
    for (int r = 0; r < R; ++r) {
        const float2 a = part[(size_t)r * n + i];
        c.x += a.x;
        c.y += a.y;
    }
    gobj[i] = c;
}

extern "C" int adm_rotate_adj_staged_stack(adm_plan* plan, const float* grad_rot, const void* tables_dev, int n_tables, float* grad_obj,
                                           float* scratch, size_t scratch_bytes) {
    if (!plan || !grad_rot || !tables_dev || !grad_obj) return fail(ADM_ERR_INVALID, "adm_rotate_adj_staged_stack: null argument");
    const adm_plan_desc& d = plan->d;
    if (n_tables < 1 || d.obj_y % n_tables) return fail(ADM_ERR_INVALID, "adm_rotate_adj_staged_stack: the plan's y extent is not n_tables blocks");
    const int Yb = d.obj_y / n_tables;
    RotGeom g{d.obj_y, d.obj_x, d.obj_z, plan->Yp, plan->Xp, d.pad_y0, d.pad_x0};
    // planes per block: four (one pass over a patch's CSR entries serves four planes) unless that leaves the chip short of blocks --
    // every block walks the n_tables angles one after the other, so a 64^3 object wants all 1024 (patch, plane) pairs in flight
    int npl = 4;
    const int n_patch = ((d.obj_x + 15) / 16) * ((d.obj_z + 15) / 16);
    while (npl > 1 && n_patch * ((Yb + npl - 1) / npl) < 1024) npl >>= 1;
    const size_t n_real = (size_t)Yb * d.obj_x * d.obj_z;
    if (scratch) {
        // the angles side by side (scratch: n_tables copies of the real gradient's size), then their sum in angle order
        if (scratch_bytes < (size_t)n_tables * n_real * sizeof(float2))
            return fail(ADM_ERR_INVALID, "adm_rotate_adj_staged_stack: scratch smaller than n_tables x the real object");
        npl = 4;
        while (npl > 1 && (size_t)n_patch * ((Yb + npl - 1) / npl) * n_tables < (size_t)ADM_STACK_MIN_BLOCKS) npl >>= 1;
        dim3 gridp((d.obj_x + 15) / 16, (d.obj_z + 15) / 16, ((Yb + npl - 1) / npl) * n_tables);
        hipLaunchKernelGGL(rotate_adj_staged_stack_kernel, gridp, dim3(256), 0, plan->ctx->stream, (const float2*)grad_rot,
                           (const AdjTables*)tables_dev, n_tables, Yb, (float2*)grad_obj, g, npl, (float2*)scratch);
        hipLaunchKernelGGL(stack_sum_kernel, dim3((unsigned)((n_real + 255) / 256)), dim3(256), 0, plan->ctx->stream,
                           (const float2*)scratch, n_tables, n_real, (float2*)grad_obj);
        ADM_HIP(hipGetLastError());
        return ADM_OK;
    }
    dim3 grid((d.obj_x + 15) / 16, (d.obj_z + 15) / 16, (Yb + npl - 1) / npl);
    hipLaunchKernelGGL(rotate_adj_staged_stack_kernel, grid, dim3(256), 0, plan->ctx->stream, (const float2*)grad_rot,
                       (const AdjTables*)tables_dev, n_tables, Yb, (float2*)grad_obj, g, npl, (float2*)nullptr);
    ADM_HIP(hipGetLastError());
    return ADM_OK;
}
