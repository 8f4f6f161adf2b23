// Rotation about axis 0 fused with the sum along the beam, and the transpose of the pair: what adm_rotate_fwd + adm_project_z and
// adm_project_z_adj + adm_rotate_adj_csr compute, without the rotated-frame buffer [Z][Yp][Xp][2] between them.
//
//   adm_rotate_project_fwd  proj[y][x']    = round_fp32(sum over z' of r(y, x', z')), r the sample adm_rotate_fwd stores, the sum in double
//   adm_rotate_project_adj  grad_obj[y][t] += sum over the CSR row of t of w_j * grad_proj[y][x'_j]
//
// proj / grad_proj are the plan's one-slice padded image [1][Yp][Xp][2] of adm_project_z.
#include "adm_host.h"
#include "adm_rot_bilin.h"

namespace adm {
#define RPJ_TILE 16            // a workgroup of the gather is RPJ_TILE columns x' x RPJ_TILE lanes along z'
#define RPJ_PLANES 4           // y planes a workgroup of the gather serves with one evaluation of the weights
#define RPJ_MIN_BLOCKS 512     // below it (a minibatch's few rows) a workgroup takes one plane
#define RPJ_ADJ_PLANES 4       // y planes a workgroup of the back-projection serves with one walk over a CSR row
#define RPJ_ADJ_VOX 4          // object voxels per thread of the back-projection
#define RPJ_ADJ_LDS_MAX 65536  // bytes of LDS the staged rows of grad_proj may take

// Which axis of the rotated frame runs along the object's fastest axis: a step in z' moves the source by (d x, d z) = (-sin, cos)
// voxels.  Read from two neighbouring entries at the middle of the table; no table (coords = NULL) or a single slice: z'.
__device__ __forceinline__ bool rpj_lanes_along_z(const uint16_t* coords, int X, int Z) {
    if (coords == nullptr || Z < 2) return true;
    const __half* c = reinterpret_cast<const __half*>(coords) + 2 * ((size_t)(X / 2) * Z + (Z - 1) / 2);
    const float dx = __half2float(c[2]) - __half2float(c[0]), dz = __half2float(c[3]) - __half2float(c[1]);
    return fabsf(dz) >= fabsf(dx);
}

// Workgroup = RPJ_TILE columns x' of PL planes.  Thread (c, l) adds the samples z' = l, l + RPJ_TILE, l + 2 RPJ_TILE, ... of column c in
// that order, in double; the RPJ_TILE partial sums of a column meet in LDS and are added l = 0, 1, ... and rounded once.  No
// atomics.  Where the lanes run -- 16 consecutive z' of one column (|cos| >= |sin|: consecutive in obj[y]) or 16 consecutive x'
// of one z' (consecutive in obj[y] when |sin| is the larger) -- only transposes (c, l) inside the workgroup: the sums, their order
// and so the bits are the same either way, and the same for PL = 1 and RPJ_PLANES.
template <int PL>
__global__ __launch_bounds__(RPJ_TILE * RPJ_TILE) void rotate_project_fwd_kernel(const float2* __restrict__ obj,
                                                                                 const uint16_t* __restrict__ coords,
                                                                                 float2* __restrict__ proj, RotGeom g, int y_lo, int y_hi) {
    __shared__ double part[PL][RPJ_TILE][RPJ_TILE][2];        // [plane][l][c][channel]
    const bool along_z = rpj_lanes_along_z(coords, g.X, g.Z);
    const int c = along_z ? (threadIdx.x >> 4) : (threadIdx.x & 15);
    const int l = along_z ? (threadIdx.x & 15) : (threadIdx.x >> 4);
    const int xr = blockIdx.x * RPJ_TILE + c;
    const int y0 = y_lo + blockIdx.y * PL;
    const int ny = min(PL, y_hi - y0);
    const size_t plane = (size_t)g.X * g.Z;
    double acc[PL][2];
#pragma unroll
    for (int i = 0; i < PL; ++i) acc[i][0] = acc[i][1] = 0.0;
    if (xr < g.X) {
        for (int zr = l; zr < g.Z; zr += RPJ_TILE) {
            const Bilin b = make_bilin(coords, xr, zr, g.X, g.Z);
            float2 v[PL][4];
#pragma unroll
            for (int i = 0; i < PL; ++i) {      // a plane past ny reads the last valid one and is dropped below
                const float2* o = obj + (size_t)(y0 + min(i, ny - 1)) * plane;
                v[i][0] = o[b.i00]; v[i][1] = o[b.i01]; v[i][2] = o[b.i10]; v[i][3] = o[b.i11];
            }
#pragma unroll
            for (int i = 0; i < PL; ++i) {
                const float2 r = bilin_sample(b, v[i][0], v[i][1], v[i][2], v[i][3]);
                acc[i][0] += (double)r.x;
                acc[i][1] += (double)r.y;
            }
        }
    }
#pragma unroll
    for (int i = 0; i < PL; ++i) {
        part[i][l][c][0] = acc[i][0];
        part[i][l][c][1] = acc[i][1];
    }
    __syncthreads();
    // thread k < PL * RPJ_TILE: column k % RPJ_TILE of plane k / RPJ_TILE, both channels
    const int k = threadIdx.x;
    const int oi = k / RPJ_TILE, oc = k % RPJ_TILE, ox = blockIdx.x * RPJ_TILE + oc;
    if (oi < ny && ox < g.X) {
        double s0 = part[oi][0][oc][0], s1 = part[oi][0][oc][1];
#pragma unroll
        for (int u = 1; u < RPJ_TILE; ++u) {
            s0 += part[oi][u][oc][0];
            s1 += part[oi][u][oc][1];
        }
        proj[(size_t)(g.pad_y0 + y0 + oi) * g.Xp + g.pad_x0 + ox] = make_float2((float)s0, (float)s1);
    }
    // the x pads of the rows: +0, as the sum over a rotated frame's pads would leave them (the first workgroup of the rows)
    if (blockIdx.x == 0) {
        const int npad = g.Xp - g.X;
        for (int q = threadIdx.x; q < ny * npad; q += RPJ_TILE * RPJ_TILE) {
            const int i = q / npad, p = q - i * npad;
            const int col = p < g.pad_x0 ? p : p + g.X;
            proj[(size_t)(g.pad_y0 + y0 + i) * g.Xp + col] = make_float2(0.f, 0.f);
        }
    }
}

// Workgroup = 256 threads x RPJ_ADJ_VOX object voxels t = x * Z + z (consecutive threads are consecutive t: the read-modify-write
// of grad_obj and the reads of the tables are coalesced whatever Z is) x RPJ_ADJ_PLANES planes.  The interior columns of the
// planes' rows of grad_proj are staged in LDS (X float2 each): the gather's access pattern does not depend on the angle.  A voxel's
// entries are taken in table order from zero, a[i] += w * v in float32, then grad_obj += a -- the arithmetic of
// rotate_adj_csr_kernel on the broadcast volume.  ptr == nullptr: no rotation, the row's pixel x is added to every z.
__global__ __launch_bounds__(256) void rotate_project_adj_kernel(const float2* __restrict__ gproj, const int* __restrict__ ptr,
                                                                 const int* __restrict__ src, const float* __restrict__ wgt,
                                                                 float2* __restrict__ gobj, RotGeom g, int y_lo, int y_hi) {
    extern __shared__ float2 rpj_rows[];                     // [RPJ_ADJ_PLANES][X]
    const int y0 = y_lo + blockIdx.y * RPJ_ADJ_PLANES;
    const int ny = min(RPJ_ADJ_PLANES, y_hi - y0);
    const size_t plane = (size_t)g.X * g.Z;
    const unsigned slice = (unsigned)g.Yp * (unsigned)g.Xp;
    for (int q = threadIdx.x; q < ny * g.X; q += 256) {
        const int i = q / g.X, x = q - i * g.X;
        rpj_rows[i * g.X + x] = gproj[(size_t)(g.pad_y0 + y0 + i) * g.Xp + g.pad_x0 + x];
    }
    __syncthreads();
    for (int u = 0; u < RPJ_ADJ_VOX; ++u) {
        const size_t t = ((size_t)blockIdx.x * RPJ_ADJ_VOX + u) * 256 + threadIdx.x;
        if (t >= plane) return;
        float2* o = gobj + (size_t)y0 * plane + t;
        float2 cur[RPJ_ADJ_PLANES], a[RPJ_ADJ_PLANES];
#pragma unroll
        for (int i = 0; i < RPJ_ADJ_PLANES; ++i) {
            cur[i] = o[(size_t)min(i, ny - 1) * plane];       // in flight during the walk
            a[i] = make_float2(0.f, 0.f);
        }
        if (ptr == nullptr) {
            const int x = (int)(t / g.Z);
#pragma unroll
            for (int i = 0; i < RPJ_ADJ_PLANES; ++i)
                if (i < ny) a[i] = rpj_rows[i * g.X + x];
        } else {
            const int beg = ptr[t], end = ptr[t + 1];
            for (int j = beg; j < end; ++j) {
                const float w = wgt[j];
                const int x = (int)((unsigned)src[j] % slice) - g.pad_x0;
#pragma unroll
                for (int i = 0; i < RPJ_ADJ_PLANES; ++i) {
                    if (i < ny) {
                        const float2 v = rpj_rows[i * g.X + x];
                        a[i].x += w * v.x;
                        a[i].y += w * v.y;
                    }
                }
            }
        }
#pragma unroll
        for (int i = 0; i < RPJ_ADJ_PLANES; ++i)
            if (i < ny) o[(size_t)i * plane] = make_float2(cur[i].x + a[i].x, cur[i].y + a[i].y);
    }
}

static int rpj_range(const adm_plan* plan, int y_lo, int y_hi, const char* who) {
    if (y_lo < 0 || y_hi > plan->d.obj_y || y_lo > y_hi) return fail(ADM_ERR_INVALID, std::string(who) + ": bad y range");
    return ADM_OK;
}
}  // namespace adm
using namespace adm;

extern "C" int adm_rotate_project_fwd(adm_plan* plan, const float* obj, const uint16_t* coords, float* proj, int y_lo, int y_hi) {
    if (!plan || !obj || !proj) return fail(ADM_ERR_INVALID, "adm_rotate_project_fwd: null argument");
    if (const int rc = rpj_range(plan, y_lo, y_hi, "adm_rotate_project_fwd")) return rc;
    if (y_lo == y_hi) return ADM_OK;
    const adm_plan_desc& d = plan->d;
    RotGeom g{d.obj_y, d.obj_x, d.obj_z, plan->Yp, plan->Xp, d.pad_y0, d.pad_x0};
    const int ny = y_hi - y_lo, tiles = (d.obj_x + RPJ_TILE - 1) / RPJ_TILE;
    // RPJ_PLANES planes per workgroup share one evaluation of the weights, unless that leaves the chip short of workgroups
    if ((size_t)tiles * ((ny + RPJ_PLANES - 1) / RPJ_PLANES) >= RPJ_MIN_BLOCKS)
        hipLaunchKernelGGL(rotate_project_fwd_kernel<RPJ_PLANES>, dim3(tiles, (ny + RPJ_PLANES - 1) / RPJ_PLANES), dim3(RPJ_TILE * RPJ_TILE), 0,
                           plan->ctx->stream, (const float2*)obj, coords, (float2*)proj, g, y_lo, y_hi);
    else
        hipLaunchKernelGGL(rotate_project_fwd_kernel<1>, dim3(tiles, ny), dim3(RPJ_TILE * RPJ_TILE), 0, plan->ctx->stream, (const float2*)obj,
                           coords, (float2*)proj, g, y_lo, y_hi);
    ADM_HIP(hipGetLastError());
    return ADM_OK;
}

extern "C" int adm_rotate_project_adj(adm_plan* plan, const float* grad_proj, const int32_t* csr_ptr, const int32_t* csr_src,
                                      const float* csr_w, float* grad_obj, int y_lo, int y_hi, int lanes_along_x) {
    if (!plan || !grad_proj || !grad_obj) return fail(ADM_ERR_INVALID, "adm_rotate_project_adj: null argument");
    if ((csr_ptr || csr_src || csr_w) && !(csr_ptr && csr_src && csr_w))
        return fail(ADM_ERR_INVALID, "adm_rotate_project_adj: the three tables come together, or none of them (no rotation)");
    if (const int rc = rpj_range(plan, y_lo, y_hi, "adm_rotate_project_adj")) return rc;
    if (y_lo == y_hi) return ADM_OK;
    const adm_plan_desc& d = plan->d;
    // lanes_along_x: the gather reads LDS, where no lane order is the coalesced one: lanes run along z (grad_obj, the tables) for
    // either value, with the same bits
    (void)lanes_along_x;
    const size_t lds = (size_t)RPJ_ADJ_PLANES * d.obj_x * sizeof(float2);
    if (lds > RPJ_ADJ_LDS_MAX) return fail(ADM_ERR_UNSUPPORTED, "adm_rotate_project_adj: rows of more than 2048 pixels do not fit the LDS stage");
    if ((size_t)plan->Yp * plan->Xp > 0x7fffffffu) return fail(ADM_ERR_UNSUPPORTED, "adm_rotate_project_adj: slice of more than 2^31 pixels");
    RotGeom g{d.obj_y, d.obj_x, d.obj_z, plan->Yp, plan->Xp, d.pad_y0, d.pad_x0};
    const size_t per_block = (size_t)256 * RPJ_ADJ_VOX;
    const dim3 grid((unsigned)(((size_t)d.obj_x * d.obj_z + per_block - 1) / per_block), (unsigned)((y_hi - y_lo + RPJ_ADJ_PLANES - 1) / RPJ_ADJ_PLANES));
    hipLaunchKernelGGL(rotate_project_adj_kernel, grid, dim3(256), lds, plan->ctx->stream, (const float2*)grad_proj, csr_ptr, csr_src, csr_w,
                       (float2*)grad_obj, g, y_lo, y_hi);
    ADM_HIP(hipGetLastError());
    return ADM_OK;
}
