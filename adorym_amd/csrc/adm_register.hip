// Affine registration of the measured holograms of multi-distance holography, as kernels of their own (adm_register_*): the
// reference's optimize_prj_affine (adorym/forward_model.py:1066-1072, w.affine_transform wrappers.py:1159-1174 = F.affine_grid +
// F.grid_sample, bilinear, border padding, align_corners=False) for the paths whose forward model is NOT adm_holo.hip -- a 3-D
// object on the streamed multislice path with a detector fan-out.  The registration acts on the data, not on the wave:
//   target  reg_sample_kernel: target[d][y][x] = |samp| (magnitude data) or sqrt|samp| (intensity data), samp the bilinear sample of
//           |data[d]| at the point theta[d] maps base coordinate (X, Y) to.  The fan-out launch takes it as its `target`.
//   grad    reg_grad_kernel: with the launch's predictions, c = -(2/N) grad_scale (pred - target) dtarget/dsamp (N = D*Py*Px; 0 where
//           that is not finite), the four samples fetched again, dix / diy as holo_k3 (adm_holo.hip) forms them, six fp64 sums per
//           workgroup: ONE partial per (d, block) and matrix entry.
//   reduce  reg_reduce_kernel: one workgroup per matrix entry adds its partials in a fixed order, grad_affine[d][q] += sum.
// No atomics: the same inputs give the same bits.  Any Py, Px in [2, 2048], D in [1, 64].
#include <hip/hip_runtime.h>
#include <cstring>
#include "adm_host.h"
#include "adm_ms_col.h"

#define REG_NT 256           // threads of a sample / gradient workgroup = detector pixels per workgroup
#define REG_RED_NT 256       // threads of a reduce workgroup = the stride of its pass over the partials

struct adm_register {
    adm_ctx* ctx;
    int n_dists, ny, nx, intensity;
    int n_blocks;             // workgroups per distance: ceil(ny*nx / REG_NT)
    double* part;             // [n_dists][6][n_blocks] partials of dL/dtheta
};

namespace adm {

// torch's affine_grid base coordinate and the affine map in pixels, float for float those of adm_holo.hip (base_coord,
// affine_coords; the comment there records why): the linspace evaluated from both ends with a fused multiply-add, every product
// and sum of the map rounded on its own.
__device__ __forceinline__ float reg_base_coord(int i, int n) {
    const float step = 2.0f / (float)(n - 1);
    const float lin = (i < n / 2) ? fmaf(step, (float)i, -1.0f) : fmaf(-step, (float)(n - 1 - i), 1.0f);
    return (lin * (float)(n - 1)) / (float)n;
}
__device__ __forceinline__ void reg_affine_coords(const float (&th)[6], float X, float Y, int nx, int ny, float& ix, float& iy) {
#pragma clang fp contract(off)
    const float gx = th[0] * X + th[1] * Y + th[2];
    const float gy = th[3] * X + th[4] * Y + th[5];
    ix = ((gx + 1.f) * (float)nx - 1.f) * 0.5f;
    iy = ((gy + 1.f) * (float)ny - 1.f) * 0.5f;
}

struct RegGeom { int ny, nx, intensity; };

// the sample of pixel (y, x): base coordinates, border masks, weights and the four values
struct RegSample { float X, Y, mx, my, wx, wy, v00, v01, v10, v11, samp; };

__device__ __forceinline__ RegSample reg_sample(const RegGeom& q, const float (&th)[6], const float* __restrict__ img, int y, int x) {
    RegSample s;
    s.X = reg_base_coord(x, q.nx);
    s.Y = reg_base_coord(y, q.ny);
    float ix, iy;
    reg_affine_coords(th, s.X, s.Y, q.nx, q.ny, ix, iy);
    s.mx = (ix > 0.f && ix < (float)(q.nx - 1)) ? 1.f : 0.f;      // grid_sampler's clip_coordinates_set_grad
    s.my = (iy > 0.f && iy < (float)(q.ny - 1)) ? 1.f : 0.f;
    ix = fminf(fmaxf(ix, 0.f), (float)(q.nx - 1));                 // (a NaN coordinate lands on 0: every index stays inside)
    iy = fminf(fmaxf(iy, 0.f), (float)(q.ny - 1));
    const int x0 = (int)floorf(ix), y0 = (int)floorf(iy);
    const int x1 = min(x0 + 1, q.nx - 1), y1 = min(y0 + 1, q.ny - 1);
    s.wx = ix - (float)x0;
    s.wy = iy - (float)y0;
    s.v00 = fabsf(img[(size_t)y0 * q.nx + x0]); s.v01 = fabsf(img[(size_t)y0 * q.nx + x1]);
    s.v10 = fabsf(img[(size_t)y1 * q.nx + x0]); s.v11 = fabsf(img[(size_t)y1 * q.nx + x1]);
    s.samp = s.v00 * (1.f - s.wx) * (1.f - s.wy) + s.v01 * s.wx * (1.f - s.wy) + s.v10 * (1.f - s.wx) * s.wy + s.v11 * s.wx * s.wy;
    return s;
}

// one thread per pixel, blockIdx.y = the distance: its matrix is uniform over the workgroup
__global__ __launch_bounds__(REG_NT) void reg_sample_kernel(RegGeom q, const float* __restrict__ data, const float* __restrict__ affine,
                                                            float* __restrict__ target) {
    const int d = blockIdx.y;
    const size_t n = (size_t)q.ny * q.nx, i = (size_t)blockIdx.x * REG_NT + threadIdx.x;
    float th[6];
#pragma unroll
    for (int k = 0; k < 6; ++k) th[k] = affine[d * 6 + k];
    if (i >= n) return;
    const int y = (int)(i / q.nx), x = (int)(i - (size_t)y * q.nx);
    const RegSample s = reg_sample(q, th, data + (size_t)d * n, y, x);
    const float as = fabsf(s.samp);
    target[(size_t)d * n + i] = q.intensity ? sqrtf(as) : as;
}

// part[(d * 6 + k) * gridDim.x + blockIdx.x] = this workgroup's share of dL/dtheta[d] entry k; cscale = -(2/N) grad_scale
__global__ __launch_bounds__(REG_NT) void reg_grad_kernel(RegGeom q, const float* __restrict__ data, const float* __restrict__ affine,
                                                          const float* __restrict__ pred, float cscale, double* __restrict__ part) {
    __shared__ double red[6 * (REG_NT / 64)];
    const int d = blockIdx.y;
    const size_t n = (size_t)q.ny * q.nx, i = (size_t)blockIdx.x * REG_NT + threadIdx.x;
    float th[6];
#pragma unroll
    for (int k = 0; k < 6; ++k) th[k] = affine[d * 6 + k];
    double ga[6] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
    if (i < n) {
        const int y = (int)(i / q.nx), x = (int)(i - (size_t)y * q.nx);
        const RegSample s = reg_sample(q, th, data + (size_t)d * n, y, x);
        const float as = fabsf(s.samp);
        const float tgt = q.intensity ? sqrtf(as) : as;
        const float sg = (float)((s.samp > 0.f) - (s.samp < 0.f));
        float c = cscale * (pred[(size_t)d * n + i] - tgt) * (q.intensity ? sg / (2.f * sqrtf(as)) : sg);
        if (!(fabsf(c) <= 3.0e38f)) c = 0.f;                      // 0/0 at an exactly zero sample
        const float dix = ((s.v01 - s.v00) * (1.f - s.wy) + (s.v11 - s.v10) * s.wy) * s.mx * (0.5f * (float)q.nx) * c;
        const float diy = ((s.v10 - s.v00) * (1.f - s.wx) + (s.v11 - s.v01) * s.wx) * s.my * (0.5f * (float)q.ny) * c;
        ga[0] = (double)(dix * s.X); ga[1] = (double)(dix * s.Y); ga[2] = (double)dix;
        ga[3] = (double)(diy * s.X); ga[4] = (double)(diy * s.Y); ga[5] = (double)diy;
    }
    st_block_sum_f64(ga, red, (int)threadIdx.x, REG_NT, true);
    if (threadIdx.x == 0) {
#pragma unroll
        for (int k = 0; k < 6; ++k) part[((size_t)d * 6 + k) * gridDim.x + blockIdx.x] = ga[k];
    }
}

// grad_affine[o] += (the npart partials of output o = d * 6 + k added in a fixed order); one workgroup per output
__global__ __launch_bounds__(REG_RED_NT) void reg_reduce_kernel(const double* __restrict__ part, int npart, float* grad_affine) {
    __shared__ double red[REG_RED_NT];
    const int t = threadIdx.x, o = blockIdx.x;
    double a = 0.0;
    for (int i = t; i < npart; i += REG_RED_NT) a += part[(size_t)o * npart + i];
    red[t] = a;
    __syncthreads();
    for (int h = REG_RED_NT / 2; h > 0; h >>= 1) {
        if (t < h) red[t] += red[t + h];
        __syncthreads();
    }
    if (t == 0) grad_affine[o] += (float)red[0];
}

}  // namespace adm

using adm::fail;

extern "C" int adm_register_create(adm_ctx* ctx, int n_dists, int ny, int nx, int intensity, adm_register** out) {
    if (!ctx || !out) return fail(ADM_ERR_INVALID, "adm_register_create: null argument");
    if (ny < 2 || ny > 2048 || nx < 2 || nx > 2048) return fail(ADM_ERR_UNSUPPORTED, "adm_register_create: field sizes must be in [2, 2048]");
    if (n_dists < 1 || n_dists > 64) return fail(ADM_ERR_INVALID, "adm_register_create: n_dists must be in [1, 64]");
    adm_register* r = new adm_register();
    std::memset(r, 0, sizeof(*r));
    r->ctx = ctx;
    r->n_dists = n_dists; r->ny = ny; r->nx = nx; r->intensity = intensity ? 1 : 0;
    r->n_blocks = (int)(((size_t)ny * nx + REG_NT - 1) / REG_NT);
    const int rc = adm_malloc(ctx, (size_t)n_dists * 6 * r->n_blocks * sizeof(double), (void**)&r->part);
    if (rc) {
        delete r;
        return rc;
    }
    *out = r;
    return ADM_OK;
}

extern "C" int adm_register_destroy(adm_register* r) {
    if (!r) return ADM_OK;
    if (r->part) adm_free(r->ctx, r->part);
    delete r;
    return ADM_OK;
}

extern "C" int adm_register_targets(adm_register* r, const float* data, const float* affine, float* target) {
    if (!r || !data || !affine || !target) return fail(ADM_ERR_INVALID, "adm_register_targets: null argument");
    adm::RegGeom q;
    q.ny = r->ny; q.nx = r->nx; q.intensity = r->intensity;
    hipLaunchKernelGGL(adm::reg_sample_kernel, dim3((unsigned)r->n_blocks, (unsigned)r->n_dists), dim3(REG_NT), 0, r->ctx->stream, q, data,
                       affine, target);
    ADM_HIP(hipGetLastError());
    return ADM_OK;
}

extern "C" int adm_register_grad(adm_register* r, const float* data, const float* affine, const float* pred, float grad_scale,
                                 float* grad_affine) {
    if (!r || !data || !affine || !pred || !grad_affine) return fail(ADM_ERR_INVALID, "adm_register_grad: null argument");
    adm::RegGeom q;
    q.ny = r->ny; q.nx = r->nx; q.intensity = r->intensity;
    const float cscale = (float)(-2.0 / ((double)r->n_dists * r->ny * r->nx)) * grad_scale;
    hipLaunchKernelGGL(adm::reg_grad_kernel, dim3((unsigned)r->n_blocks, (unsigned)r->n_dists), dim3(REG_NT), 0, r->ctx->stream, q, data,
                       affine, pred, cscale, r->part);
    ADM_HIP(hipGetLastError());
    hipLaunchKernelGGL(adm::reg_reduce_kernel, dim3((unsigned)(6 * r->n_dists)), dim3(REG_RED_NT), 0, r->ctx->stream,
                       (const double*)r->part, r->n_blocks, grad_affine);
    ADM_HIP(hipGetLastError());
    return ADM_OK;
}
