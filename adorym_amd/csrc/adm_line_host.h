// The host setup of the line kernels (adm_line_fft.h), stated once for adm_holo_create, adm_ctf_create and adm_ctfinv_create: the
// sides a field may have, the twiddle table of a line length, and the frequency mesh.  Host code only.
#pragma once
#include <vector>
#include <cmath>
#include "adm_host.h"

namespace adm {

// a field side is a power of two in [ADM_LINE_MIN_SIDE, ADM_LINE_MAX_SIDE]: the lengths of ADM_LINE_SIZES
constexpr int ADM_LINE_MIN_SIDE = 16, ADM_LINE_MAX_SIDE = 2048;
inline bool line_side_ok(int n) { return n >= ADM_LINE_MIN_SIDE && n <= ADM_LINE_MAX_SIDE && (n & (n - 1)) == 0; }

// *out = device table exp(-2 pi i j / N), j < N
inline int line_upload_twiddles(adm_ctx* ctx, int N, float2** out) {
    std::vector<float2> t(N);
    for (int j = 0; j < N; ++j) {
        const double a = -2.0 * M_PI * (double)j / (double)N;
        t[j] = make_float2((float)std::cos(a), (float)std::sin(a));
    }
    int rc = adm_malloc(ctx, N * sizeof(float2), (void**)out);
    if (rc) return rc;
    return adm_h2d(ctx, *out, t.data(), N * sizeof(float2));
}

// *out = device table [nx][ny]: u^2 + v^2 (nm^-2) of frequency (ky, kx) at [kx][ky]
inline int line_upload_uv2t(adm_ctx* ctx, int ny, int nx, double voxel_nm_y, double voxel_nm_x, float** out) {
    // gen_freq_mesh (adorym/propagate.py:54-60): u along y, v along x; cast to fp32 before squaring like the tensors
    const size_t n = (size_t)ny * nx;
    std::vector<float> uv(n);
    for (int y = 0; y < ny; ++y) {
        const int ky = y < (ny + 1) / 2 ? y : y - ny;
        const float u = (float)(((double)ky / ny) / voxel_nm_y);
        for (int x = 0; x < nx; ++x) {
            const int kx = x < (nx + 1) / 2 ? x : x - nx;
            const float v = (float)(((double)kx / nx) / voxel_nm_x);
            uv[(size_t)x * ny + y] = u * u + v * v;
        }
    }
    int rc = adm_malloc(ctx, n * sizeof(float), (void**)out);
    if (rc) return rc;
    return adm_h2d(ctx, *out, uv.data(), n * sizeof(float));
}

}  // namespace adm
