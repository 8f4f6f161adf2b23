// The bilinear sample of the rotation about axis 0, shared by the kernels that gather with it (adm_rotate.hip,
// adm_rotate_project.hip).  Reference: apply_rotation -> w.grid_sample (adorym/util.py:536-552, adorym/wrappers.py:1105-1147),
// torch grid_sampler bilinear / border / align_corners=False.  The coordinate pipeline is fp16 table -> fp64 normalise -> fp32
// un-normalise -> clamp -> weights.
#pragma once
#include <hip/hip_runtime.h>
#include <hip/hip_fp16.h>
#include <cstdint>

namespace adm {
struct RotGeom {
    int Y, X, Z, Yp, Xp, pad_y0, pad_x0;
};

struct Bilin {
    int i00, i01, i10, i11;   // float2 offsets inside one y plane of obj ([X][Z])
    float w00, w01, w10, w11;
};

__device__ __forceinline__ Bilin make_bilin(const uint16_t* coords, int xr, int zr, int X, int Z) {
#pragma clang fp contract(off)      // torch / NumPy evaluate this pipeline without fused multiply-adds: match them bit for bit
    Bilin b;
    if (coords == nullptr) {
        b.i00 = b.i01 = b.i10 = b.i11 = xr * Z + zr;
        b.w00 = 1.f; b.w01 = b.w10 = b.w11 = 0.f;
        return b;
    }
    const __half* ch = reinterpret_cast<const __half*>(coords) + 2 * ((size_t)xr * Z + zr);
    const double x_old = (double)__half2float(ch[0]);
    const double z_old = (double)__half2float(ch[1]);
    // wrappers.py:1137: grid = -1 + 2*grid/arr_shape + 1/arr_shape on the flipped (z, x) pair, arr_shape = (X, Z)
    const float gz = (float)(-1.0 + 2.0 * z_old / (double)X + 1.0 / (double)X);
    const float gx = (float)(-1.0 + 2.0 * x_old / (double)Z + 1.0 / (double)Z);
    float iz = ((gz + 1.f) * (float)Z - 1.f) / 2.f;
    float ix = ((gx + 1.f) * (float)X - 1.f) / 2.f;
    iz = fminf((float)(Z - 1), fmaxf(iz, 0.f));
    ix = fminf((float)(X - 1), fmaxf(ix, 0.f));
    const float fz = floorf(iz), fx = floorf(ix);
    const float tz = iz - fz, tx = ix - fx;
    const int z0 = (int)fz, x0 = (int)fx;
    const bool vz = (z0 + 1 <= Z - 1), vx = (x0 + 1 <= X - 1);
    const int z1 = vz ? z0 + 1 : z0, x1 = vx ? x0 + 1 : x0;
    b.i00 = x0 * Z + z0; b.i01 = x0 * Z + z1; b.i10 = x1 * Z + z0; b.i11 = x1 * Z + z1;
    b.w00 = (1.f - tx) * (1.f - tz);
    b.w01 = vz ? (1.f - tx) * tz : 0.f;
    b.w10 = vx ? tx * (1.f - tz) : 0.f;
    b.w11 = (vx && vz) ? tx * tz : 0.f;
    return b;
}

// The four-term sample in float32, the terms in the order rotate_fwd_kernel writes them.  That kernel keeps its own inline copy of
// the expression and both are compiled under the default contraction, so the compiler is free to fuse them differently: the fused
// gather is held to the sample's error bound, not to rotate_fwd_kernel's bits (in practice they agree).
__device__ __forceinline__ float2 bilin_sample(const Bilin& b, float2 v00, float2 v01, float2 v10, float2 v11) {
    float2 r;
    r.x = v00.x * b.w00 + v01.x * b.w01 + v10.x * b.w10 + v11.x * b.w11;
    r.y = v00.y * b.w00 + v01.y * b.w01 + v10.y * b.w10 + v11.y * b.w11;
    return r;
}
}  // namespace adm
