// Kernel-argument structs of the multislice and probe-shift kernels, and nothing else.
// bench.py hashes this file together with adm_multislice.hip, adm_fft.h and adm_ms_math.h and accepts the measured HBM traffic
// of profiles/traffic_latest.json only while that hash matches its stamp: whatever is declared here is taken to be part of
// ms_fwd_adj_kernel.  So this header changes only when a kernel argument changes.  Host bookkeeping (contexts, plans, the
// workspace layout, launcher prototypes) lives in adm_host.h.
#pragma once
#include <hip/hip_runtime.h>

#define ADM_DET_NONE_ 0
#define ADM_DET_FARFIELD_ 1
#define ADM_DET_FRESNEL_ 2

namespace adm {
struct MsParams {
    const float2* obj_rot;     // [Z][Yp][Xp] (delta, beta); pre_t: the cached slice transmissions instead
    int want_grad;             // 0 = forward only
    const float2* probe;       // [P][P]
    float2* grad_probe;        // [P][P] or nullptr
    const int2* pos;           // [B] (y, x) in object coordinates
    const float* target;       // [B][P][P]
    float* pred;               // [B][P][P] or nullptr
    float* loss_sum;           // [B]
    float2* stash;             // [B][n_steps][R1][NT] post-modulation wavefields
    float2* gtile;             // [B][n_steps][R1][NT] per-position tile gradients (d/ddelta, d/dbeta)
    const float2* h;           // [P][P] natural order, unscaled
    const float2* hfree;       // [n_hfree][P][P] or nullptr
    const float2* twid;        // [N] exp(-2 pi i j / N)
    int Z, Yp, Xp, pad_y0, pad_x0;
    int binning, n_steps;
    int det_mode, det_inverse;     // det_inverse: far field uses the inverse transform (sign_convention -1)
    float det_scale;               // far-field scale: 1, 1/N^2, or 1/N (ortho)
    float k1, sigma;
    float grad_scale;
    int n_modes;               // incoherent probe modes
    float2* det;               // [B][n_modes][G][NT] detector-plane fields of the modes (n_modes > 1 only)
    int loss_type;             // 0 LSQ on magnitudes, 1 Poisson
    float poisson_mult;
    int real_imag;             // unknown_type == 'real_imag'
    int pre_t;                 // obj_rot holds exp(-k1 beta) (cos, sin)(-sigma k1 delta) per voxel (adm_plan_set_transmission_cache)
    const float* det_weight;   // [P][P] 0/1 weights of the detector pixels in the loss (beamstop), reference layout; or nullptr
    size_t probe_bstride;      // float2 elements between the probes of consecutive positions (0 = one shared probe set)
    size_t gprobe_bstride;     // same for grad_probe (per-position gradients when the probes are per position)
    // generic kernel (adm_ms_generic.hip) only
    int gen_py, gen_px, gen_nrx, gen_nry, gen_rx[8], gen_ry[8];
    const float2* gen_twid_y;  // [Py]; twid is [Px]
    const float2* gen_hs;      // [Py][Px] H / (Py*Px)
    const float2* gen_hfree_s; // [n_hfree][Py][Px] or nullptr
    // (last, so that the fields above keep their kernel-argument offsets)
    int n_hfree;               // detector-plane kernels in hfree / gen_hfree_s: position b is propagated with kernel b % n_hfree
};
// per-position sub-pixel probe shifts (adorym/util.py:380-397, forward_model.py:296-311)
struct ShiftParams {
    const float2* probe;       // [M][P][P]
    const float2* shifts;      // (sy, sx) entries; entry of position b = shifts[index ? index[b] : b]
    const int* index;          // [B] or nullptr
    float2* probes_out;        // forward: [B][M][P][P]
    const float2* grad_probes; // adjoint: [B][M][P][P]
    float2* slots;             // adjoint, large batches: every (position, mode) leaves its probe-gradient term in its own [P][P] slot
                               // (= grad_probes, in place) for a fixed-order sum afterwards instead of atomics on grad_probe
    float2* grad_probe;        // adjoint: [M][P][P] accumulated (atomics) or nullptr
    float* grad_shifts;        // adjoint: accumulated (atomics) at [index ? index[b] : b][2]
    const float2* twid;
    int n_modes;
};
}  // namespace adm
