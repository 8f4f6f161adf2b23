// Host-side definitions shared by the libadm translation units (not part of the C ABI): contexts, plans, the workspace layout,
// error plumbing and the launcher prototypes.  Nothing here is read by device code of adm_multislice.hip; what that kernel
// takes as arguments is in adm_common.h.
#pragma once
#include <hip/hip_runtime.h>
#include <string>
#include <cstdio>
#include "../../include/adm.h"
#include "adm_common.h"

#define ADM_MAXCOVER 64    // cover-list entries per rotated-frame pixel (adm_overlap_add.hip: cover_build_kernel)

struct adm_ctx {
    int device;
    hipStream_t stream;      // stream new work is enqueued on (main, or aux between adm_ctx_fork / adm_ctx_end_fork)
    hipStream_t main_stream;
    hipStream_t aux_stream;  // side stream for work that is independent of the multislice chain
    hipEvent_t ev_fork, ev_join;
    bool owns_stream;
    bool join_pending;
    void* comm;              // ncclComm_t of adm_comm_init (adm_comm.hip) or nullptr
    void* comm_aux;          // ncclComm_t of adm_comm_init_aux: collectives queued on the side stream, or nullptr
    int comm_rank, comm_size;
    void* p2p;               // peer-to-peer group of adm_p2p_create (adm_p2p.hip) or nullptr
};

struct adm_plan {
    adm_ctx* ctx = nullptr;
    adm_plan_desc d = {};            // host pointers inside are NOT kept valid; see device copies below
    int Yp = 0, Xp = 0;              // padded rotated-frame extents
    int n_steps = 0;                 // ceil(obj_z / binning)
    float2* h_dev = nullptr;         // [Py*Px] slice transfer function
    float2* hfree_dev = nullptr;     // [n_hfree][Py*Px] or nullptr
    int n_hfree = 1;                 // detector-plane Fresnel kernels held (1; adm_plan_set_detector_kernels: the distances of multi-distance data)
    float2* twid_dev = nullptr;      // [Px] exp(-2 pi i j / N)
    float* det_weight_dev = nullptr; // [Py*Px] beamstop weights or nullptr (adm_plan_set_detector_mask)
    float* reg_stats = nullptr;      // 2 floats of scratch for the real_imag L1 regulariser (lazily allocated)
    float* reg_partial = nullptr;    // [obj_y*obj_x] per-row partial sums of the regulariser value (lazily allocated)
    bool generic = false;            // probe size outside the tuned kernels' set (or forced): adm_ms_generic.hip, pixel-major workspace rows
    bool streamed = false;           // adm_plan_create_streamed: adm_ms_streamed.hip (fields in the workspace, row / column launches); generic is set too
    int gen_nrx = 0, gen_nry = 0, gen_rx[8] = {}, gen_ry[8] = {};   // radix lists of the x / y transforms of the generic kernel
    float2* hs_dev = nullptr;        // [Py*Px] H / (Py*Px), one rounding per element (generic kernel)
    float2* hfree_s_dev = nullptr;   // same for the detector-plane Fresnel kernel, or nullptr
    float2* twid_y_dev = nullptr;    // [Py] exp(-2 pi i j / Py)
    float2* trans_dev = nullptr;     // [Z][Yp][Xp] slice transmissions of the voxels of trans_src, or nullptr (adm_plan_set_transmission_cache)
    const void* trans_src = nullptr; // the obj_rot buffer trans_dev was last filled from (adm_rotate_fwd / adm_transmission_refresh)
    bool trans_only = false;         // adm_plan_set_transmission_cache(plan, 2): adm_rotate_fwd writes ONLY the transmissions (obj_rot is an identity, not data)
    // adm_plan_set_slice_positions (streamed plans): sparse multislice
    const float* zpos_dev = nullptr; // [n_zpos] slice positions in cm, the CALLER's device buffer; nullptr = equidistant slices (h_dev)
    int n_zpos = 0;
    bool zpos_dirty = false;         // the table below has to be rebuilt from zpos_dev before the next launch
    double sp_lambda_nm = 0, sp_voxel_nm_y = 0, sp_voxel_nm_x = 0;
    float2* sp_hs_dev = nullptr;     // [n_zpos-1][Py*Px] H_s / (Py*Px)
    float* sp_a_dev = nullptr;       // [Py] then [Px]: a_yx = sp_a[y] + sp_a[Py + x], the phase of H per nm
    bool exit_shift = false;         // adm_plan_set_exit_shift (streamed plans): the workspace holds the kept spectrum and the dL/ds partials
    bool probe_shift = false;        // adm_plan_set_probe_shift (streamed plans): the workspace holds FFT2(probe) and the dL/ds partials
    int n_fan = 0;                   // adm_plan_set_detector_fanout (streamed plans): detector planes per position, 0 = off
    float2* fan_hs_dev = nullptr;    // [n_fan][Py*Px] H_d / (Py*Px), one rounding per element
    // adm_plan_set_fanout_distances: the distances of the fan-out are parameters that live on the device
    const float* fan_dists_dev = nullptr;   // [n_fan] distances in cm, the CALLER's device buffer; nullptr = host-built kernels (above)
    bool fan_dists_dirty = false;    // fan_hs_dev has to be rebuilt from fan_dists_dev before the next launch
    double fd_lambda_nm = 0, fd_voxel_nm_y = 0, fd_voxel_nm_x = 0;
    float* fan_a_dev = nullptr;      // [Py] then [Px]: a_yx = fan_a[y] + fan_a[Py + x], the phase of H_d per nm
    // adm_tile_cover_build: the cover lists in workspace `ws` are current for (pos, batch, window); a few entries, so that every
    // round of a batch launched in parts can have its lists built ahead
    struct CoverKey { const void* ws; const void* pos; int batch, row0, nrows; unsigned long long fp; } cover_keys[4] = {};
};

namespace adm {
void set_error(const std::string& msg);
int fail(int code, const std::string& msg);
int hip_fail(hipError_t e, const char* what);

int ms_threads_for(int n);
int ms_r1_for(int n);
int ms_r2_for(int n);
size_t ms_row_elems(const adm_plan* plan);

// The one description of a multislice workspace of `batch` positions: the byte offset of every section, in this order, and the
// size of the whole.  M = n_modes, row = ms_row_elems float2, S = n_zpos, cg = ms_streamed_col_groups.  E = detector entries:
// B, or B * n_fan on a plan with a detector fan-out.
struct WsLayout {
    size_t stash;       // [B][M][n_steps][row] post-modulation wavefields
    size_t gtile;       // [B][n_steps][row] per-position tile gradients
    size_t cover;       // [Yp*Xp][1 + ADM_MAXCOVER] u32 cover lists of the overlap-add ...
    size_t overflow;    // ... and 64 bytes behind them whose first int is the overflow flag
    size_t det;         // [E][M][G*NT or Py*Px] parked detector-plane fields (M > 1)
    size_t gprobe;      // [B][M][Py][Px] per-position probe-gradient slots
    size_t field;       // streamed plans: [B][M][Py][Px] fields
    size_t loss_part;   // streamed plans: [E][cg] float loss partials
    size_t keep;        // sparse plans (streamed, S >= 2): [B][M][S-1][Py][Px] kept spectra
    size_t dd_part;     // sparse plans: [S-1][B*M*cg] double dL/dd partials
    size_t xs_keep;     // plans with exit-wave shifts (streamed): [B][M][Py][Px] kept detector-step spectra
    size_t xs_part;     // plans with exit-wave shifts: [B*M*cg][2] double dL/ds partials
    size_t ps_phat;     // plans with probe shifts (streamed): [M][Py][Px] FFT2 of the probe modes
    size_t ps_part;     // plans with probe shifts: [B*M*cg][2] double dL/ds partials
    size_t fan_field;   // plans with a detector fan-out (streamed): [E][M][Py][Px] detector-plane fields
    size_t fan_pos;     // plans with a detector fan-out: [E] int2 zeros, the positions of the row launches over the detector fields
    size_t fan_keep;    // plans whose fan-out distances are refined (adm_plan_set_fanout_distances): [B][M][Py][Px] kept exit-wave spectra
    size_t fan_part;    // plans whose fan-out distances are refined: [D][B*M*cg] double dL/dd partials
    size_t total;
};
WsLayout ws_layout(const adm_plan* plan, int batch);

hipError_t probe_grad_reduce(const float2* part, int batch, size_t n, float2* out, hipStream_t st);
hipError_t probe_grad_reduce_large(float2* part, int batch, size_t n, float2* out, hipStream_t st);   // two levels, `part` is scratch
hipError_t ms_launch(int n, const MsParams& p, int batch, hipStream_t st);
bool ms_generic_supported(int py, int px);
int ms_generic_threads(int py, int px);
hipError_t ms_generic_launch(const MsParams& p, int batch, hipStream_t st);
bool ms_streamed_supported(int py, int px);
int ms_streamed_col_groups(int py, int px);
// n Fresnel transfer functions of py x px built on the device from float32 lengths (cm) as they sit in a caller's buffer: gaps != 0,
// table s is the gap between slice positions s and s + 1 of a sparse plan (n + 1 positions); gaps == 0, table d is detector distance d
// of a fan-out whose distances are refined
struct StFresnelGeom { int py, px, n, gaps; double sigma, lambda_nm, voxel_nm_y, voxel_nm_x; };
hipError_t ms_fresnel_table_launch(const StFresnelGeom& q, const float* src_cm, float2* hs, float* ay, float* ax, hipStream_t st);
// sparse multislice on streamed plans (adm_ms_streamed.hip)
struct StSparse {              // kernel argument of the column launches that serve the slice-position gradient
    float2* keep;              // [B][M][S-1][Py][Px] H_s * spectrum / (Py*Px) of the forward sweep
    double* part;              // [S-1][B*M*column groups] dL/dd partials
    const float* ay;           // [Py], [Px]: a_yx = ay[y] + ax[x]
    const float* ax;
    int step, n_conv;
};
struct StSparseLaunch {
    const float2* hs;          // [S-1][Py][Px]
    float2* keep; double* part; const float* ay; const float* ax;
    float* grad_z;             // [S] += dL/dz (cm), or nullptr
};
hipError_t ms_sparse_anchor_launch(float* z, int n, hipStream_t st);
int ms_sparse_max_slices();
// per-angle projection alignment on streamed plans (adm_ms_exitshift.hip): the detector step's column launches with a sub-pixel
// Fourier shift of the exit wave per position
struct StExitShift {           // kernel argument
    const float2* shifts;      // [n_entries] (s_y, s_x)
    const int* index;          // [B] entry of position b, or nullptr: b
    float2* keep;              // [B][M][Py][Px] Phi H_free * spectrum / (Py*Px) of the forward sweep, or nullptr: not kept / not read
    double* part;              // [B*M*column groups][2] dL/ds partials (before the factor 2 PI), or nullptr: no sums
};
struct StExitShiftLaunch {
    const float* shifts; const int32_t* index;
    float* grad_shifts;        // [n_entries][2] += dL/ds, or nullptr
    float2* keep; double* part;
};
// the detector step's column launch: hs = H_free / (Py*Px), or nullptr for H = 1
hipError_t ms_exitshift_col_launch(const MsParams& p, int batch, float2* fld, const float2* hs, bool conj, const StExitShiftLaunch& xs,
                                   hipStream_t st);
// sub-pixel probe positions on streamed plans (adm_plan_set_probe_shift, adm_ms_probeshift.hip): the probe modes Fourier-shifted
// by an offset per position inside the sweep
struct StProbeShift {          // kernel argument
    const float2* shifts;      // [n_entries] (s_y, s_x)
    const int* index;          // [B] entry of position b, or nullptr: b
    const float2* phat;        // [M][Py][Px] FFT2(probe_m), unnormalised
    double* part;              // [B*M*column groups][2] dL/ds partials (before the factor 2 PI), or nullptr: no sums
};
struct StProbeShiftLaunch {
    const float* shifts; const int32_t* index;
    float* grad_shifts;        // [n_entries][2] += dL/ds, or nullptr
    float2* phat; double* part;
};
hipError_t ms_probeshift_spectrum_launch(const MsParams& p, float2* phat, hipStream_t st);
hipError_t ms_probeshift_col_launch(const MsParams& p, int batch, float2* fld, bool conj, const StProbeShift& q, hipStream_t st);
// one exit wave to several detector planes on streamed plans (adm_plan_set_detector_fanout, adm_ms_multidist.hip): the detector
// step's column launches fan the B*M sweep fields out to B*D*M detector fields and back in
struct StFanout {              // kernel argument
    const float2* hs;          // [D][Py][Px] H_d / (Py*Px)
    float2* dfld;              // [B][D][M][Py][Px] detector-plane fields
    int n;                     // D
};
struct StDistGrad {            // kernel argument beside StFanout; read by the instantiations with the distance gradient only
    float2* keep;              // [B][M][Py][Px]
    double* part;              // [D][B*M*column groups]
    const float* ay;
    const float* ax;
};
struct StFanoutLaunch {
    int n; const float2* hs;
    float2* fld;               // [B*D][M][Py][Px] detector-plane fields
    float2* det;               // [B*D][M][Py][Px] the detector kernel's parked fields (M > 1), or nullptr
    const int2* pos;           // [B*D] zeros
    // the distance gradient (distances on the device: adm_plan_set_fanout_distances); grad_dists set = requested: the two launchers
    // below then start the instantiations that keep the spectra and form the partials
    float* grad_dists = nullptr;      // [D] += dL/d distance (per cm), or nullptr
    float2* keep = nullptr;    // [B][M][Py][Px] column-transformed spectra of the exit waves
    double* part = nullptr;    // [D][B*M*column groups] dL/dd partials
    const float* ay = nullptr; // [Py], [Px]: a_yx = ay[y] + ax[x]
    const float* ax = nullptr;
};
hipError_t ms_multidist_fanout_launch(const MsParams& p, int batch, const float2* fld, const StFanoutLaunch& fo, hipStream_t st);
hipError_t ms_multidist_fanin_launch(const MsParams& p, int batch, float2* fld, const StFanoutLaunch& fo, hipStream_t st);
// the streamed launch sequence of one minibatch: fld = [B][M][Py][Px] field buffer, part = [B][col groups] loss partials;
// sp: the tables of a sparse plan, or nullptr; xs: the exit-wave shifts of a plan with adm_plan_set_exit_shift, or nullptr; ps:
// the probe shifts of a plan with adm_plan_set_probe_shift, or nullptr; fo: the detector fan-out of a plan with
// adm_plan_set_detector_fanout, or nullptr (part is then [B*D][col groups] and p.target / p.pred / p.loss_sum hold B*D entries)
hipError_t ms_streamed_launch(const MsParams& p, int batch, float2* fld, float* part, hipStream_t st, const StSparseLaunch* sp = nullptr,
                              const StExitShiftLaunch* xs = nullptr, const StFanoutLaunch* fo = nullptr,
                              const StProbeShiftLaunch* ps = nullptr);
// One multislice launch: the arguments every adm_multislice_fwd_adj* entry point takes behind the plan, then what single entry
// points add, absent unless set (xs / ps: absent = no shifts; their keep / phat / part come from the workspace)
struct MsCall {
    const float* obj_rot; const float* probe; const int32_t* pos; int batch; const float* target; int want_grad;
    float* grad_probe; float* pred; float* loss_sum; float grad_scale; void* workspace; size_t workspace_bytes;
    bool per_position = false;        // adm_multislice_fwd_adj_pp: one probe set per position
    float* grad_slice_pos = nullptr;  // adm_multislice_fwd_adj_sparse
    StExitShiftLaunch xs = {};        // adm_multislice_fwd_adj_exit_shift
    StProbeShiftLaunch ps = {};       // adm_multislice_fwd_adj_probe_shift
    float* grad_dists = nullptr;      // adm_multislice_fwd_adj_fanout_dist
};
int multislice_call(adm_plan* plan, const MsCall& c);
hipError_t shift_launch(int n, const ShiftParams& q, int batch, bool adjoint, hipStream_t st);
inline int stream_grid(size_t n) {      // blocks of 256 threads for a grid-stride pass over n elements
    size_t b = (n + 255) / 256;
    return (int)(b > 4096 ? 4096 : (b ? b : 1));
}
}  // namespace adm

#define ADM_HIP(call)                                          \
    do {                                                       \
        hipError_t e__ = (call);                               \
        if (e__ != hipSuccess) return adm::hip_fail(e__, #call); \
    } while (0)
