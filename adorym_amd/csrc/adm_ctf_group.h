// libadm -- the handle of the CTF forward model and the runner of its launch group (adm_holo_ctf.hip), for the entry points that
// live in other files: adm_ctf_fwd_adj (adm_holo_ctf.hip; host distances) and adm_ctfd_fwd_adj (adm_ctf_dist.hip; distances on the
// device, dL/d dists).  Host code only.
#pragma once
#include "adm_host.h"

struct adm_ctf {
    adm_ctx* ctx;
    adm_ctf_desc d;
    float2 *tw_y, *tw_x;      // exp(-2 pi i j / N) for N = ny, nx
    float* uv2t;              // [nx][ny]: u^2 + v^2 (nm^-2) of frequency (ky, kx) at [kx][ky], fp32 like the reference's tensors
    float2 *T14, *Ft;         // T14 [nx][ny]: x spectra of the rows (C1 -> C2), later the y-inverse of G (C4 -> C5); Ft [nx][ny] = FFT2(D)
    float2 *W, *T3;           // [n_dists][ny][nx] / [n_dists][nx][ny] work fields
    float* part3;             // [n_dists][ny] per-row loss sums
    double* part4;            // [nx] per-line sums of the kappa gradient
    float* loss_scratch;      // [n_dists]: where the loss sums go when the caller wants none
    double* partd;            // [n_dists][nx] per-line sums of the distance gradient; allocated by the first call that wants them
};

namespace adm {
namespace ctf {

// One launch group (C1 ... C5, or C1 ... C3 and the loss sums) on the handle's stream; `who` names the entry point in messages.
// Exactly one of dists_cm (HOST doubles) and dists_dev (DEVICE floats, cm) is given.  grad_dists [n_dists] (device; needs
// h->partd) follows want_grad like grad_lg_kappa.  The other arguments are those of adm_ctf_fwd_adj (include/adm.h).
int group_run(adm_ctf* h, const char* who, const float* obj, const double* dists_cm, const float* dists_dev, const float* lg_kappa,
              const float* data, int want_grad, float* grad_obj, float* grad_lg_kappa, float* grad_dists, float* pred, float* loss_sum);

}  // namespace ctf
}  // namespace adm
