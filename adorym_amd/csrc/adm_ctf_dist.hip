// libadm -- the CTF forward model with its distances on the device and their gradient (optimize_free_prop under
// forward_algorithm='ctf'; adorym/propagate.py:467-476, 590-606 with free_prop_cm a tensor that requires grad).
//
// The launch group is the one of adm_holo_ctf.hip (adm_ctf_group.h): C2 and C4 form c_d from the float32 array in cm with the
// reference's float32 roundings, C4 writes one double partial of dL/dd_d per (d, kx) and C5's blocks sum them in a fixed order.  No
// kernel lives here: this file holds the entry point and the partials' buffer, [n_dists][nx] doubles, allocated by the first call
// that asks for dL/dd and freed by adm_ctf_destroy.
#include "adm_ctf_group.h"

using namespace adm;

extern "C" int adm_ctfd_fwd_adj(adm_ctf* h, const float* obj, const float* dists_cm_dev, const float* lg_kappa, const float* data,
                                int want_grad, float* grad_obj, float* grad_lg_kappa, float* grad_dists, float* pred, float* loss_sum) {
    if (!h || !dists_cm_dev) return fail(ADM_ERR_INVALID, "adm_ctfd_fwd_adj: null argument");
    if (want_grad && grad_dists && !h->partd) {
        int rc = adm_malloc(h->ctx, (size_t)h->d.n_dists * h->d.nx * sizeof(double), (void**)&h->partd);
        if (rc) return rc;
    }
    return ctf::group_run(h, "adm_ctfd_fwd_adj", obj, nullptr, dists_cm_dev, lg_kappa, data, want_grad, grad_obj, grad_lg_kappa, grad_dists,
                          pred, loss_sum);
}
