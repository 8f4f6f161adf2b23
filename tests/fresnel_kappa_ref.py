"""NumPy restatement of the single-material constraint of Fresnel multi-distance holography (test infrastructure only: the checker,
never the product).

  kappa = 10 ** ctf_lg_kappa[0] handed to the forward model   adorym/forward_model.py:876-878, 1003-1010
  beta_slice = delta_slice * kappa                            adorym/propagate.py:223-225

NOTE the sense: beta = kappa delta here, cos(xi) / kappa in the CTF model (tests/ctf_ref.py) -- the reference's two meanings of one
number, restated and not reconciled.

Two layers.  (1) The float32 mirrors of the two kernels of adm_kappa_tie.hip with their order of operations: kappa formed in double
and rounded once, the product and the sum of the fold rounded separately, the sum S over exactly representable products.  (2) The
multi-distance forward / adjoint with kappa, built on the oracle's functions through tests/multidist3d_ref.py (one sweep, D
free-space steps; S = 1 without a rotation is the undivided 2-D field), and the two driver loops.  The reference ties the ROTATED
object; the rotation is linear and acts on each channel alone, so tying in front of it -- as here and as on the GPU -- is the same
function, and in floating point the two differ by the rounding of one product.
"""
import math

import numpy as np

from oracle import adorym_oracle as O
from tests import multidist3d_ref as MR

LN10 = 2.302585092994045684


# ---------------------------------------------------------------------------------------------------- (1) the kernels' mirrors
def kappa64(lg_kappa):
    """exp(ln10 * (double)lg_kappa[0]) as the kernels form it; ``lg_kappa`` is rounded to float32 first, like the device array."""
    return math.exp(LN10 * float(np.float32(np.asarray(lg_kappa).reshape(-1)[0])))


def kappa32(lg_kappa):
    return np.float32(kappa64(lg_kappa))


def tie(obj, lg_kappa):
    """(delta, fl32(kappa) * delta) of float32 voxels [..., 2]; the beta channel of ``obj`` is not read."""
    d = np.asarray(obj, np.float32)[..., 0]
    return np.stack([d, kappa32(lg_kappa) * d], -1)


def fold(lg_kappa, grad_tied, grad_obj, mode):
    """grad_obj after adm_kappa_fold: u = g_delta + fl32(fl32(kappa) * g_beta); mode 1 adds u to the delta channel and leaves beta,
    mode 2 writes (u, 0)."""
    gt = np.asarray(grad_tied, np.float32)
    u = gt[..., 0] + kappa32(lg_kappa) * gt[..., 1]          # (float32 arrays: each operation rounds once)
    out = np.array(grad_obj, np.float32, copy=True)
    if mode == 1:
        out[..., 0] = out[..., 0] + u
    else:
        out[..., 0], out[..., 1] = u, 0
    return out


def fold_sum_exact(obj, grad_tied):
    """S = sum_v delta_v * g_beta_v, exactly rounded: the products of two float32 values are exact in double, math.fsum adds them
    without error.  Also returns sum |delta_v g_beta_v|, the scale of the bound on a double sum in any order."""
    p = np.asarray(obj, np.float32)[..., 0].astype(np.float64).ravel() * np.asarray(grad_tied, np.float32)[..., 1].astype(np.float64).ravel()
    return math.fsum(p), math.fsum(np.abs(p))


def grad_lg_kappa32(lg_kappa, S):
    """(float)(ln10 * kappa * S) with kappa in double, evaluated left to right like the finishing kernel."""
    return np.float32(LN10 * kappa64(lg_kappa) * float(S))


# --------------------------------------------------------------------------------------------- (2) forward, adjoint, driver loops
def forward_adjoint(obj, lg_kappa, coords_fp16, probes, meas, phys, dists_cm, dtype='float64', raw_data_type='magnitude'):
    """L(delta, lg_kappa) = the multi-distance loss on the tied object (delta, 10^lg_kappa delta): obj [Y,X,S,2] (beta is not read),
    one undivided field of view at (0, 0), meas [D,Y,X].  Returns loss, pred [D,Y,X], grad [Y,X,S,2] w.r.t. the FREE object (its
    beta channel exactly zero), grad_lg_kappa, the probe gradient and 'grad_tied', the gradient w.r.t. the tied object."""
    dt = np.dtype(dtype)
    kappa = dt.type(10.0 ** float(np.asarray(lg_kappa).reshape(-1)[0]))
    delta = np.asarray(obj)[..., 0].astype(dt)
    tied = np.stack([delta, delta * kappa], -1)
    loss, pred, g, gp = MR.forward_adjoint_object(tied, coords_fp16, np.asarray(probes), np.zeros((1, 2), int), np.asarray(meas), phys,
                                                  list(dists_cm), dt, raw_data_type=raw_data_type)
    grad = np.zeros_like(g)
    grad[..., 0] = g[..., 0] + kappa * g[..., 1]
    gk = math.log(10.) * float(kappa) * float((delta.astype(np.float64) * g[..., 1].astype(np.float64)).sum())
    return dict(loss=float(loss), pred=pred, grad=grad, grad_lg_kappa=gk, gprobe=gp, grad_tied=g)


def loss_only(obj, lg_kappa, coords_fp16, probes, meas, phys, dists_cm, raw_data_type='magnitude'):
    return forward_adjoint(obj, lg_kappa, coords_fp16, probes, meas, phys, dists_cm, 'float64', raw_data_type)['loss']


def reconstruct(prj, obj_init, probe, phys, dists_cm, theta_ls, lg_kappa, n_epochs=1, learning_rate=1e-3, ctf_lg_kappa_learning_rate=1e-3,
                raw_data_type='magnitude', dtype='float64', kappa_dtype=np.float64, two_d=False):
    """reconstruct_ptychography(optimize_ctf_lg_kappa=True, forward_algorithm='fresnel') on multi-distance data of one undivided
    field of view: prj [n_theta, D, Y, X]; 'immediate' updates, Adam on the object (its beta channel sees a zero gradient and does
    not move) and plain Adam on ctf_lg_kappa (optimizers.py:945-956), both with the driver's step counter, no regulariser, one
    rank.  ``two_d``: one slice, no rotation, the same angle in every epoch (so the counter is 0 throughout, ptychography.py:848).
    The control flow of multidist3d_ref.reconstruct.  ``kappa_dtype``: float64 as the reference keeps the parameter, float32 as
    the GPU driver does."""
    dt = np.dtype(dtype)
    obj = np.stack([obj_init[0], obj_init[1]], -1).astype(dt)
    m, v = np.zeros_like(obj), np.zeros_like(obj)
    k = np.array([lg_kappa], dtype=kappa_dtype)
    km, kv = np.zeros_like(k), np.zeros_like(k)
    pc = np.asarray(probe).astype(O._cdtype(dt))
    n_theta = 1 if two_d else len(theta_ls)
    tables, losses, trace = {}, [], []
    for i_epoch in range(n_epochs):
        batches = O.epoch_task_list(i_epoch, n_theta, 1, 1, 1, 'immediate')
        i_opt = 0
        for i_batch in range(len(batches)):
            i_theta, _ = O.rank_batch(batches, i_batch, 0, 1, 1)
            if not two_d and i_theta not in tables:
                tables[i_theta] = O.rotation_coords(obj.shape[:3], theta_ls[i_theta], dt)
            r = forward_adjoint(obj, k[0], None if two_d else tables[i_theta], pc, np.abs(prj[i_theta]), phys, dists_cm, dt, raw_data_type)
            losses.append(r['loss'])
            obj, m, v = O.adam_step(obj, r['grad'].astype(dt), m, v, i_opt, step_size=learning_rate)
            k, km, kv = O.adam_step(k, np.array([r['grad_lg_kappa']], dtype=kappa_dtype), km, kv, i_opt, step_size=ctf_lg_kappa_learning_rate)
            trace.append(float(k[0]))
            last_of_theta = i_batch == len(batches) - 1 or int(batches[i_batch + 1][0, 0]) != int(batches[i_batch][0, 0])
            if last_of_theta:
                i_opt += 1
    return dict(obj=obj, losses=losses, lg_kappa=float(k[0]), lg_kappa_trace=trace)
