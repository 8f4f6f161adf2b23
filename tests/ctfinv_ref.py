"""NumPy restatement of the direct inversion of the CTF model (update_using_external_algorithm='ctf': adorym/array_ops.py:274-286,
adorym/conventional.py:112-152, multidistance_ctf_wrapped) and of the driver loop that overwrites the delta channel with it.
fp64, and float32 with the roundings of the reference's float32 run: I - 1 in float32, orthonormal transforms in complex64,
PI * lambda_nm * dist_nm a Python double that meets a float32 tensor (rounded once), u^2 + v^2 a float32 tensor, 1 / kappa formed
in double and rounded once, the regulariser a float32.

It serves the fields too large for golden F31 (tests/test_ctfinv_ref_vs_golden.py holds it to the golden where both exist).
safe_zone_width is 0 and nothing is registered, as in the kernels (include/adm.h, adm_ctfinv_*)."""
import numpy as np
import scipy.fft as sfft

from oracle.adorym_oracle import adam_step
from tests import ctf_ref as R

ALPHA = 1e-10               # adorym/conventional.py:146


def weights(shape, dists_cm, lg_kappa, energy_ev, psize_cm, dtype=np.float64):
    """w_d = sin xi_d + cos xi_d / kappa  [n_dists, ny, nx]: half of ctf_ref.osc."""
    dt = np.dtype(dtype).type
    sn, cs = R.xi_sincos(shape, dists_cm, energy_ev, psize_cm, dt)
    return sn + dt(1. / 10. ** float(lg_kappa)) * cs


def retrieve(data, dists_cm, lg_kappa, energy_ev, psize_cm, alpha=None, dtype=np.float64):
    """data [n_dists, ny, nx] (raw, used as given) or [B, n_dists, ny, nx]; alpha: None (1e-10), a scalar or [ny, nx] in fftfreq
    order.  Returns the phase map(s) [ny, nx] / [B, ny, nx]."""
    dt = np.dtype(dtype).type
    I = np.asarray(data, dtype=dt)
    if I.ndim == 4:
        return np.stack([retrieve(i, dists_cm, lg_kappa, energy_ev, psize_cm, alpha, dtype) for i in I])
    w = weights(I.shape[1:], dists_cm, lg_kappa, energy_ev, psize_cm, dt)
    F = sfft.fft2(I - dt(1), norm='ortho')
    num = (w * F).sum(axis=0)
    den = (dt(2) * w ** 2).sum(axis=0) + np.asarray(ALPHA if alpha is None else alpha, dtype=dt)
    return sfft.ifft2(num / den, norm='ortho').real.astype(dt)


def drive(data, delta0, beta0, dists_cm, lg_kappa, energy_ev, psize_cm, n_epochs=1, learning_rate=1e-3,
          ctf_lg_kappa_learning_rate=1e-3, raw_data_type='intensity', dtype=np.float64, kappa_dtype=np.float32):
    """ctf_ref.reconstruct(optimize_ctf_lg_kappa=True) with update_using_external_algorithm='ctf' (ptychography.py:1135-1163):
    per minibatch (1) Adam on the object from the gradient at the object and kappa the minibatch began with, (2) -- constraints:
    none here --, (3) delta = retrieve(data, dists, lg_kappa as it is BEFORE this minibatch's kappa step), (4) Adam on lg_kappa
    from the same gradient evaluation.  The losses are those the minibatches began with.  ``kappa_dtype``: float32 as the GPU
    driver keeps it.  Returns dict(obj, losses, lg_kappa_trace, first_delta (after the first minibatch))."""
    dt = np.dtype(dtype)
    obj = np.stack([delta0, beta0], -1).astype(dt)
    m, v = np.zeros_like(obj), np.zeros_like(obj)
    k = np.array([lg_kappa], dtype=kappa_dtype)
    km, kv = np.zeros_like(k), np.zeros_like(k)
    losses, trace, first_delta = [], [], None
    for i_epoch in range(n_epochs):
        r = R.forward_adjoint(obj[..., 0], dists_cm, k[0], data, energy_ev, psize_cm, raw_data_type, dt)
        g = np.stack([r['grad_delta'], np.zeros_like(r['grad_delta'])], -1)
        obj, m, v = adam_step(obj, g, m, v, 0, step_size=learning_rate)
        obj = obj.astype(dt)
        obj[..., 0] = retrieve(data, dists_cm, k[0], energy_ev, psize_cm, dtype=dt)
        if first_delta is None:
            first_delta = obj[..., 0].copy()
        k, km, kv = adam_step(k, np.array([r['grad_lg_kappa']], dtype=kappa_dtype), km, kv, 0, step_size=ctf_lg_kappa_learning_rate)
        trace.append(float(k[0]))
        losses.append(r['loss'])
    return dict(obj=obj, losses=losses, lg_kappa=float(k[0]), lg_kappa_trace=trace, first_delta=first_delta)
