"""NumPy restatement of the contrast-transfer-function model of multi-distance holography (forward_algorithm='ctf':
adorym/forward_model.py:1011-1014, adorym/propagate.py:467-476, 590-606), of its loss, of the closed-form gradients w.r.t. delta
and lg_kappa, and of the driver loop around them.  fp64, and fp32 with the roundings of the reference's float32 run: the factor
PI * lambda_nm * dist_nm is a Python double that meets a float32 tensor (rounded once), u^2 + v^2 is a float32 tensor, 1 / kappa
is formed in double (ctf_lg_kappa stays float64) and rounded once, the transforms run in complex64.

It serves the fields too large for golden F26 (tests/test_ctf_ref_vs_golden.py holds it to the golden where both exist).
Deviation from the reference, as the kernels have it: a pixel with I_d <= 0 predicts 0 and contributes to no gradient (the
reference's autograd returns NaN for every gradient then)."""
import numpy as np
import scipy.fft as sfft

from oracle.adorym_oracle import adam_step

PI = 3.14159265359          # adorym/constants.py:90
LN10 = 2.302585092994045684


def uv2(shape, psize_cm, dtype=np.float64):
    """u^2 + v^2 of gen_freq_mesh (adorym/propagate.py:54-60), the mesh cast to ``dtype`` before squaring like the tensors."""
    voxel_nm = psize_cm * 1e7
    u = (np.fft.fftfreq(shape[0]) / voxel_nm).astype(dtype)
    v = (np.fft.fftfreq(shape[1]) / voxel_nm).astype(dtype)
    return u[:, None] ** 2 + v[None, :] ** 2


def xi_sincos(shape, dists_cm, energy_ev, psize_cm, dtype=np.float64):
    """sin xi_d, cos xi_d  [n_dists, ny, nx]"""
    dt = np.dtype(dtype).type
    lmbda_nm = 1240. / energy_ev
    q = uv2(shape, psize_cm, dt)
    xi = np.stack([dt(PI * lmbda_nm * (float(d) * 1e7)) * q for d in np.asarray(dists_cm, dtype=np.float64).reshape(-1)])
    return np.sin(xi), np.cos(xi)


def osc(sn, cs, lg_kappa, dtype=np.float64):
    dt = np.dtype(dtype).type
    return dt(2) * (sn + dt(1. / 10. ** float(lg_kappa)) * cs)


def apply(o, field):
    """Re IFFT2(o FFT2(field)) per distance: the model's linear operator A_d (real, symmetric)."""
    F = sfft.fft2(field)
    return sfft.ifft2(o * F).real.astype(field.dtype)


def target(data, raw_data_type='intensity'):
    a = np.abs(data)
    return np.sqrt(a) if raw_data_type == 'intensity' else a


def forward_adjoint(delta, dists_cm, lg_kappa, data, energy_ev, psize_cm, raw_data_type='intensity', dtype=np.float64, want_grad=True):
    """delta [ny, nx], data [n_dists, ny, nx] (raw).  Returns dict(I, pred, loss, loss_d (per-distance sums of squares), grad_delta,
    grad_lg_kappa)."""
    dt = np.dtype(dtype).type
    D = np.asarray(delta, dtype=dt)
    nd, n = len(data), D.size
    sn, cs = xi_sincos(D.shape, dists_cm, energy_ev, psize_cm, dt)
    o = osc(sn, cs, lg_kappa, dt)
    F = sfft.fft2(D)
    I = (dt(1) + sfft.ifft2(o * F).real).astype(dt)
    pos = I > 0
    pred = np.sqrt(np.where(pos, I, dt(0))).astype(dt)
    diff = pred - target(np.asarray(data, dtype=dt), raw_data_type)
    loss_d = (diff.astype(np.float64) ** 2).sum(axis=(1, 2))
    out = dict(I=I, pred=pred, loss=float(loss_d.sum() / (nd * n)), loss_d=loss_d)
    if not want_grad:
        return out
    with np.errstate(divide='ignore', invalid='ignore'):
        q = np.where(pos, diff / (pred * dt(nd * n)), dt(0)).astype(dt)
    Q = sfft.fft2(q)
    out['q'] = q
    out['grad_delta'] = sfft.ifft2((o * Q).sum(axis=0)).real.astype(dt)
    s = (np.conj(Q).astype(np.complex128) * cs * F).real.sum()
    out['grad_lg_kappa'] = float(-(2. * LN10 / 10. ** float(lg_kappa)) / n * s)
    return out


def reconstruct(data, delta0, beta0, dists_cm, lg_kappa, energy_ev, psize_cm, n_epochs=1, learning_rate=1e-3,
                optimize_ctf_lg_kappa=False, ctf_lg_kappa_learning_rate=1e-3, other_params_update_delay=0,
                raw_data_type='intensity', dtype=np.float64, kappa_dtype=np.float64):
    """The driver loop for multi-distance data of one undivided tile (two_d_mode, minibatch 1: one minibatch per epoch, so the
    object's Adam step counter is 0 in every epoch, ptychography.py:848) -- Adam on the object (the beta channel sees a zero
    gradient and does not move) and, from minibatch ``other_params_update_delay`` on, plain Adam on ctf_lg_kappa
    (optimizers.py:945-956, 1077-1083).  ``kappa_dtype``: float64 as the reference keeps it, float32 as the GPU driver does."""
    dt = np.dtype(dtype)
    obj = np.stack([delta0, beta0], -1).astype(dt)
    m, v = np.zeros_like(obj), np.zeros_like(obj)
    k = np.array([lg_kappa], dtype=kappa_dtype)
    km, kv = np.zeros_like(k), np.zeros_like(k)
    losses, trace, first_grad = [], [], None
    for i_epoch in range(n_epochs):
        r = forward_adjoint(obj[..., 0], dists_cm, k[0], data, energy_ev, psize_cm, raw_data_type, dt)
        g = np.stack([r['grad_delta'], np.zeros_like(r['grad_delta'])], -1)
        if first_grad is None:
            first_grad = g.copy()
        obj, m, v = adam_step(obj, g, m, v, 0, step_size=learning_rate)
        if optimize_ctf_lg_kappa and i_epoch >= other_params_update_delay:
            k, km, kv = adam_step(k, np.array([r['grad_lg_kappa']], dtype=kappa_dtype), km, kv, 0, step_size=ctf_lg_kappa_learning_rate)
        trace.append(float(k[0]))
        losses.append(r['loss'])
    return dict(obj=obj, losses=losses, lg_kappa=float(k[0]), lg_kappa_trace=trace, first_grad=first_grad)
