"""NumPy restatement of the CTF model of multi-distance holography with the distances as parameters (optimize_free_prop under
forward_algorithm='ctf': adorym/propagate.py:467-476, 590-606 with free_prop_cm a tensor that requires grad) and with the affine
registration of the holograms in front of the loss (optimize_prj_affine: adorym/forward_model.py:1066-1072), on top of
tests/ctf_ref.py (unchanged) and tests/multidist3d_affine_ref.py.

    dL/dd_d [per cm] = (2 PI lambda_nm 1e7 / n) sum_k (cos xi_d - sin xi_d / kappa) (u^2 + v^2)(k) Re(conj(Q_d(k)) F(k))

fp64, and float32 with the roundings of the reference's float32 run when free_prop_cm is a float32 tensor:
    dist_nm = free_prop_cm * 1e7                      a float32 product
    PI * lmbda_nm * dist_nm                           the Python double PI * lmbda_nm meets the 0-dim float32 tensor as a float32 scalar
so c_d = fl32(fl32(PI lambda_nm) * fl32(d * 1e7)) (tests/ctf_ref.py rounds the double product once: distances from the host), and
the gradient follows autograd's float32 chain: dL/dosc, dL/dxi, the sum over the frequencies, then the two scalar factors.
Callers hand in distances that float32 holds exactly (``round32``, ``model_dists``): the reference pair and the kernels see the same
numbers.
"""
import numpy as np
import scipy.fft as sfft

from oracle.adorym_oracle import adam_step
from tests import ctf_ref as R
from tests import multidist3d_affine_ref as AR

PI, LN10 = R.PI, R.LN10


def round32(d):
    return np.asarray(d, dtype=np.float32).astype(np.float64).reshape(-1)


def model_dists(d):
    """The table's model distances: d (1 + 0.1 cos(1.3 i + 2.9)) rounded to float32 (the data are made at d)."""
    d = np.asarray(d, dtype=np.float64).reshape(-1)
    return round32(d * (1. + 0.1 * np.cos(1.3 * np.arange(d.size) + 2.9)))


def c_of(dists_cm, energy_ev, dtype=np.float64):
    """c_d = PI lambda_nm dist_nm_d of distances in cm, [n_dists] in ``dtype`` (float32: the distances are rounded to it first)."""
    lmbda_nm = 1240. / energy_ev
    d = np.asarray(dists_cm, dtype=np.float64).reshape(-1)
    if np.dtype(dtype) == np.float64:
        return PI * lmbda_nm * (d * 1e7)
    return np.float32(PI * lmbda_nm) * (d.astype(np.float32) * np.float32(1e7))


def forward_adjoint(delta, dists_cm, lg_kappa, data, energy_ev, psize_cm, raw_data_type='intensity', dtype=np.float64, target=None):
    """delta [ny, nx], data [n_dists, ny, nx] (raw), dists_cm [n_dists].  ``target`` [n_dists, ny, nx]: the
    registered targets, used in place of ctf_ref.target(data).  Returns dict(I, pred, loss, loss_d, q, grad_delta, grad_lg_kappa,
    grad_dists [n_dists] per cm)."""
    dt = np.dtype(dtype).type
    D = np.asarray(delta, dtype=dt)
    nd, n = len(dists_cm), D.size
    q2 = R.uv2(D.shape, psize_cm, dt)
    c = c_of(dists_cm, energy_ev, dt)
    xi = np.stack([cd * q2 for cd in c]).astype(dt)
    sn, cs = np.sin(xi), np.cos(xi)
    ik = dt(1. / 10. ** float(lg_kappa))
    o = dt(2) * (sn + ik * cs)
    F = sfft.fft2(D)
    I = (dt(1) + sfft.ifft2(o * F).real).astype(dt)
    pos = I > 0
    pred = np.sqrt(np.where(pos, I, dt(0))).astype(dt)
    t = R.target(np.asarray(data, dtype=dt), raw_data_type) if target is None else np.asarray(target, dtype=dt)
    diff = pred - t
    loss_d = (diff.astype(np.float64) ** 2).sum(axis=(1, 2))
    with np.errstate(divide='ignore', invalid='ignore'):
        q = np.where(pos, diff / (pred * dt(nd * n)), dt(0)).astype(dt)
    Q = sfft.fft2(q)
    out = dict(I=I, pred=pred, loss=float(loss_d.sum() / (nd * n)), loss_d=loss_d, q=q)
    out['grad_delta'] = sfft.ifft2((o * Q).sum(axis=0)).real.astype(dt)
    out['grad_lg_kappa'] = float(-(2. * LN10 / 10. ** float(lg_kappa)) / n * (np.conj(Q).astype(np.complex128) * cs * F).real.sum())
    # autograd's chain in ``dtype``: dL/dosc = Re(conj(Q) F) / n, dL/dxi = dL/dosc 2 (cos - sin / kappa), dL/dc = sum dL/dxi (u^2 + v^2)
    g_osc = ((Q.real * F.real + Q.imag * F.imag) / dt(n)).astype(dt)
    g_xi = (g_osc * (dt(2) * (cs - ik * sn))).astype(dt)
    g_c = (g_xi * q2).sum(axis=(1, 2), dtype=dt)
    out['grad_dists'] = np.asarray(g_c * dt(PI * (1240. / energy_ev)) * dt(1e7), dtype=np.float64)
    return out


def central_differences(delta, dists_cm, lg_kappa, data, energy_ev, psize_cm, raw_data_type='intensity', rel_step=1e-4, target=None):
    """dL/dd_d by central differences of ctf_ref's fp64 loss at a step of rel_step * d."""
    d = np.asarray(dists_cm, dtype=np.float64).reshape(-1)
    out = np.zeros(d.size)
    for i in range(d.size):
        ls = []
        for s in (1., -1.):
            dd = d.copy()
            dd[i] += s * rel_step * d[i]
            if target is None:
                ls.append(R.forward_adjoint(delta, dd, lg_kappa, data, energy_ev, psize_cm, raw_data_type, want_grad=False)['loss'])
            else:      # (ctf_ref forms its own target: magnitudes go in as magnitude data)
                ls.append(R.forward_adjoint(delta, dd, lg_kappa, target, energy_ev, psize_cm, 'magnitude', want_grad=False)['loss'])
        out[i] = (ls[0] - ls[1]) / (2 * rel_step * d[i])
    return out


def registered(delta, dists_cm, lg_kappa, data, theta, energy_ev, psize_cm, raw_data_type='intensity', dtype=np.float64):
    """The same with the holograms registered by theta [n_dists, 2, 3] in front of the loss; adds 'target' and 'grad_theta'."""
    _, tgt = AR.register(data, theta, raw_data_type, dtype)
    out = forward_adjoint(delta, dists_cm, lg_kappa, data, energy_ev, psize_cm, raw_data_type, dtype, target=tgt)
    out['target'] = tgt
    out['grad_theta'] = AR.affine_grad(data, theta, out['pred'], raw_data_type, dtype)
    return out


def reconstruct(data, delta0, beta0, dists_cm, lg_kappa, energy_ev, psize_cm, n_epochs=1, learning_rate=1e-3, optimize_free_prop=False,
                free_prop_learning_rate=1e-3, optimize_prj_affine=False, prj_affine_learning_rate=1e-3, optimize_ctf_lg_kappa=False,
                ctf_lg_kappa_learning_rate=1e-3, raw_data_type='intensity', dtype=np.float64, small_dtype=None):
    """ctf_ref.reconstruct's loop (one minibatch per epoch, every Adam step counter 0) with plain Adam on the distances and on the
    registration matrices, matrix 0 pinned to the identity after every step (optimizers.py:905-943).  ``small_dtype``: the type the
    small parameters live in (the reference: ``dtype``; the GPU driver: float32).  Returns obj, losses, the distances and matrices
    after every update (dists_trace [n_epochs, D], theta_trace [n_epochs, D, 2, 3]) and the kappa trace."""
    dt = np.dtype(dtype)
    sd = np.dtype(small_dtype or dtype)
    obj = np.stack([delta0, beta0], -1).astype(dt)
    m, v = np.zeros_like(obj), np.zeros_like(obj)
    d = round32(dists_cm).astype(sd)
    nd = d.size
    th = np.tile(AR.IDENTITY, (nd, 1, 1)).astype(sd)
    k = np.array([lg_kappa], dtype=sd)
    mom = {n: [np.zeros_like(x), np.zeros_like(x)] for n, x in (('d', d), ('th', th), ('k', k))}
    losses, d_tr, th_tr, k_tr = [], [], [], []
    for _ in range(n_epochs):
        if optimize_prj_affine:
            r = registered(obj[..., 0], d, k[0], data, th, energy_ev, psize_cm, raw_data_type, dt)
        else:
            r = forward_adjoint(obj[..., 0], d, k[0], data, energy_ev, psize_cm, raw_data_type, dt)
        g = np.stack([r['grad_delta'], np.zeros_like(r['grad_delta'])], -1)
        obj, m, v = adam_step(obj, g, m, v, 0, step_size=learning_rate)
        if optimize_free_prop:
            d, mom['d'][0], mom['d'][1] = adam_step(d, r['grad_dists'].astype(sd), mom['d'][0], mom['d'][1], 0, step_size=free_prop_learning_rate)
        if optimize_prj_affine:
            th, mom['th'][0], mom['th'][1] = adam_step(th, np.asarray(r['grad_theta']).astype(sd), mom['th'][0], mom['th'][1], 0,
                                                       step_size=prj_affine_learning_rate)
            th[0] = AR.IDENTITY
        if optimize_ctf_lg_kappa:
            k, mom['k'][0], mom['k'][1] = adam_step(k, np.array([r['grad_lg_kappa']], dtype=sd), mom['k'][0], mom['k'][1], 0,
                                                    step_size=ctf_lg_kappa_learning_rate)
        losses.append(r['loss'])
        d_tr.append(np.asarray(d, np.float64).copy())
        th_tr.append(np.asarray(th, np.float64).copy())
        k_tr.append(float(k[0]))
    return dict(obj=obj, losses=losses, dists_trace=np.array(d_tr), theta_trace=np.array(th_tr), lg_kappa_trace=k_tr)


def reconstruct_tomo(prj, obj0, dists_cm, lg_kappa, theta_ls, energy_ev, psize_cm, n_epochs=1, learning_rate=1e-3, optimize_free_prop=False,
                     free_prop_learning_rate=1e-3, optimize_prj_affine=False, prj_affine_learning_rate=1e-3, optimize_ctf_lg_kappa=False,
                     ctf_lg_kappa_learning_rate=1e-3, raw_data_type='intensity', dtype=np.float64, small_dtype=None):
    """The same driver loop for a 3-D object (CTF holotomography): prj [n_theta, D, Y, X], obj0 [Y, X, Z, 2]; a minibatch is one
    angle with all its distances, in the order of the reference's epoch task list; the rotated object summed along the beam
    (tests/ctf_tomo_ref.project) is the model's one slice and its gradient is back-projected; the Adam step counter of the object
    and of every small parameter counts the angles of the epoch (the control flow of tests/multidist3d_ref.reconstruct).  Returns
    obj, losses and the distances, matrices and kappa after every update."""
    from oracle import adorym_oracle as O
    from tests import ctf_tomo_ref as TR
    dt = np.dtype(dtype)
    sd = np.dtype(small_dtype or dtype)
    obj = np.asarray(obj0).astype(dt)
    Z = obj.shape[2]
    m, v = np.zeros_like(obj), np.zeros_like(obj)
    d = round32(dists_cm).astype(sd)
    th = np.tile(AR.IDENTITY, (d.size, 1, 1)).astype(sd)
    k = np.array([lg_kappa], dtype=sd)
    mom = {n: [np.zeros_like(x), np.zeros_like(x)] for n, x in (('d', d), ('th', th), ('k', k))}
    tables, losses, d_tr, th_tr, k_tr = {}, [], [], [], []
    for i_epoch in range(n_epochs):
        batches = O.epoch_task_list(i_epoch, len(theta_ls), 1, 1, 1, 'immediate')
        for i_opt in range(len(batches)):
            i_theta, _ = O.rank_batch(batches, i_opt, 0, 1, 1)
            if i_theta not in tables:
                tables[i_theta] = O.rotation_coords(obj.shape[:3], np.float32(theta_ls[i_theta]))
            p = TR.project(obj, tables[i_theta], dt)
            if optimize_prj_affine:
                r = registered(p[..., 0], d, k[0], prj[i_theta], th, energy_ev, psize_cm, raw_data_type, dt)
            else:
                r = forward_adjoint(p[..., 0], d, k[0], prj[i_theta], energy_ev, psize_cm, raw_data_type, dt)
            g = TR.backproject(np.stack([r['grad_delta'], np.zeros_like(r['grad_delta'])], -1), tables[i_theta], Z, dt)
            obj, m, v = adam_step(obj, g.astype(dt), m, v, i_opt, step_size=learning_rate)
            if optimize_free_prop:
                d, mom['d'][0], mom['d'][1] = adam_step(d, r['grad_dists'].astype(sd), mom['d'][0], mom['d'][1], i_opt,
                                                        step_size=free_prop_learning_rate)
            if optimize_prj_affine:
                th, mom['th'][0], mom['th'][1] = adam_step(th, np.asarray(r['grad_theta']).astype(sd), mom['th'][0], mom['th'][1], i_opt,
                                                           step_size=prj_affine_learning_rate)
                th[0] = AR.IDENTITY
            if optimize_ctf_lg_kappa:
                k, mom['k'][0], mom['k'][1] = adam_step(k, np.array([r['grad_lg_kappa']], dtype=sd), mom['k'][0], mom['k'][1], i_opt,
                                                        step_size=ctf_lg_kappa_learning_rate)
            losses.append(r['loss'])
            d_tr.append(np.asarray(d, np.float64).copy())
            th_tr.append(np.asarray(th, np.float64).copy())
            k_tr.append(float(k[0]))
    return dict(obj=obj, losses=losses, dists_trace=np.array(d_tr), theta_trace=np.array(th_tr), lg_kappa_trace=k_tr)
