"""NumPy restatement of the reference's per-angle projection alignment (test infrastructure only: the checker, never the product).

  shift_exit_wave in multislice_propagate_batch   adorym/propagate.py:260-261
  realign_image_fourier                           adorym/util.py:380-397
  the prj_pos_offset optimiser                    adorym/optimizers.py:863-875, 1135-1138

built on the pinned oracle (oracle/adorym_oracle.py).  Position b carries the offset s_b = shifts[index[b]] = (s_y, s_x); the field
behind the last slice is Fourier-shifted by it before the free-space step.  The reference runs shift and propagation as two
transform pairs; one pair with the product is the same mathematics:

    Psi_det = IFFT2(Phi_b H_free FFT2(Psi_S)),   Phi_b = exp(-2 PI i (fx s_x + fy s_y)),   H_free = 1 for an exit-wave detector,

which is the oracle's Fresnel detector with ``phys.h_free`` set to the per-position product [B, Py, Px] (it broadcasts through
_detector_fwd / _detector_adj unchanged).  A far-field magnitude does not depend on the shift: nothing is applied and the gradient
is zero.  With G = dL/dRe + i dL/dIm at the detector plane, Ghat = FFT2(G) / (Py Px) and W = Phi_b H_free FFT2(Psi_S):

    dL/ds_y = 2 PI sum_k fy_k Im(conj(Ghat_k) W_k),   dL/ds_x the same with fx_k,

summed over the probe modes and over the positions that share an entry.
"""
import copy

import numpy as np

from oracle import adorym_oracle as O
from tests.sparse_ref import masked_loss

PI = O.PI


def shifted_physics(phys, shifts_b, dtype='float64'):
    """``phys`` with the detector step replaced by the per-position product Phi_b * H_free; None for a far-field detector."""
    if phys.det_mode == 'far':
        return None
    dt = np.dtype(dtype)
    cdt = O._cdtype(dt)
    phi = np.stack([O.fourier_shift_phase(phys.probe_size, s, dt) for s in shifts_b])
    q = copy.copy(phys)
    q.h_free = (phi * phys.h_free_cast(dt)[None]).astype(cdt) if phys.det_mode == 'fresnel' else phi
    q.det_mode = 'fresnel'
    return q


def forward_adjoint_tiles(tiles, probes, meas, phys, shifts, index=None, dtype='float64', raw_data_type='magnitude',
                          loss_function_type='lsq', poisson_multiplier=1., beamstop=None):
    """Loss, prediction [B,Py,Px], grad_tiles [B,Py,Px,S,2], grad_probes complex [M,Py,Px] (O.forward_adjoint_tiles, its loss
    arguments and ``beamstop`` included) and dL/dshifts [n_entries, 2].  ``shifts`` [n_entries, 2] = (s_y, s_x); ``index`` [B] or None = b."""
    dt = np.dtype(dtype)
    cdt = O._cdtype(dt)
    probes = np.asarray(probes)
    if probes.ndim == 2:
        probes = probes[None]
    shifts = np.asarray(shifts, dtype=np.float64).reshape(-1, 2)
    B, Py, Px = tiles.shape[:3]
    index = np.arange(B) if index is None else np.asarray(index).astype(int)
    q = shifted_physics(phys, shifts[index], dt)
    gs = np.zeros(shifts.shape, dtype=dt)
    loss_kw = dict(raw_data_type=raw_data_type, loss_function_type=loss_function_type, poisson_multiplier=poisson_multiplier,
                   beamstop=beamstop)
    if q is None:
        return O.forward_adjoint_tiles(tiles, probes, meas, phys, dt, **loss_kw) + (gs,)
    loss, pred, gt, gp = O.forward_adjoint_tiles(tiles, probes, meas, q, dt, **loss_kw)
    # the shift gradient: the exit waves once more (the oracle does not hand them out), then the sums above
    bare = copy.copy(phys)
    bare.det_mode, bare.h_free = 'none', None
    dldp = masked_loss(pred, np.asarray(meas).astype(dt, copy=False), dt, loss_function_type, raw_data_type, poisson_multiplier, beamstop)[1]
    fy = np.fft.fftfreq(Py, 1).astype(dt)[:, None]
    fx = np.fft.fftfreq(Px, 1).astype(dt)[None, :]
    hq = q.h_free_cast(dt)
    for p in probes:
        W = (np.fft.fft2(O.multislice_forward(tiles, p, bare, dt)).astype(cdt) * hq).astype(cdt)
        f = np.fft.ifft2(W).astype(cdt)
        with np.errstate(divide='ignore', invalid='ignore'):
            unit = np.where(pred > 0, f / pred, 0) if len(probes) == 1 else f / pred
        Gh = (np.fft.fft2((dldp * unit).astype(cdt)) / dt.type(Py * Px)).astype(cdt)
        t = np.imag(np.conj(Gh) * W).astype(dt)
        gb = np.stack([(t * fy).sum(axis=(1, 2)), (t * fx).sum(axis=(1, 2))], -1) * dt.type(2 * PI)
        np.add.at(gs, index, gb.astype(dt))
    return loss, pred, gt, gp, gs


def predict(tiles, probes, phys, shifts, index=None, dtype='float64'):
    B = tiles.shape[0]
    shifts = np.asarray(shifts, dtype=np.float64).reshape(-1, 2)
    index = np.arange(B) if index is None else np.asarray(index).astype(int)
    q = shifted_physics(phys, shifts[index], dtype)
    return O.predict(tiles, probes, q if q is not None else phys, dtype)[0]


def forward_adjoint_object(obj, coords_fp16, probes, pos_batch, meas, phys, shifts, index=None, dtype='float64', raw_data_type='magnitude',
                           loss_function_type='lsq', poisson_multiplier=1., beamstop=None):
    """O.forward_adjoint_object with the offsets: rotate, cut tiles, evaluate, scatter, rotate back.  Returns loss, pred, the object
    gradient [Y,X,S,2], the probe gradient and dL/dshifts."""
    dt = np.dtype(dtype)
    obj = obj.astype(dt, copy=False)
    rot = O.rotate_fwd(obj, coords_fp16, dt) if coords_fp16 is not None else obj
    tiles, _ = O.extract_tiles(rot, pos_batch, phys.probe_size, phys.unknown_type)
    loss, pred, gt, gp, gs = forward_adjoint_tiles(tiles, probes, meas, phys, shifts, index, dt, raw_data_type=raw_data_type,
                                                   loss_function_type=loss_function_type, poisson_multiplier=poisson_multiplier, beamstop=beamstop)
    g = O.scatter_tiles_adj(gt, pos_batch, obj.shape)
    if coords_fp16 is not None:
        g = O.rotate_adj(g, coords_fp16, dt)
    return loss, pred, g, gp, gs


def reconstruct(prj, obj_init, probes, probe_pos, phys, theta_ls, n_epochs=1, minibatch_size=1, learning_rate=1e-3,
                raw_data_type='magnitude', optimize_object=True, prj_pos_offset_learning_rate=1e-2, offset_optimizer='gd',
                offsets_init=None, other_params_update_delay=0, n_ranks=1, dtype='float64'):
    """reconstruct_ptychography with optimize_prj_pos_offset ('immediate' updates, Adam on the object, no regulariser): the control
    flow of O.reconstruct with prj_pos_offset [n_theta, 2] as one more small parameter -- every minibatch uses the entry of its
    angle, the gradients are summed over the ranks, and from global minibatch ``other_params_update_delay`` on the WHOLE array
    takes a step (optimizers.py:1077-1083): plain gradient descent with a constant step (the default, optimizers.py:863-875) or
    Adam.  Returns obj, offsets, losses (rank 0's), offset_history (the offsets after every update)."""
    dt = np.dtype(dtype)
    cdt = O._cdtype(dt)
    obj = np.stack([obj_init[0], obj_init[1]], -1).astype(dt)
    m, v = np.zeros_like(obj), np.zeros_like(obj)
    probes = np.asarray(probes)
    if probes.ndim == 2:
        probes = probes[None]
    pc = probes.astype(cdt)
    n_theta = len(theta_ls)
    off = np.zeros((n_theta, 2), dtype=dt) if offsets_init is None else np.asarray(offsets_init).astype(dt)
    om, ov = np.zeros_like(off), np.zeros_like(off)
    pos_int = np.round(np.asarray(probe_pos, dtype=float)).astype(int)
    n_pos = len(pos_int)
    tables, losses, hist = {}, [], []
    for i_epoch in range(n_epochs):
        batches = O.epoch_task_list(i_epoch, n_theta, n_pos, minibatch_size, n_ranks, 'immediate')
        n_batch = len(batches)
        i_opt = 0
        for i_batch in range(n_batch):
            g_sum = go_sum = None
            for rank in range(n_ranks):
                i_theta, ind = O.rank_batch(batches, i_batch, rank, minibatch_size, n_ranks)
                if i_theta not in tables:
                    tables[i_theta] = O.rotation_coords(obj.shape[:3], theta_ls[i_theta], dt)
                loss, _, g, _, go = forward_adjoint_object(obj, tables[i_theta], pc, pos_int[ind], np.abs(prj[i_theta, ind]), phys, off,
                                                           np.full(len(ind), i_theta), dt, raw_data_type=raw_data_type)
                if rank == 0:
                    losses.append(float(loss))
                g_sum = g if g_sum is None else g_sum + g
                go_sum = go if go_sum is None else go_sum + go
            i_global = i_batch + i_epoch * n_batch
            if optimize_object:
                obj, m, v = O.adam_step(obj, g_sum.astype(dt), m, v, i_opt, step_size=learning_rate)
            if i_global >= other_params_update_delay:
                if offset_optimizer == 'gd':
                    off = O.gd_step(off, go_sum.astype(dt), i_opt, step_size=prj_pos_offset_learning_rate, dynamic_rate=False).astype(dt)
                else:
                    off, om, ov = O.adam_step(off, go_sum.astype(dt), om, ov, i_opt, step_size=prj_pos_offset_learning_rate)
                hist.append(off.copy())
            last_of_theta = i_batch == n_batch - 1 or int(batches[i_batch + 1][0, 0]) != int(batches[i_batch][0, 0])
            if last_of_theta:
                i_opt += 1
    return dict(obj=obj, offsets=off, losses=losses, offset_history=np.array(hist))


# the recovery problem shared by the CPU and GPU tests: a 16^3 object known exactly, full field, 4 angles, data from TRUE offsets of
# +-0.5 px; only the offsets move.  RECOVERY_STEP: chosen on the CPU (tests/test_prj_offset_ref_vs_golden.py) so that this
# restatement's own gradient descent is within 0.02 px of the truth after 40 updates
RECOVERY = dict(N=16, n_theta=4, free_prop_cm=2e-4, energy_ev=8000., psize_cm=1e-6, n_epochs=10, step=25.,
                true_offsets=[[0.5, -0.5], [-0.5, 0.5], [0.5, 0.5], [-0.5, -0.5]])


def recovery_inputs(smooth_field):
    """``smooth_field``: tests/golden/cases.py:smooth_field.  Returns truth [N,N,N,2], the probe, theta_ls, phys and the data
    [n_theta, 1, N, N] (fp64)."""
    R = RECOVERY
    N, n_theta = R['N'], R['n_theta']
    truth = np.stack([4e-3 * (0.2 + smooth_field((N, N, N), 2461)), 4e-4 * (0.2 + smooth_field((N, N, N), 2462))], -1)
    yy, xx = np.mgrid[:N, :N] - N / 2
    probe = (0.6 + 0.4 * np.exp(-(yy ** 2 + xx ** 2) / 60.)) * np.exp(1j * 0.1 * yy / N)
    theta_ls = np.linspace(0, np.pi, n_theta, dtype='float32')
    phys = O.Physics((N, N), R['energy_ev'], R['psize_cm'], free_prop_cm=R['free_prop_cm'])
    prj = np.zeros((n_theta, 1, N, N))
    for it, th in enumerate(theta_ls):
        rot = O.rotate_fwd(truth, O.rotation_coords((N, N, N), th), 'float64')
        tiles, _ = O.extract_tiles(rot, np.zeros((1, 2), int), (N, N))
        prj[it] = predict(tiles, probe, phys, np.array(R['true_offsets'])[it:it + 1])
    return truth, probe, theta_ls, phys, prj
