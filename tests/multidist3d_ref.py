"""NumPy restatement of the reference's multi-distance holography of a 3-D object (test infrastructure only: the checker, never
the product).

  MultiDistModel.predict, one undivided field of view   adorym/forward_model.py:905-914, 971-1019
  fresnel_propagate behind multislice_propagate_batch   adorym/propagate.py:282-288, 537-553
  the loss over all distances                           adorym/forward_model.py:1056-1061, 1090

built on the pinned oracle (oracle/adorym_oracle.py).  The reference runs multislice_propagate_batch once per distance on the same
tiles; the field behind the last slice does not depend on the distance, so that is one sweep and D free-space steps,

    Psi_d = IFFT2(H_d FFT2(Psi_S)),   pred[b, d] = sqrt(sum_m |Psi_d,m|^2),   loss = mean over B * D * (kept pixels),

which is the oracle's Fresnel detector on every tile listed D times in a row with ``phys.h_free`` set to the per-entry kernels
[B * D, Py, Px] (it broadcasts through _detector_fwd / _detector_adj unchanged).  Entries are position-major: b * D + d.  The tile
gradient of a position is the sum over its D entries, the probe gradient the sum over all entries.
"""
import copy

import numpy as np

from oracle import adorym_oracle as O


def fanout_physics(phys, dists_cm, batch):
    """``phys`` (any detector) with the detector step replaced by the Fresnel kernels of ``dists_cm``, one per entry b * D + d."""
    hs = np.stack([O.get_kernel(float(d) * 1e7, phys.lmbda_nm, phys.voxel_nm, phys.probe_size, sign_convention=phys.sigma) for d in dists_cm])
    q = copy.copy(phys)
    q.det_mode = 'fresnel'
    q.h_free = np.tile(hs, (batch, 1, 1))
    return q


def forward_adjoint_tiles(tiles, probes, meas, phys, dists_cm, dtype='float64', **loss_kw):
    """tiles [B,Py,Px,S,2], meas [B*D,Py,Px] position-major.  Returns loss, pred [B*D,Py,Px], grad_tiles [B,Py,Px,S,2] and
    grad_probes complex [M,Py,Px] (O.forward_adjoint_tiles; ``loss_kw``: its loss arguments and ``beamstop``)."""
    B, D = tiles.shape[0], len(dists_cm)
    q = fanout_physics(phys, dists_cm, B)
    loss, pred, gt, gp = O.forward_adjoint_tiles(np.repeat(tiles, D, axis=0), probes, meas, q, dtype, **loss_kw)
    return loss, pred, gt.reshape((B, D) + gt.shape[1:]).sum(axis=1), gp


def predict(tiles, probes, phys, dists_cm, dtype='float64'):
    B, D = tiles.shape[0], len(dists_cm)
    return O.predict(np.repeat(tiles, D, axis=0), probes, fanout_physics(phys, dists_cm, B), dtype)[0]


def forward_adjoint_object(obj, coords_fp16, probes, pos_batch, meas, phys, dists_cm, dtype='float64', **loss_kw):
    """Rotate, cut the tiles, evaluate, scatter, rotate back.  Returns loss, pred [B*D,Py,Px], the object gradient [Y,X,S,2] and
    the probe gradient."""
    dt = np.dtype(dtype)
    obj = obj.astype(dt, copy=False)
    rot = O.rotate_fwd(obj, coords_fp16, dt) if coords_fp16 is not None else obj
    tiles, _ = O.extract_tiles(rot, pos_batch, phys.probe_size, phys.unknown_type)
    loss, pred, gt, gp = forward_adjoint_tiles(tiles, probes, meas, phys, dists_cm, dt, **loss_kw)
    g = O.scatter_tiles_adj(gt, pos_batch, obj.shape)
    if coords_fp16 is not None:
        g = O.rotate_adj(g, coords_fp16, dt)
    return loss, pred, g, gp


def reconstruct(prj, obj_init, probe, phys, dists_cm, theta_ls, n_epochs=1, learning_rate=1e-3, raw_data_type='magnitude',
                dtype='float64'):
    """reconstruct_ptychography on multi-distance data of a 3-D object, one undivided field of view ('immediate' updates, Adam on
    the object, no regulariser, one rank): prj [n_theta, D, Y, X]; a minibatch is one angle with all its distances.  The control
    flow of O.reconstruct.  Returns obj [Y,X,Z,2] and every loss."""
    dt = np.dtype(dtype)
    obj = np.stack([obj_init[0], obj_init[1]], -1).astype(dt)
    m, v = np.zeros_like(obj), np.zeros_like(obj)
    pc = np.asarray(probe).astype(O._cdtype(dt))
    n_theta = len(theta_ls)
    pos = np.zeros((1, 2), int)
    tables, losses = {}, []
    for i_epoch in range(n_epochs):
        batches = O.epoch_task_list(i_epoch, n_theta, 1, 1, 1, 'immediate')
        i_opt = 0
        for i_batch in range(len(batches)):
            i_theta, _ = O.rank_batch(batches, i_batch, 0, 1, 1)
            if i_theta not in tables:
                tables[i_theta] = O.rotation_coords(obj.shape[:3], theta_ls[i_theta], dt)
            loss, _, g, _ = forward_adjoint_object(obj, tables[i_theta], pc, pos, np.abs(prj[i_theta]), phys, dists_cm, dt,
                                                   raw_data_type=raw_data_type)
            losses.append(float(loss))
            obj, m, v = O.adam_step(obj, g.astype(dt), m, v, i_opt, step_size=learning_rate)
            last_of_theta = i_batch == len(batches) - 1 or int(batches[i_batch + 1][0, 0]) != int(batches[i_batch][0, 0])
            if last_of_theta:
                i_opt += 1
    return dict(obj=obj, losses=losses)
