"""NumPy restatement of the reference's sparse multislice path (test infrastructure only: the checker, never the product).

  sparse_multislice_propagate_batch   adorym/propagate.py:479-534
  SparseMultisliceModel               adorym/forward_model.py:589-806
  the slice_pos_cm_ls optimiser       adorym/optimizers.py:891-903, 1051-1060

built on the pieces of the pinned oracle (oracle/adorym_oracle.py: modulator, detector, loss, Adam, task lists, rotation).  For a
tile stack [B, Py, Px, S, 2], slice positions z_0 .. z_{S-1} (cm) and one probe set:

    psi <- probe;  for s: psi <- psi * c_s;  if s < S-1: psi <- IFFT2(H_s FFT2(psi)),  H_s = exp(i a d_s),
    d_s = (z_{s+1} - z_s) * 1e7 nm,  a = -sigma PI lambda_nm (u^2 + v^2)            (always the Fresnel approximation)

and, with G the adjoint field arriving at the output of convolution s (dL = Re sum conj(G) d psi), Ghat = FFT2(G) and Psihat'_s
the spectrum that entered the convolution:

    dL/dd_s = -(1 / (Py Px)) sum a_k Im(conj(Ghat_k) H_{s,k} Psihat'_{s,k}),    dL/dz_j = 1e7 (dL/dd_{j-1} - dL/dd_j).

``dtype='float32'`` follows the reference's fp32 tensors: z, the distances, the phase a * d and H are formed in fp32.
"""
import numpy as np

from oracle import adorym_oracle as O

PI = O.PI


def gap_phase_per_nm(phys):
    """a [Py, Px] (fp64): the phase of a gap's transfer function per nm of distance."""
    u, v = O.gen_freq_mesh(phys.voxel_nm, phys.probe_size)
    return -phys.sigma * PI * phys.lmbda_nm * (u ** 2 + v ** 2)


def gap_kernels(phys, z_cm, dtype='float64'):
    """H [S-1, Py, Px] complex and the distances d [S-1] (nm), formed in ``dtype`` like get_kernel_wrapped (propagate.py:84-93)
    from ``slice_pos_cm_ls * 1e7`` (propagate.py:491, 515)."""
    dt = np.dtype(dtype)
    cdt = O._cdtype(dt)
    u, v = O.gen_freq_mesh(phys.voxel_nm, phys.probe_size)
    u, v = u.astype(dt), v.astype(dt)
    z_nm = np.asarray(z_cm).astype(dt) * dt.type(1e7)
    d = (z_nm[1:] - z_nm[:-1]).astype(dt)
    hs = []
    for ds in d:
        ph = ((-phys.sigma * PI * phys.lmbda_nm) * ds).astype(dt) * (u ** 2 + v ** 2)
        hs.append((np.cos(ph) + 1j * np.sin(ph)).astype(cdt))
    return (np.stack(hs) if hs else np.zeros((0,) + tuple(phys.probe_size), cdt)), d


def masked_loss(pred, meas, dtype, loss_function_type='lsq', raw_data_type='magnitude', poisson_multiplier=1., beamstop=None):
    """The loss and dL/dpred exactly as O.forward_adjoint_tiles forms them: with a ``beamstop`` [Py,Px] only the pixels with
    beamstop >= 1e-5 enter the mean, and dL/dpred is zero elsewhere.  pred, meas [N,Py,Px]."""
    if beamstop is None:
        loss = O.mismatch_loss(pred, meas, loss_function_type, raw_data_type, poisson_multiplier)
        return loss, O._dloss_dpred(pred, meas, loss_function_type, raw_data_type, poisson_multiplier).astype(dtype)
    keep = np.asarray(beamstop) >= 1e-5
    loss = O.mismatch_loss(pred[:, keep], meas[:, keep], loss_function_type, raw_data_type, poisson_multiplier)
    dldp = np.zeros_like(pred)
    dldp[:, keep] = O._dloss_dpred(pred[:, keep], meas[:, keep], loss_function_type, raw_data_type, poisson_multiplier)
    return loss, dldp


def forward_adjoint_tiles(tiles, probes, meas, phys, z_cm, dtype='float64', raw_data_type='magnitude', want_grad=True,
                          loss_function_type='lsq', poisson_multiplier=1., beamstop=None):
    """Loss, prediction [B,Py,Px], grad_tiles [B,Py,Px,S,2], grad_probes complex [M,Py,Px] (the conventions of
    O.forward_adjoint_tiles, its loss arguments and ``beamstop`` included) and dL/dz [S] in 1/cm, for slices at ``z_cm``.
    ``phys``: O.Physics with binning 1 (its own slice kernel ``h`` is not used)."""
    dt = np.dtype(dtype)
    cdt = O._cdtype(dt)
    assert phys.binning == 1
    probes = np.asarray(probes)
    if probes.ndim == 2:
        probes = probes[None]
    tiles = tiles.astype(dt, copy=False)
    B, Py, Px, S, _ = tiles.shape
    assert len(z_cm) == S
    H, _ = gap_kernels(phys, z_cm, dt)
    a = gap_phase_per_nm(phys).astype(dt)
    cs = [O._modulator(tiles[:, :, :, s, 0], tiles[:, :, :, s, 1], phys, dt) for s in range(S)]
    fields, kepts, specs = [], [], []
    for p in probes:
        psi = np.broadcast_to(p.astype(cdt), (B, Py, Px)).copy()
        kept, spec = [], []
        for s in range(S):
            psi = (psi * cs[s]).astype(cdt)
            kept.append(psi)
            if s < S - 1:
                sp = np.fft.fft2(psi).astype(cdt)
                spec.append(sp)
                psi = np.fft.ifft2(sp * H[s]).astype(cdt)
        fields.append(O._detector_fwd(psi, phys, dt).astype(cdt))
        kepts.append(kept)
        specs.append(spec)
    pred = np.abs(fields[0]) if len(fields) == 1 else np.sqrt(sum((f.real ** 2 + f.imag ** 2) for f in fields))
    meas = np.asarray(meas).astype(dt, copy=False)
    loss, dldp = masked_loss(pred, meas, dt, loss_function_type, raw_data_type, poisson_multiplier, beamstop)
    if not want_grad:
        return loss, pred
    grad_tiles = np.zeros_like(tiles)
    grad_probes = np.zeros(probes.shape, dtype=cdt)
    gd_gap = np.zeros(max(S - 1, 0), dtype=dt)
    k1, sg = dt.type(phys.k1), dt.type(phys.sigma)
    for m, (f, kept, spec) in enumerate(zip(fields, kepts, specs)):
        with np.errstate(divide='ignore', invalid='ignore'):
            unit = np.where(pred > 0, f / pred, 0) if len(fields) == 1 else f / pred
        G = O._detector_adj((dldp * unit).astype(cdt), phys, dt).astype(cdt)
        for s in range(S - 1, -1, -1):
            if phys.unknown_type == 'real_imag':
                zc = G * np.conj(kept[s] / cs[s])
                gd, gb = zc.real.astype(dt), zc.imag.astype(dt)
            else:
                z = np.conj(G) * kept[s]
                gb = (-k1 * z.real).astype(dt)
                gd = (sg * k1 * z.imag).astype(dt)
            grad_tiles[:, :, :, s, 0] += gd
            grad_tiles[:, :, :, s, 1] += gb
            G = (G * np.conj(cs[s])).astype(cdt)
            if s > 0:
                Gh = np.fft.fft2(G).astype(cdt)
                gd_gap[s - 1] += -(a * np.imag(np.conj(Gh) * H[s - 1] * spec[s - 1])).sum() / dt.type(Py * Px)
                G = np.fft.ifft2(Gh * np.conj(H[s - 1])).astype(cdt)
        grad_probes[m] = G.sum(axis=0)
    gz = np.zeros(S, dtype=dt)
    gz[1:] += gd_gap
    gz[:-1] -= gd_gap
    return loss, pred, grad_tiles, grad_probes, (gz * dt.type(1e7)).astype(dt)


def predict(tiles, probes, phys, z_cm, dtype='float64'):
    return forward_adjoint_tiles(tiles, probes, np.zeros(tiles.shape[:3]), phys, z_cm, dtype, want_grad=False)[1]


def forward_adjoint_object(obj, coords_fp16, probes, pos_batch, meas, phys, z_cm, dtype='float64', raw_data_type='magnitude',
                           loss_function_type='lsq', poisson_multiplier=1., beamstop=None):
    """O.forward_adjoint_object for the sparse model: rotate, cut tiles, evaluate, scatter, rotate back.  Returns loss, pred, the
    object gradient [Y,X,S,2], the probe gradient and dL/dz."""
    dt = np.dtype(dtype)
    obj = obj.astype(dt, copy=False)
    rot = O.rotate_fwd(obj, coords_fp16, dt) if coords_fp16 is not None else obj
    tiles, _ = O.extract_tiles(rot, pos_batch, phys.probe_size, phys.unknown_type)
    loss, pred, gt, gp, gz = forward_adjoint_tiles(tiles, probes, meas, phys, z_cm, dt, raw_data_type=raw_data_type,
                                                   loss_function_type=loss_function_type, poisson_multiplier=poisson_multiplier,
                                                   beamstop=beamstop)
    g = O.scatter_tiles_adj(gt, pos_batch, obj.shape)
    if coords_fp16 is not None:
        g = O.rotate_adj(g, coords_fp16, dt)
    return loss, pred, g, gp, gz


def reconstruct(prj, obj_init, probes, probe_pos, phys, z_cm, theta_ls=None, n_epochs=1, minibatch_size=1, learning_rate=1e-3,
                raw_data_type='magnitude', optimize_probe=False, probe_learning_rate=1e-3, optimize_slice_pos=False,
                slice_pos_learning_rate=1e-4, other_params_update_delay=0, probe_update_delay=0, n_ranks=1, dtype='float64'):
    """reconstruct_ptychography with SparseMultisliceModel ('immediate' updates, Adam everywhere, no regulariser): the control flow
    of O.reconstruct / O.reconstruct_2d with the slice positions as one more small parameter -- gradients summed over the ranks,
    Adam with ``slice_pos_learning_rate`` from global minibatch ``other_params_update_delay`` on, then z <- z - z[0]
    (optimizers.py:1051-1060).  ``theta_ls=None``: two_d_mode.  Returns obj, probes, z, losses (rank 0's), z_history (z after
    every update of it)."""
    dt = np.dtype(dtype)
    cdt = O._cdtype(dt)
    two_d = theta_ls is None
    obj = np.stack([obj_init[0], obj_init[1]], -1).astype(dt)
    m, v = np.zeros_like(obj), np.zeros_like(obj)
    probes = np.asarray(probes)
    if probes.ndim == 2:
        probes = probes[None]
    pst = np.stack([probes.real, probes.imag], -1).astype(dt)
    pm, pv = np.zeros_like(pst), np.zeros_like(pst)
    z = np.asarray(z_cm).astype(dt)
    zm, zv = np.zeros_like(z), np.zeros_like(z)
    pos_int = np.round(np.asarray(probe_pos, dtype=float)).astype(int)
    n_pos, n_theta = len(pos_int), 1 if two_d else len(theta_ls)
    tables, losses, z_hist = {}, [], []
    for i_epoch in range(n_epochs):
        batches = O.epoch_task_list(i_epoch, n_theta, n_pos, minibatch_size, n_ranks, 'immediate', two_d_mode=two_d)
        n_batch = len(batches)
        i_opt = 0
        for i_batch in range(n_batch):
            g_sum = gp_sum = gz_sum = None
            for rank in range(n_ranks):
                i_theta, ind = O.rank_batch(batches, i_batch, rank, minibatch_size, n_ranks)
                coords = None
                if not two_d:
                    if i_theta not in tables:
                        tables[i_theta] = O.rotation_coords(obj.shape[:3], theta_ls[i_theta], dt)
                    coords = tables[i_theta]
                pc = (pst[..., 0] + 1j * pst[..., 1]).astype(cdt)
                loss, _, g, gp, gz = forward_adjoint_object(obj, coords, pc, pos_int[ind], np.abs(prj[i_theta, ind]), phys, z, dt,
                                                            raw_data_type=raw_data_type)
                if rank == 0:
                    losses.append(float(loss))
                gp = np.stack([gp.real, gp.imag], -1).astype(dt)
                g_sum = g if g_sum is None else g_sum + g
                gp_sum = gp if gp_sum is None else gp_sum + gp
                gz_sum = gz if gz_sum is None else gz_sum + gz
            i_global = i_batch + i_epoch * n_batch
            obj, m, v = O.adam_step(obj, g_sum.astype(dt), m, v, i_opt, step_size=learning_rate)
            if optimize_probe and i_global >= probe_update_delay:
                pst, pm, pv = O.adam_step(pst, gp_sum.astype(dt), pm, pv, i_opt, step_size=probe_learning_rate)
            if optimize_slice_pos and i_global >= other_params_update_delay:
                z, zm, zv = O.adam_step(z, gz_sum.astype(dt), zm, zv, i_opt, step_size=slice_pos_learning_rate)
                z = (z - z[0]).astype(dt)
                z_hist.append(z.copy())
            last_of_theta = i_batch == n_batch - 1 or int(batches[i_batch + 1][0, 0]) != int(batches[i_batch][0, 0])
            if last_of_theta:
                i_opt += 1
    return dict(obj=obj, probes=pst[..., 0] + 1j * pst[..., 1], z=z, losses=losses, z_history=np.array(z_hist))
