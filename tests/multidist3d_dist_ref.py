"""NumPy restatement of the reference's multi-distance holography of a 3-D object WITH the distances as parameters
(optimize_free_prop; test infrastructure only: the checker, never the product).

  fresnel_propagate_wrapped behind the slice loop   adorym/propagate.py:272-277, 556-568
  get_kernel_wrapped                                adorym/propagate.py:84-93:  H_d = exp(i a d_d),
                                                    a = -sign_convention PI lambda (u^2 + v^2) per nm, d_d = free_prop_cm[d] * 1e7
  the loss over all distances                       adorym/forward_model.py:1056-1061, 1090

on top of tests/multidist3d_ref.py and the pinned oracle: the exit wave Psi_S of every (position, mode) is the oracle's multislice
sweep without a detector step, then

    Psi_d = IFFT2(H_d Psihat),  Psihat = FFT2(Psi_S),       dPsi_d / dd_d = IFFT2(i a H_d Psihat)
    dL/dd_d = sum over positions, modes, pixels of Re( conj(G_d) dPsi_d / dd_d ),    G_d = dL/dRe Psi_d + i dL/dIm Psi_d,

times 1e7 for the derivative per cm.  The distances go in ROUNDED TO float32 (the engine holds them as float32 on the device), so
that fp64, fp32 and the GPU see the same values.
"""
import copy

import numpy as np

from oracle import adorym_oracle as O
from tests.sparse_ref import masked_loss


def round32(dists_cm):
    return np.asarray(dists_cm, dtype=np.float32).astype(np.float64)


def phase_per_nm(phys, dtype):
    """a[y, x] = -sigma PI lambda (u^2 + v^2), evaluated in ``dtype`` like the reference's tensors."""
    dt = np.dtype(dtype)
    u, v = O.gen_freq_mesh(phys.voxel_nm, phys.probe_size)
    u, v = u.astype(dt), v.astype(dt)
    return (dt.type(-phys.sigma * O.PI * phys.lmbda_nm) * (u ** 2 + v ** 2)).astype(dt)


def kernels(phys, dists_cm, dtype):
    """[D, Py, Px] complex: get_kernel_wrapped with dist_nm = free_prop_cm * 1e7 in ``dtype``."""
    dt = np.dtype(dtype)
    a = phase_per_nm(phys, dt)
    d_nm = (round32(dists_cm).astype(dt) * dt.type(1e7)).astype(dt)
    ph = (d_nm[:, None, None] * a[None]).astype(dt)
    return (np.cos(ph) + 1j * np.sin(ph)).astype(O._cdtype(dt))


def exit_waves(tiles, probes, phys, dtype):
    """[M, B, Py, Px]: the field behind the last slice of every (mode, position)."""
    q = copy.copy(phys)
    q.det_mode, q.h_free = 'none', None
    return np.stack([O.multislice_forward(tiles, p, q, dtype) for p in np.asarray(probes)])


def forward_dist_grad(tiles, probes, meas, phys, dists_cm, dtype='float64', raw_data_type='magnitude', loss_function_type='lsq',
                      poisson_multiplier=1., beamstop=None):
    """tiles [B,Py,Px,S,2], probes complex [M,Py,Px], meas [B*D,Py,Px] position-major (entry b * D + d); the loss arguments and
    ``beamstop`` [Py,Px] as O.forward_adjoint_tiles takes them.
    Returns loss, pred [B*D,Py,Px], dL/d free_prop_cm [D] (per cm) and its per-field terms [B, M, D] (their sum over the first two
    axes is the gradient)."""
    dt = np.dtype(dtype)
    cdt = O._cdtype(dt)
    probes = np.asarray(probes)
    if probes.ndim == 2:
        probes = probes[None]
    M, B, D = len(probes), tiles.shape[0], len(dists_cm)
    Py, Px = phys.probe_size
    H = kernels(phys, dists_cm, dt)                                        # [D,Py,Px]
    a = phase_per_nm(phys, dt)
    spec = np.fft.fft2(exit_waves(tiles.astype(dt, copy=False), probes, phys, dt)).astype(cdt)     # [M,B,Py,Px]
    prod = (spec[:, :, None] * H[None, None]).astype(cdt)                  # [M,B,D,Py,Px]
    fields = np.fft.ifft2(prod).astype(cdt)
    pred = np.abs(fields[0]) if M == 1 else np.sqrt((fields.real ** 2 + fields.imag ** 2).sum(axis=0))
    pred = pred.reshape(B * D, Py, Px).astype(dt)
    meas = np.asarray(meas).astype(dt, copy=False)
    loss, dldp = masked_loss(pred, meas, dt, loss_function_type, raw_data_type, poisson_multiplier, beamstop)
    dldp = dldp.reshape(B, D, Py, Px)
    with np.errstate(divide='ignore', invalid='ignore'):
        unit = fields / pred.reshape(B, D, Py, Px)[None]
        if M == 1:
            unit = np.where(pred.reshape(B, D, Py, Px)[None] > 0, unit, 0)
    G = (dldp[None] * unit).astype(cdt)                                    # [M,B,D,Py,Px]
    dfield = np.fft.ifft2((1j * a[None, None, None] * prod).astype(cdt)).astype(cdt)       # dPsi_d / dd_d per nm
    terms = (np.conj(G) * dfield).real.sum(axis=(-2, -1)).astype(dt)       # [M,B,D]
    terms = np.transpose(terms, (1, 0, 2)) * dt.type(1e7)                  # [B,M,D], per cm
    return loss, pred, terms.sum(axis=(0, 1)), terms


def forward_dist_grad_object(obj, coords_fp16, probes, pos_batch, meas, phys, dists_cm, dtype='float64', raw_data_type='magnitude',
                             loss_function_type='lsq', poisson_multiplier=1., beamstop=None):
    """Rotate, cut the tiles, evaluate.  Returns loss, pred, dL/d free_prop_cm [D] and the per-field terms [B, M, D]."""
    dt = np.dtype(dtype)
    obj = obj.astype(dt, copy=False)
    rot = O.rotate_fwd(obj, coords_fp16, dt) if coords_fp16 is not None else obj
    tiles, _ = O.extract_tiles(rot, pos_batch, phys.probe_size, phys.unknown_type)
    return forward_dist_grad(tiles, probes, meas, phys, dists_cm, dt, raw_data_type, loss_function_type, poisson_multiplier, beamstop)
