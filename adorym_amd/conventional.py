"""
Closed-form ("conventional") phase retrieval, numpy in and out, on the GPU (adorym/conventional.py).  Only what has kernels
here is present: multidistance_ctf_wrapped, on adorym_amd.CTFInversion (include/adm.h adm_ctfinv_*, csrc/adm_ctf_invert.hip).
"""
import numpy as np

from .device import Context
from .holography import CTFInversion


def multidistance_ctf_wrapped(this_prj_batch, free_prop_cm, energy_ev, psize_cm, kappa=50, safe_zone_width=0,
                              prj_affine_ls=None, device=None):
    """The reference's signature (adorym/conventional.py:112-152): this_prj_batch [n_dists, ny, nx] holograms of one angle, used
    as given (I - 1); free_prop_cm [n_dists]; kappa = delta / beta; prj_affine_ls [n_dists, 2, 3] or None.  Returns the phase map
    [ny, nx] as a float32 numpy array.  ``device``: an adorym_amd Context, a device index, or None (device 0).
    With prj_affine_ls the holograms are registered as bilinear samples of |data| (holograms are positive), where the reference
    samples the signed values.  safe_zone_width must be 0, as adorym/array_ops.py:282-285 calls it."""
    if safe_zone_width != 0:
        raise NotImplementedError('multidistance_ctf_wrapped: safe_zone_width != 0 is outside the accelerated path')
    prj = np.ascontiguousarray(np.asarray(this_prj_batch), dtype=np.float32)
    if prj.ndim != 3:
        raise ValueError('multidistance_ctf_wrapped: this_prj_batch must be [n_dists, ny, nx], got %r' % (list(prj.shape),))
    dists = np.asarray(free_prop_cm, dtype=np.float64).reshape(-1)
    if dists.size != prj.shape[0]:
        raise ValueError('multidistance_ctf_wrapped: %d distances for %d holograms' % (dists.size, prj.shape[0]))
    if not kappa > 0:
        raise ValueError('multidistance_ctf_wrapped: kappa must be positive')
    ctx = device if isinstance(device, Context) else Context(0 if device is None else int(device))
    engine = CTFInversion(ctx, prj.shape[1:], prj.shape[0], energy_ev, psize_cm)
    affine = None
    if prj_affine_ls is not None:
        affine = ctx.array(np.ascontiguousarray(np.asarray(prj_affine_ls, dtype=np.float32).reshape(prj.shape[0], 2, 3)), np.float32)
    lg_kappa = ctx.array(np.array([np.log10(float(kappa))]), np.float32)
    out = engine.retrieve(ctx.array(prj, np.float32), dists, lg_kappa, affine=affine)
    return out.get()[0]
