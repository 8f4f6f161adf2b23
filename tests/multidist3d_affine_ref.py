"""NumPy restatement of the reference's multi-distance holography of a 3-D object WITH the affine registration of the measured
holograms (optimize_prj_affine; test infrastructure only: the checker, never the product).

  the registration in front of the loss     adorym/forward_model.py:1066-1072  (w.affine_transform, wrappers.py:1159-1174)
  the loss over all distances               adorym/forward_model.py:1056-1061, 1090

on top of tests/multidist3d_ref.py (the fan-out) and the pinned oracle's affine_sample (torch's affine_grid + grid_sample, bilinear,
border padding, align_corners=False, and its backward).  The registration acts on the data, not on the wave:

    samp_e = affine_sample(|meas_e|, theta_e),   target_e = |samp_e| (magnitude data) or sqrt|samp_e| (intensity data),
    loss   = mean over entries and pixels of (pred_e - target_e)^2,

so prediction, object and probe gradients are the fan-out's with ``target`` as its (magnitude) data, and

    dL/dtheta_e = affine_sample's backward of the cotangent  c_e = -(2/N) (pred_e - target_e) dtarget/dsamp,  N = E * Py * Px,

with c = 0 where it is not finite (an exactly zero sample: 0/0), as oracle.holo_forward_adjoint lines 1135-1149 do it.  Entries are
position-major (e = b * D + d); ``theta`` is [D, 2, 3] (entry e takes matrix e % D, the gradient is summed over the positions) or
[E, 2, 3].  The matrices go in ROUNDED TO float32 (the device holds them as float32), so that fp64, fp32 and the GPU see the same
values.
"""
import numpy as np

from oracle import adorym_oracle as O
from tests import multidist3d_ref as MR

IDENTITY = np.array([[1., 0., 0.], [0., 1., 0.]])


def round32(theta):
    return np.asarray(theta, dtype=np.float32).astype(np.float64)


def matrix(angle=0., scale=1., shift=(0., 0.), mirror=False):
    """[[s cos a, -s sin a, tx], [s sin a, s cos a, ty]] rounded to float32; ``mirror`` negates the first column (determinant < 0)."""
    c, s = scale * np.cos(angle), scale * np.sin(angle)
    m = np.array([[c, -s, shift[0]], [s, c, shift[1]]])
    if mirror:
        m[:, 0] = -m[:, 0]
    return round32(m)


def register(meas, theta, raw_data_type='magnitude', dtype='float64'):
    """meas [E, Py, Px] raw, theta [E, 2, 3].  Returns samp, target [E, Py, Px] in ``dtype``."""
    dt = np.dtype(dtype)
    data = np.abs(np.asarray(meas)).astype(dt)
    th = round32(theta).astype(dt)
    samp = np.stack([O.affine_sample(data[e], th[e]) for e in range(len(data))]).astype(dt)
    a = np.abs(samp)
    return samp, (np.sqrt(a) if raw_data_type == 'intensity' else a).astype(dt)


def affine_grad(meas, theta, pred, raw_data_type='magnitude', dtype='float64', grad_scale=1.):
    """dL/dtheta [E, 2, 3] of L = mean (pred - target)^2 for given predictions [E, Py, Px] (what adm_register_grad computes)."""
    dt = np.dtype(dtype)
    data = np.abs(np.asarray(meas)).astype(dt)
    th = round32(theta).astype(dt)
    samp, tgt = register(meas, theta, raw_data_type, dt)
    pred = np.asarray(pred).astype(dt)
    with np.errstate(divide='ignore', invalid='ignore'):
        dtds = np.sign(samp) / (dt.type(2) * np.sqrt(np.abs(samp))) if raw_data_type == 'intensity' else np.sign(samp)
        cot = (dt.type(-2. * grad_scale / pred.size) * (pred - tgt) * dtds).astype(dt)
    cot = np.where(np.isfinite(cot), cot, 0).astype(dt)
    return np.stack([O.affine_sample(data[e], th[e], cot=cot[e])[1] for e in range(len(data))]).astype(dt)


def per_entry(theta, n_entries):
    theta = np.asarray(theta, dtype=np.float64).reshape(-1, 2, 3)
    if n_entries % len(theta):
        raise ValueError('%d matrices for %d entries' % (len(theta), n_entries))
    return np.tile(theta, (n_entries // len(theta), 1, 1))


def forward_adjoint_tiles(tiles, probes, meas, phys, dists_cm, theta, dtype='float64', raw_data_type='magnitude'):
    """tiles [B,Py,Px,S,2], meas [B*D,Py,Px] position-major (raw), theta [D,2,3] or [B*D,2,3].  Returns a dict: loss, pred and
    target [B*D,Py,Px], gtiles [B,Py,Px,S,2], gprobe complex [M,Py,Px], gtheta (shaped like ``theta``)."""
    dt = np.dtype(dtype)
    E = len(meas)
    th = per_entry(theta, E)
    _, tgt = register(meas, th, raw_data_type, dt)
    loss, pred, gt, gp = MR.forward_adjoint_tiles(tiles.astype(dt, copy=False), probes, tgt, phys, dists_cm, dt, raw_data_type='magnitude')
    g = affine_grad(meas, th, pred, raw_data_type, dt)
    n = len(np.asarray(theta).reshape(-1, 2, 3))
    return dict(loss=loss, pred=pred, target=tgt, gtiles=gt, gprobe=gp, gtheta=g.reshape(E // n, n, 2, 3).sum(axis=0))


def forward_adjoint_object(obj, coords_fp16, probes, pos_batch, meas, phys, dists_cm, theta, dtype='float64', raw_data_type='magnitude'):
    """Rotate, cut the tiles, evaluate, scatter, rotate back.  The dict of forward_adjoint_tiles with 'grad' [Y,X,S,2] for 'gtiles'."""
    dt = np.dtype(dtype)
    obj = obj.astype(dt, copy=False)
    rot = O.rotate_fwd(obj, coords_fp16, dt) if coords_fp16 is not None else obj
    tiles, _ = O.extract_tiles(rot, pos_batch, phys.probe_size, phys.unknown_type)
    r = forward_adjoint_tiles(tiles, probes, meas, phys, dists_cm, theta, dt, raw_data_type)
    g = O.scatter_tiles_adj(r.pop('gtiles'), pos_batch, obj.shape)
    r['grad'] = O.rotate_adj(g, coords_fp16, dt) if coords_fp16 is not None else g
    return r


def warp(images, theta, dtype='float64'):
    """The holograms as a detector displaced by ``theta`` records them: affine_sample of every image by its matrix (how the driver
    fixtures make mis-registered data; registering them with the inverse matrices brings them back up to the interpolation)."""
    dt = np.dtype(dtype)
    th = round32(theta).astype(dt)
    return np.stack([O.affine_sample(np.asarray(images[e], dtype=dt), th[e]) for e in range(len(images))])


def inverse(theta):
    """The inverse maps of [D, 2, 3] matrices (in normalised coordinates), float32-rounded."""
    out = []
    for m in np.asarray(theta, dtype=np.float64).reshape(-1, 2, 3):
        a = np.linalg.inv(m[:, :2])
        out.append(np.concatenate([a, -(a @ m[:, 2])[:, None]], axis=1))
    return round32(np.stack(out))
