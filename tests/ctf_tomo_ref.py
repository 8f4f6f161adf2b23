"""NumPy restatement of the contrast-transfer-function model of a 3-D object (forward_algorithm='ctf', two_d_mode=False:
adorym/forward_model.py:905-914 rotates the object, adorym/propagate.py:467-476 sums it along the beam, w.sum(grid_batch, axis=-2),
and hands the sum of delta to pure_phase_ctf), of its loss and of the gradients w.r.t. the object and lg_kappa: O.rotate_fwd, a sum,
tests/ctf_ref.py, and the transposes in reverse.  fp64, and fp32 with the reference's float32 roundings.
tests/test_ctf_tomo_ref_vs_golden.py holds it to golden F30; ``cases`` are the golden's inputs."""
import numpy as np

from oracle import adorym_oracle as O
from tests import ctf_matrix as CM
from tests import ctf_ref as R
from tests.golden import cases as GC

#       name: (Y, X, Z), theta, number of distances
CASES = {
    'y16x16z16_t0.7_d3':  ((16, 16, 16), 0.7, 3),
    'y32x16z8_t0.3_d2':   ((32, 16, 8), 0.3, 2),          # Y != X != Z
    'y16x16z16_t0_d2':    ((16, 16, 16), 0.0, 2),
    'y16x16z16_halfpi_d2': ((16, 16, 16), np.pi / 2, 2),
    'y16x32z5_t2.0_d2':   ((16, 32, 5), 2.0, 2),
}


def inputs(name):
    """obj [Y, X, Z, 2] float32 -- delta a windowed random map with a profile along the beam, scaled by 1 / Z because the model's
    phase map is the raw sum of delta; beta non-zero: the model must ignore it -- data [nd, Y, X] float32 (intensities: the fp64 model
    of a second map at lg_kappa 1.5), dists [nd] float64, theta float32."""
    (Y, X, Z), theta, nd = CASES[name]
    s = 3000 + 31 * Y + 7 * X + 3 * Z + nd
    r = GC.rng(s)
    prof = 0.5 + r.uniform(size=Z)
    delta = CM.delta_map(Y, X, s)[:, :, None] * prof[None, None, :] / Z + 2e-3 / Z * r.standard_normal((Y, X, Z))
    beta = 1e-3 / Z * r.uniform(size=(Y, X, Z))
    obj = np.stack([delta, beta], -1).astype(np.float32)
    dists = CM.dists_for(nd)
    truth = CM.delta_map(Y, X, s + 50, scale=1.2)
    I = R.forward_adjoint(truth.astype(np.float32), dists, CM.LG_KAPPA_TRUTH, np.ones((nd, Y, X)), CM.ENERGY_EV, CM.PSIZE_CM, want_grad=False)['I']
    return dict(size=(Y, X, Z), theta=np.float32(theta), nd=nd, obj=obj, data=I.astype(np.float32), dists=dists, lg_kappa=np.float32(CM.LG_KAPPA),
                raw='intensity')


def driver_inputs(N, n_theta, nd):
    """The driver run of golden F30: the initial guess obj [N, N, N, 2] float32 (delta scaled by 1 / N, beta non-zero), the truth
    [N, N, N, 2] the measurement is the fp64 model of, dists [nd]."""
    r = GC.rng(3090)
    mk = lambda seed, scale: (CM.delta_map(N, N, seed, scale)[:, :, None] * (0.5 + r.uniform(size=N))[None, None, :] / N
                              + 2e-3 / N * r.standard_normal((N, N, N)))
    delta, truth = mk(3091, 1.), mk(3141, 1.2)
    beta = 1e-3 / N * r.uniform(size=(N, N, N))
    return dict(obj=np.stack([delta, beta], -1).astype(np.float32), truth=np.stack([truth, np.zeros_like(truth)], -1).astype(np.float32),
                dists=CM.dists_for(nd))


def project(obj, coords, dtype='float64'):
    """[Y, X, Z, 2] -> [Y, X, 2]: the rotated object summed along the beam."""
    o = np.asarray(obj, dtype=dtype)
    rot = o if coords is None else np.asarray(O.rotate_fwd(o, coords, dtype), dtype=dtype)
    return rot.sum(axis=2, dtype=dtype)


def backproject(gproj, coords, Z, dtype='float64'):
    """The transpose: [Y, X, 2] copied to every z', then back-rotated -> [Y, X, Z, 2]."""
    vol = np.ascontiguousarray(np.broadcast_to(np.asarray(gproj, dtype=dtype)[:, :, None, :], gproj.shape[:2] + (Z, 2)))
    return vol if coords is None else np.asarray(O.rotate_adj(vol, coords, dtype), dtype=dtype)


def forward_adjoint(c, dtype='float64', lg_kappa=None):
    """dict(pred [nd, Y, X], loss, I, grad [Y, X, Z, 2] (beta's channel zero), gkappa) of the case ``c`` (``inputs``)."""
    coords = O.rotation_coords(c['size'], np.float32(c['theta']))
    p = project(c['obj'], coords, dtype)
    r = R.forward_adjoint(p[..., 0], c['dists'], c['lg_kappa'] if lg_kappa is None else lg_kappa, c['data'], CM.ENERGY_EV, CM.PSIZE_CM, c['raw'], dtype)
    g2 = np.stack([r['grad_delta'], np.zeros_like(r['grad_delta'])], -1)
    return dict(pred=r['pred'], loss=r['loss'], I=r['I'], proj=p, grad=backproject(g2, coords, c['size'][2], dtype), gkappa=r['grad_lg_kappa'])
