"""Generates tests/golden/F31_ctf_invert.npz from the reference implementation (data only).

Usage: python tests/golden/gen_f31_ctf_invert.py        (needs the reference checkout that gen_goldens.py imports; CPU only)

(a) conventional.multidistance_ctf_wrapped (adorym/conventional.py:112-152), the direct inversion of the CTF model, in fp64 AND
    fp32 on the holograms of tests/ctf_matrix.py's GOLDEN_FIELDS (``inputs``: the model of an object at lg_kappa 1.5), inverted at
    lg_kappa 1.7 as the driver would at its first minibatch.  Stored: the inputs, the fp64 phase whole, of the fp32 run only its
    distance from it (the yardstick of the 3x rule).  The same with prj_affine_ls = identity matrices (the reference's own
    bilinear resample of the holograms): the distance of that phase from the one without, in either precision.
(b) one case at lg_kappa = 30 (pure phase: 1 / kappa = 1e-30) on ctf_matrix.PHASE_FIELD.
(c) what the reference DRIVER does with update_using_external_algorithm='ctf' (ptychography.py:1135-1163, array_ops.py:274-286):
    the outcome of the attempt, as text, under 'drv/external_ctf'.
"""
import contextlib
import io
import os
import sys
import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.join(HERE, '..', '..'))
import gen_goldens as G  # noqa: E402  (the I/O shims and the reference on sys.path)
import torch  # noqa: E402
import adorym  # noqa: E402,F401
import adorym.global_settings as gs  # noqa: E402
from adorym.conventional import multidistance_ctf_wrapped  # noqa: E402
from tests import ctf_matrix as CM  # noqa: E402

PURE_PHASE_LG_KAPPA = 30.
DRV = dict(field=(16, 16, 3), n_epochs=2, learning_rate=1e-3, ctf_lg_kappa_learning_rate=2e-2)


def ref_run(c, fp64, lg_kappa, identity=False):
    gs.run_fp64 = fp64
    aff = None
    if identity:
        aff = torch.tensor(np.tile(np.array([[1., 0., 0.], [0., 1., 0.]]), (c['nd'], 1, 1)), dtype=torch.float64 if fp64 else torch.float32)
    with contextlib.redirect_stdout(io.StringIO()):
        phase = multidistance_ctf_wrapped(c['data'].astype(np.float64), np.asarray(c['dists'], dtype=np.float64), CM.ENERGY_EV, CM.PSIZE_CM,
                                          kappa=10. ** float(lg_kappa), safe_zone_width=0, prj_affine_ls=aff)
    return phase.detach().numpy()


def gen_cases(out):
    rel = lambda a, b: float(np.linalg.norm(np.asarray(a, np.float64) - b) / np.linalg.norm(b))
    names = []
    fields = [(f, raw, float(CM.LG_KAPPA)) for f, raw in CM.GOLDEN_FIELDS.items()] + [(CM.PHASE_FIELD, 'intensity', PURE_PHASE_LG_KAPPA)]
    for (ny, nx, nd), raw, lgk in fields:
        name = '%dx%dx%d_%s%s' % (ny, nx, nd, raw, '' if lgk != PURE_PHASE_LG_KAPPA else '_pure_phase')
        names.append(name)
        c = CM.inputs(ny, nx, nd, raw=raw)
        p64, p32 = ref_run(c, True, lgk), ref_run(c, False, lgk)
        a64, a32 = ref_run(c, True, lgk, identity=True), ref_run(c, False, lgk, identity=True)
        assert p64.dtype == np.float64 and p32.dtype == np.float32 and p64.shape == (ny, nx)
        out[name + '/data'], out[name + '/dists'], out[name + '/lg_kappa'] = c['data'], c['dists'], np.array(lgk)
        out[name + '/phase'] = p64
        out[name + '/err32'] = np.array(rel(p32, p64))
        # the identity resample: phase with prj_affine_ls = identity against the phase without, fp64 and fp32
        out[name + '/identity'] = np.array([rel(a64, p64), rel(a32, p32)])
        print(name, 'max |phase| %.4g; fp32 vs fp64 %.1e; identity resample: fp64 %.1e fp32 %.1e'
              % (np.abs(p64).max(), out[name + '/err32'], out[name + '/identity'][0], out[name + '/identity'][1]))
    out['cases'] = np.array(names)


def gen_driver(out):
    ny, nx, nd = DRV['field']
    c = CM.inputs(ny, nx, nd)
    prj = c['data'][None].astype(np.float64)                   # [1, n_dists, ny, nx]

    class MultiDistPlugin(adorym.MultiDistModel):
        # (see gen_goldens.gen_f12: the 'auto' selection passes two keywords MultiDistModel.__init__ does not accept)
        def __init__(self, *a, run_bfloat16=False, run_float64=False, **k):
            super().__init__(*a, **k)

    rec = {}
    try:
        with contextlib.redirect_stdout(io.StringIO()):
            G.run_driver(prj, [ny, nx, 1], np.array([[0., 0.]]), 0, 1,
                         dict(minibatch_size=1, n_epochs=DRV['n_epochs'], two_d_mode=True, energy_ev=CM.ENERGY_EV, psize_cm=CM.PSIZE_CM,
                              free_prop_cm=np.array(c['dists']), initial_guess=[c['obj'][:, :, None, 0].astype(np.float64),
                                                                                c['obj'][:, :, None, 1].astype(np.float64)],
                              probe_type='plane', raw_data_type='intensity', unknown_type='delta_beta', gamma=0, alpha_d=0, alpha_b=0,
                              optimizer='adam', learning_rate=DRV['learning_rate'], forward_algorithm='ctf', ctf_lg_kappa=CM.LG_KAPPA,
                              optimize_ctf_lg_kappa=True, ctf_lg_kappa_learning_rate=DRV['ctf_lg_kappa_learning_rate'], n_dp_batch=1,
                              run_float64=True, randomize_probe_pos=True, safe_zone_width=0, forward_model=MultiDistPlugin,
                              update_using_external_algorithm='ctf'), rec)
        out['drv/external_ctf'] = np.array('ran: losses %r' % (list(rec['losses']),))
    except Exception as e:      # noqa: BLE001  (what the reference does is the datum)
        out['drv/external_ctf'] = np.array('%s: %s' % (type(e).__name__, e))
    print("update_using_external_algorithm='ctf' ->", out['drv/external_ctf'])
    out['drv/params'] = np.array(repr(DRV))


if __name__ == '__main__':
    out = {}
    gen_cases(out)
    gen_driver(out)
    gs.run_fp64 = False
    G.save('F31_ctf_invert', **out)
