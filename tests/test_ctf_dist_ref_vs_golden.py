"""CPU: tests/ctf_dist_ref.py against golden F32 (the reference's own runs, tests/golden/gen_f32_ctf_dist.py) and against central
differences in fp64, and every case of tests/ctf_dist_matrix.py against the conditions the reference pair alone decides."""
import ast
import os

import numpy as np
import pytest

from tests import ctf_dist_matrix as DM
from tests import ctf_dist_ref as DR
from tests import ctf_matrix as CM

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope='module')
def F():
    return np.load(os.path.join(ROOT, 'tests', 'golden', 'F32_ctf_dist.npz'))


def _case(F, name):
    ny, nx, nd = (int(v) for v in name.split('_')[0].split('x'))
    raw = name.split('_')[1]
    return dict(ny=ny, nx=nx, nd=nd, raw=raw, obj=F[name + '/obj'], data=F[name + '/data'], dists=F[name + '/model_dists'])


def test_golden_holds_the_fields_of_F26_and_a_yardstick():
    F = np.load(os.path.join(ROOT, 'tests', 'golden', 'F32_ctf_dist.npz'))
    names = ['%dx%dx%d_%s' % (f + (raw,)) for f, raw in CM.GOLDEN_FIELDS.items()]
    assert sorted(F['model_cases']) == sorted(names)
    for n in names:
        for tag in (n, 'reg/' + n):
            assert F[tag + '/err32'][4:].max() < 1e-2          # (the generator's assertion: the fp32 reference is a yardstick)
        assert np.array_equal(F[n + '/model_dists'], np.float32(F[n + '/model_dists']))


@pytest.mark.parametrize('reg', (False, True), ids=('plain', 'registered'))
def test_restatement_vs_golden(F, reg):
    """fp64 restatement against the reference's fp64 run to 1e-9 (registered: 1e-6, grid_sample's coordinates are float chains of
    their own); the float32 restatement's distance from fp64 within 3 x the reference's own + 1e-6."""
    for name in F['model_cases']:
        c = _case(F, str(name))
        tag = ('reg/' if reg else '') + str(name)
        run = lambda dt: (DR.registered(c['obj'][..., 0], c['dists'], CM.LG_KAPPA, c['data'], F['kernel_theta'][:c['nd']], CM.ENERGY_EV,
                                        CM.PSIZE_CM, c['raw'], dt) if reg else
                          DR.forward_adjoint(c['obj'][..., 0], c['dists'], CM.LG_KAPPA, c['data'], CM.ENERGY_EV, CM.PSIZE_CM, c['raw'], dt))
        o, s = run(np.float64), run(np.float32)
        tol = 1e-6 if reg else 1e-9
        assert CM.rel(o['pred'], F[tag + '/pred']) < tol and abs(o['loss'] / float(F[tag + '/loss']) - 1) < 10 * tol
        assert CM.rel(o['grad_delta'], F[tag + '/grad'][..., 0]) < 10 * tol
        assert abs(o['grad_lg_kappa'] / float(F[tag + '/gkappa']) - 1) < 1e3 * tol
        e = DM.dist_errors(o['grad_dists'], F[tag + '/gdists'])
        e32 = DM.dist_errors(s['grad_dists'], F[tag + '/gdists'])
        print(tag, 'dL/dd fp64 restatement %.1e, fp32 restatement %s, fp32 reference %s' % (e.max(), e32, F[tag + '/err32'][4:]))
        assert e.max() < 1e3 * tol
        assert (e32 <= 3 * F[tag + '/err32'][4:] + 1e-5).all()
        if reg:
            assert CM.rel(o['target'], F[tag + '/target']) < tol
            for d in range(1, c['nd']):
                assert CM.rel(o['grad_theta'][d], F[tag + '/gtheta'][d]) < 1e-5, (tag, d)


def test_restatement_vs_central_differences(F):
    """The closed form against central differences of tests/ctf_ref.py's fp64 loss at a step of 1e-4 d."""
    for f in (s for s in DM.FIELDS if s[0] * s[1] * s[2] <= 4096):
        c = DM.case(*f)
        cd = DR.central_differences(c['obj'][:, :, 0], c['model_dists'], c['lg_kappa'], c['data'], CM.ENERGY_EV, CM.PSIZE_CM, c['raw'])
        e = DM.dist_errors(o := c['o64']['grad_dists'], cd)
        print(f, o, cd, e)
        assert e.max() < 5e-4, (f, e)


@pytest.mark.parametrize('shape', DM.FIELDS, ids=lambda s: '%dx%dx%d' % tuple(s))
def test_conditions(shape):
    """Every |dL/dd_i| is at least 1e-2 of the largest and the float32 restatement lies within a third of every bar."""
    print(shape, DM.conditions(DM.case(*shape)))


@pytest.mark.parametrize('tag', ('drv_dist', 'drv_aff', 'drv_both'))
def test_driver_loop_vs_golden(F, tag):
    """ctf_dist_ref.reconstruct against the reference driver's fp64 run: losses, distances and matrices after every update."""
    par = ast.literal_eval(str(F['drv/params']))
    dist, aff = tag != 'drv_aff', tag != 'drv_dist'
    obj = F['drv/obj']
    r = DR.reconstruct(F['drv/data_warped' if aff else 'drv/data'], obj[..., 0], obj[..., 1], F['drv/model_dists' if dist else 'drv/dists_true'],
                       CM.LG_KAPPA, CM.ENERGY_EV, CM.PSIZE_CM, n_epochs=par['n_epochs'], learning_rate=par['learning_rate'],
                       optimize_free_prop=dist, free_prop_learning_rate=par['free_prop_learning_rate'], optimize_prj_affine=aff,
                       prj_affine_learning_rate=par['prj_affine_learning_rate'])
    t = tag + '/fp64/'
    e = np.abs(np.array(r['losses']) / F[t + 'losses'] - 1).max()
    print(tag, 'losses', e)
    assert e < 1e-6
    if dist:
        assert np.abs(r['dists_trace'] / F[t + 'dists'] - 1).max() < 1e-6
        # the distances move towards the truth
        assert (np.abs(F[t + 'dists'][-1] - F['drv/dists_true']) < np.abs(F['drv/model_dists'] - F['drv/dists_true'])).all()
    if aff:
        assert np.abs(r['theta_trace'] - F[t + 'theta']).max() < 1e-5
        assert np.array_equal(F[t + 'theta'][:, 0], np.tile(np.array([[1., 0, 0], [0, 1., 0]]), (par['n_epochs'], 1, 1)))


def test_tomography_loop_vs_golden_F30():
    """ctf_dist_ref.reconstruct_tomo with the distances and matrices held fixed is the reference's own driver run of golden F30:
    losses, kappa after every update and the final object."""
    F30 = np.load(os.path.join(ROOT, 'tests', 'golden', 'F30_ctf_tomo.npz'))
    par = ast.literal_eval(str(F30['drv/params']))
    theta_ls = np.linspace(0, np.pi, par['n_theta'], dtype='float32')
    r = DR.reconstruct_tomo(F30['drv/prj'], F30['drv/obj'], F30['drv/dists'], CM.LG_KAPPA, theta_ls, CM.ENERGY_EV, CM.PSIZE_CM,
                            n_epochs=par['n_epochs'], learning_rate=par['learning_rate'], optimize_ctf_lg_kappa=True,
                            ctf_lg_kappa_learning_rate=par['ctf_lg_kappa_learning_rate'])
    assert np.abs(np.array(r['losses']) / F30['drv/fp64/losses'] - 1).max() < 1e-7
    assert np.abs(np.array(r['lg_kappa_trace']) - F30['drv/fp64/lg_kappa_trace']).max() < 1e-9
    x64 = np.stack([F30['drv/fp64/delta'], F30['drv/fp64/beta']], -1)
    assert np.abs(r['obj'] - x64).max() < 1e-9
