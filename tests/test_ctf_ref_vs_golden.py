"""CPU: tests/ctf_ref.py -- the reference of the CTF kernels' GPU tests -- against golden F26 (the reference implementation's own
results), its internal consistency, and the conditions every case of the GPU tables must meet before a GPU is asked."""
import ast
import os

import numpy as np
import pytest

from tests import ctf_matrix as CM
from tests import ctf_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope='module')
def F():
    return np.load(os.path.join(ROOT, 'tests', 'golden', 'F26_ctf.npz'))


def golden_case(F, name):
    ny, nx, nd = (int(v) for v in name.split('_')[0].split('x'))
    raw = name.split('_')[1]
    return dict(ny=ny, nx=nx, nd=nd, raw=raw, obj=F[name + '/obj'], data=F[name + '/data'], dists=F[name + '/dists'],
                lg_kappa=np.float32(CM.LG_KAPPA), clip=False)


def test_golden_holds_every_stated_case(F):
    assert sorted(F['kernel_cases']) == sorted('%dx%dx%d_%s' % (k + (v,)) for k, v in CM.GOLDEN_FIELDS.items())
    for name in F['kernel_cases']:
        c = golden_case(F, name)
        g = CM.inputs(c['ny'], c['nx'], c['nd'], raw=c['raw'])
        for k in ('obj', 'data', 'dists'):
            assert np.array_equal(c[k], g[k]), (name, k)          # the golden's inputs are the matrix's
        assert c['obj'][..., 1].any()                             # beta is there to be ignored


def test_fp64_restatement_equals_the_reference(F):
    for name in F['kernel_cases']:
        c = golden_case(F, name)
        r = CM.ref_run(c, 'float64')
        assert CM.rel(r['pred'], F[name + '/pred']) < 1e-10, name
        assert abs(r['loss'] / float(F[name + '/loss']) - 1) < 1e-10, name
        assert CM.rel(r['grad_delta'], F[name + '/grad'][..., 0]) < 1e-10, name
        assert not F[name + '/grad'][..., 1].any(), name          # dL/dbeta = 0 exactly
        assert abs(r['grad_lg_kappa'] / float(F[name + '/gkappa']) - 1) < 1e-10, name


def test_fp32_restatement_errs_like_the_reference_fp32(F):
    """The float32 restatement is the yardstick of the 3x rule where the golden does not reach: its distance from fp64 is that of
    the reference's own float32 run, within a factor of three either way (prediction and delta gradient), and both kappa gradients
    are far inside the bar."""
    for name in F['kernel_cases']:
        c = golden_case(F, name)
        o, s = CM.ref_run(c, 'float64'), CM.ref_run(c, 'float32')
        e32 = F[name + '/err32']
        mine = [CM.rel(s['pred'], o['pred']), abs(s['loss'] / o['loss'] - 1), CM.rel(s['grad_delta'], o['grad_delta']),
                abs(s['grad_lg_kappa'] / o['grad_lg_kappa'] - 1)]
        print(name, 'reference fp32', e32, 'restatement fp32', mine)
        for k in (0, 2):
            assert e32[k] / 3 < mine[k] < 3 * e32[k], (name, k, mine[k], e32[k])
        assert mine[3] < CM.BARS['gkappa'] / 3 and e32[3] < CM.BARS['gkappa'] / 3


def test_reference_returns_nan_where_I_is_negative(F):
    """What the reference does on the clipped field (recorded, not imitated): prediction 0 on the pixels with I_d < 0, NaN in every
    entry of either gradient.  ctf_ref predicts 0 there too and gives finite gradients."""
    c = CM.inputs(16, 16, 2, clip=True)
    assert np.array_equal(c['obj'], F['clip/obj'])
    r = CM.ref_run(c, 'float64')
    neg = r['I'] <= 0
    assert neg.sum() == 64 and np.array_equal(F['clip/fp64/pred'] == 0, neg)
    assert np.abs(r['pred'] - F['clip/fp64/pred']).max() < 1e-12
    for tag in ('fp64', 'fp32'):
        n_nan, n, k_nan = F['clip/%s/nan_counts' % tag]
        assert n_nan == n and k_nan == 1
    assert np.isfinite(r['grad_delta']).all() and np.isfinite(r['grad_lg_kappa'])


def test_operator_is_self_adjoint():
    r = CM.cases.rng(5)
    for ny, nx, nd in ((16, 16, 3), (32, 16, 2), (16, 64, 1)):
        sn, cs = R.xi_sincos((ny, nx), CM.dists_for(nd), CM.ENERGY_EV, CM.PSIZE_CM)
        o = R.osc(sn, cs, CM.LG_KAPPA)
        x, y = r.standard_normal((ny, nx)), r.standard_normal((nd, ny, nx))
        lhs = float((R.apply(o, x) * y).sum())
        rhs = float((x * R.apply(o, y).sum(axis=0)).sum())
        assert abs(lhs - rhs) <= 1e-12 * max(abs(lhs), np.linalg.norm(x) * np.linalg.norm(y)), (ny, nx, lhs, rhs)


def test_gradients_against_central_differences():
    c = CM.case(16, 32, 2)
    f = lambda k, obj=c['obj']: R.forward_adjoint(obj[:, :, 0], c['dists'], k, c['data'], CM.ENERGY_EV, CM.PSIZE_CM, c['raw'], want_grad=False)['loss']
    k0, h = float(c['lg_kappa']), 1e-4
    fd = (f(k0 + h) - f(k0 - h)) / (2 * h)
    assert abs(fd / c['o64']['grad_lg_kappa'] - 1) < 1e-6, (fd, c['o64']['grad_lg_kappa'])
    r = CM.cases.rng(6)
    v = r.standard_normal((16, 32))
    o = c['obj'].astype(np.float64)
    step = lambda t: np.stack([o[..., 0] + t * v, o[..., 1]], -1)
    fd = (f(k0, step(1e-6)) - f(k0, step(-1e-6))) / 2e-6
    an = float((c['o64']['grad_delta'] * v).sum())
    assert abs(fd / an - 1) < 1e-6, (fd, an)


@pytest.mark.parametrize('shape', CM.FIELDS + (CM.VARIANT_FIELD + ('magnitude',), CM.VARIANT_FIELD + (99,)), ids=lambda s: 'x'.join(str(v) for v in s))
def test_conditions_of_every_gpu_case(shape):
    """min I_d >= 0.05, the float32 restatement within a third of every bar, no band without signal."""
    kw = {}
    if len(shape) == 4:
        kw = dict(raw=shape[3]) if isinstance(shape[3], str) else dict(seed=shape[3])
    print(CM.conditions(CM.case(*shape[:3], **kw)))


@pytest.mark.parametrize('phase', CM.PHASE_RUNGS, ids=lambda v: '%g_rad' % v)
def test_conditions_of_the_large_phase_cases(phase):
    """The same conditions with the distances scaled until xi reaches the rung (MIN_I included: the object needs no less contrast)."""
    c = CM.case(*CM.PHASE_FIELD, phase=phase)
    assert abs(CM.max_xi(c['ny'], c['nx'], c['dists']) / phase - 1) < 1e-9 and CM.max_xi(16, 16, CM.dists_for(3)) < 104
    assert CM.PHASE_FIELD in CM.FIELDS and CM.PHASE_RUNGS[0] <= 100 and CM.PHASE_RUNGS[-1] >= 3000
    print(CM.conditions(c))


def test_conditions_of_the_clipped_case():
    c = CM.case(*CM.VARIANT_FIELD, clip=True)
    print(CM.conditions(c))
    assert np.isfinite(c['o64']['grad_delta']).all() and not c['o64']['pred'][c['o64']['I'] <= 0].any()


def test_driver_restatement_equals_the_reference_driver(F):
    """ctf_ref.reconstruct against the reference driver's fp64 run (golden F26 (b))."""
    obj, data, dists = F['drv/obj'], F['drv/data'], F['drv/dists']
    p = ast.literal_eval(str(F['drv/params']))
    r = R.reconstruct(data, obj[..., 0], obj[..., 1], dists, CM.LG_KAPPA, CM.ENERGY_EV, CM.PSIZE_CM, n_epochs=p['n_epochs'],
                      learning_rate=p['learning_rate'], optimize_ctf_lg_kappa=True, ctf_lg_kappa_learning_rate=p['ctf_lg_kappa_learning_rate'])
    assert np.abs(np.array(r['losses']) / F['drv/fp64/losses'] - 1).max() < 1e-9
    assert np.abs(np.array(r['lg_kappa_trace']) - F['drv/fp64/lg_kappa_trace']).max() < 1e-9
    assert np.abs(r['obj'][..., 0] - F['drv/fp64/delta'][..., 0]).max() < 1e-9 * np.abs(F['drv/fp64/delta']).max()
    assert np.array_equal(r['obj'][..., 1], F['drv/fp64/beta'][..., 0].astype(np.float64)) or np.abs(r['obj'][..., 1] - F['drv/fp64/beta'][..., 0]).max() < 1e-12
    assert CM.rel(r['first_grad'][..., 0], np.asarray(F['drv/first_grad']).reshape(16, 16, -1)[..., 0]) < 1e-9
    assert str(F['drv/flag_off']).startswith('TypeError')          # the reference driver does not run the model with the flag off
