"""The CTF model's distance gradient (adm_ctfd_fwd_adj, adm_ctf_dist.hip: the launch group of adm_holo_ctf.hip with the distances on
the device, dL/dd summed in C4 / C5) through the C ABI against tests/ctf_dist_ref.py in fp64 (pytest -m gpu).
tests/ctf_dist_matrix.py holds the fields, the branches and the references; tests/test_ctf_dist_coverage.py ties those tables to the
sources, tests/test_ctf_dist_ref_vs_golden.py the reference to golden F32, to central differences and to its conditions.

dL/dd is judged element by element: |g - g64| <= max(2e-4, 3 x the float32 restatement's error) x max|g64|; every element is at least
1e-2 of the largest, so a dropped or doubled distance is 50 bars away.  Prediction, loss, delta and kappa gradients stay under
ctf_matrix.BARS by ctf_matrix's judgement.

adm_ctf_fwd_adj itself is held to the bits it gave before the feature by tests/test_gpu_ctf_group_bits.py.

Every case builds one handle, uploads, launches once and reads back; the reference pair is built once per module (DM.case)."""
import ctypes as C

import numpy as np
import pytest

from tests import ctf_dist_matrix as DM
from tests import ctf_dist_ref as DR
from tests import ctf_matrix as CM
from tests.test_gpu_ctf import Handle, check_whole, same_bits
from tests.test_gpu_ctf import launch as old_launch

pytestmark = pytest.mark.gpu
ident = lambda s: '%dx%dx%d' % tuple(s)


@pytest.fixture(scope='module')
def A():
    import adorym_amd
    return adorym_amd


@pytest.fixture(scope='module')
def ctx(A):
    c = A.Context(0)
    yield c
    c.close()


def seeds(c, kind, like=None):
    shapes = dict(g_obj=(c['ny'], c['nx'], 2), g_kappa=(1,), g_dists=(c['nd'],))
    if kind is None:
        return {k: np.zeros(s, np.float32) for k, s in shapes.items()}
    if kind == 'nan':
        return {k: np.full(s, np.nan, np.float32) for k, s in shapes.items()}
    if kind == 'sentinel':
        return {k: CM.sentinel(s, 51 + n) for n, (k, s) in enumerate(shapes.items())}
    r = CM.cases.rng(31)
    rms = lambda a: float(np.sqrt(np.mean(np.asarray(a, np.float64).reshape(-1, a.shape[-1] if a.ndim == 3 else 1)[:, 0] ** 2))) or 1.
    return {k: (r.uniform(0.5, 2, s) * r.choice([-1., 1.], s) * rms(like[k])).astype(np.float32) for k, s in shapes.items()}


def launch(ctx, c, h=None, want_grad=True, overwrite=False, seed=None, like=None, want_dists=True, n_launches=1, dists=None):
    """adm_ctfd_fwd_adj of the case ``c`` at its model distances; everything it wrote, and the buffers it was given."""
    own = h is None
    h = h or Handle(ctx, c['ny'], c['nx'], c['nd'], c['raw'])
    s0 = seeds(c, seed, like)
    d = {k: ctx.array(v) for k, v in s0.items()}
    obj, data, lgk = ctx.array(c['obj']), ctx.array(c['data']), ctx.array(np.array([c['lg_kappa']], np.float32))
    dd = ctx.array(np.asarray(c['model_dists'] if dists is None else dists, np.float32))
    pred = ctx.array(np.full((c['nd'], c['ny'], c['nx']), -7., np.float32))
    loss = ctx.array(np.full((c['nd'],), -7., np.float32))
    for _ in range(n_launches):
        h.check(ctx.lib.adm_ctfd_fwd_adj(h.h, obj.ptr, dd.ptr, lgk.ptr, data.ptr, (2 if overwrite else 1) if want_grad else 0,
                                         d['g_obj'].ptr, d['g_kappa'].ptr, d['g_dists'].ptr if want_dists else None, pred.ptr, loss.ptr))
    out = dict(pred=pred.get(), seeds=s0, loss_d=loss.get(), loss=float(loss.get().astype(np.float64).sum() / c['data'].size))
    out.update({k: v.get() for k, v in d.items()})
    if own:
        h.close()
    return out


def check_dists(res, c, what):
    e, bar = DM.dist_errors(res['g_dists'], c['o64']['grad_dists']), DM.dist_bar(c)
    print('%s: dL/dd %s (fp64 %s): errors %s, bars %s' % (what, res['g_dists'], c['o64']['grad_dists'], e, bar))
    assert np.isfinite(res['g_dists']).all() and (e <= bar).all(), (what, e, bar)


_BASE = {}


def base_launch(ctx, c, key):
    if key not in _BASE:
        _BASE[key] = launch(ctx, c)
    return _BASE[key]


# ------------------------------------------------------------------------------------------------------------ accuracy
@pytest.mark.parametrize('shape', DM.FIELDS, ids=ident)
def test_fields(ctx, shape):
    """C1 ... C5 with the distances on the device and grad_dists, accumulating into zeros: dL/dd element by element, the other
    outputs under ctf_matrix's bars; the beta channel stays zero."""
    c = DM.case(*shape)
    res = base_launch(ctx, c, shape)
    check_dists(res, c, ident(shape))
    check_whole(res, c, ident(shape))
    assert not CM.bits(res['g_obj'][..., 1]).any()


def test_golden_cases(ctx):
    """The cases of golden F32 (a): dL/dd against the reference's own fp64 run, its fp32 run the yardstick."""
    import os
    F = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden', 'F32_ctf_dist.npz'))
    for name in F['model_cases']:
        name = str(name)
        ny, nx, nd = (int(v) for v in name.split('_')[0].split('x'))
        c = dict(ny=ny, nx=nx, nd=nd, raw=name.split('_')[1], obj=F[name + '/obj'], data=F[name + '/data'], model_dists=F[name + '/model_dists'],
                 lg_kappa=np.float32(CM.LG_KAPPA))
        res = launch(ctx, c)
        g64 = F[name + '/gdists']
        e, bar = DM.dist_errors(res['g_dists'], g64), np.maximum(DM.BARS['grad'], 3 * F[name + '/err32'][4:])
        print('%s: dL/dd %s (golden %s): errors %s, bars %s' % (name, res['g_dists'], g64, e, bar))
        assert (e <= bar).all(), (name, e, bar)
        assert CM.rel(res['pred'], F[name + '/pred']) < DM.BARS['pred'] and abs(res['loss'] / float(F[name + '/loss']) - 1) < DM.BARS['loss']
        assert CM.rel(res['g_obj'][..., 0], F[name + '/grad'][..., 0]) < DM.BARS['grad']
        assert abs(res['g_kappa'][0] / float(F[name + '/gkappa']) - 1) < DM.BARS['gkappa']


def test_large_phase(ctx):
    """The distances of 32 x 16 x 2 scaled so that xi reaches 3000 rad: dL/dd under the same rule."""
    c = DM.case(*DM.PHASE_FIELD, phase=DM.PHASE_RUNG)
    res = launch(ctx, c)
    check_dists(res, c, '%s at %g rad' % (ident(DM.PHASE_FIELD), DM.PHASE_RUNG))


# ------------------------------------------------------------------------------------------------------------ variants
@pytest.mark.parametrize('name', list(DM.VARIANTS))
def test_variants(ctx, name):
    """'+=' on a seeded buffer: seeded + the base launch's bits; '=' over a NaN sentinel: the base launch's bits, every output finite."""
    kw = DM.VARIANTS[name]
    c = DM.case(*DM.VARIANT_FIELD)
    base = base_launch(ctx, c, DM.VARIANT_FIELD)
    res = launch(ctx, c, like=base, **kw)
    same_bits(res['pred'], base['pred'], name + ': prediction')
    assert res['loss'] == base['loss']
    if kw.get('overwrite'):
        for k in ('g_dists', 'g_kappa'):
            same_bits(res[k], base[k], (name, k))
        same_bits(res['g_obj'][..., 0], base['g_obj'][..., 0], name)
        assert not CM.bits(res['g_obj'][..., 1]).any()
    else:
        for k in ('g_dists', 'g_kappa'):
            same_bits(res[k], res['seeds'][k] + base[k], (name, k, 'accumulated = seeded + overwritten'))
        same_bits(res['g_obj'][..., 0], res['seeds']['g_obj'][..., 0] + base['g_obj'][..., 0], name)


@pytest.mark.parametrize('shape', ((16, 16, 3), (1024, 16, 3), (256, 16, 64)), ids=ident)
def test_null_grad_dists_changes_no_other_bit(ctx, shape):
    """With grad_dists NULL every other output has the bits it has with it, and the buffer is not touched."""
    c = DM.case(*shape)
    base = base_launch(ctx, c, shape)
    res = launch(ctx, c, want_dists=False, seed=None)
    for k in ('pred', 'g_obj', 'g_kappa'):
        same_bits(res[k], base[k], (shape, k))
    assert res['loss'] == base['loss'] and not CM.bits(res['g_dists']).any()


@pytest.mark.regression
def test_two_launches_give_identical_bits_and_twice_accumulated_is_double(ctx):
    for shape in ((16, 16, 3), (2048, 16, 3), (256, 16, 64)):
        c = DM.case(*shape)
        a, b = base_launch(ctx, c, shape), launch(ctx, c)
        for k in ('g_obj', 'g_kappa', 'g_dists', 'pred'):
            same_bits(a[k], b[k], (shape, k))
        twice = launch(ctx, c, n_launches=2)
        same_bits(twice['g_dists'], 2 * a['g_dists'], (shape, 'twice += equals 2 x one launch'))
        same_bits(twice['g_kappa'], 2 * a['g_kappa'], (shape, 'g_kappa'))


def test_forward_only_touches_no_gradient(ctx):
    c = DM.case(*DM.VARIANT_FIELD)
    base = base_launch(ctx, c, DM.VARIANT_FIELD)
    res = launch(ctx, c, want_grad=False, seed='sentinel')
    for k in ('g_obj', 'g_kappa', 'g_dists'):
        same_bits(res[k], res['seeds'][k], (k, 'written by a forward-only launch'))
    same_bits(res['pred'], base['pred'], 'prediction')
    assert res['loss'] == base['loss']


@pytest.mark.regression
def test_one_handle_alternates_the_entries(ctx):
    """One handle through adm_ctf_fwd_adj and adm_ctfd_fwd_adj in turn equals fresh handles."""
    c = DM.case(*DM.VARIANT_FIELD)
    old_c = dict(c, dists=c['model_dists'])
    h = Handle(ctx, *DM.VARIANT_FIELD)
    fresh_old, fresh_new = old_launch(ctx, old_c), base_launch(ctx, c, DM.VARIANT_FIELD)
    for _ in range(2):
        a = old_launch(ctx, old_c, h=h)
        for k in ('g_obj', 'g_kappa', 'pred'):
            same_bits(a[k], fresh_old[k], ('old entry', k))
        b = launch(ctx, c, h=h)
        for k in ('g_obj', 'g_kappa', 'g_dists', 'pred'):
            same_bits(b[k], fresh_new[k], ('new entry', k))
    h.close()
    # host and device distances are two roundings of the same numbers: the entries agree far inside the bars
    assert CM.rel(fresh_old['pred'], fresh_new['pred']) < DM.BARS['pred'] / 3


# ------------------------------------------------------------------------------------------------------------ refusals, engine
def test_refusals(ctx):
    from adorym_amd._lib import ADM_ERR_INVALID
    c = DM.case(*DM.VARIANT_FIELD)
    h = Handle(ctx, *DM.VARIANT_FIELD)
    obj, data, lgk = ctx.array(c['obj']), ctx.array(c['data']), ctx.array(np.array([c['lg_kappa']], np.float32))
    dd, g, gd = ctx.array(np.asarray(c['model_dists'], np.float32)), ctx.zeros((c['ny'], c['nx'], 2)), ctx.zeros((c['nd'],))
    f = ctx.lib.adm_ctfd_fwd_adj
    calls = {'null handle': (None, obj.ptr, dd.ptr, lgk.ptr, data.ptr, 1, g.ptr, None, gd.ptr, None, None),
             'null distances': (h.h, obj.ptr, None, lgk.ptr, data.ptr, 1, g.ptr, None, gd.ptr, None, None),
             'null object': (h.h, None, dd.ptr, lgk.ptr, data.ptr, 1, g.ptr, None, gd.ptr, None, None),
             'want_grad 3': (h.h, obj.ptr, dd.ptr, lgk.ptr, data.ptr, 3, g.ptr, None, gd.ptr, None, None),
             'want_grad without grad_obj': (h.h, obj.ptr, dd.ptr, lgk.ptr, data.ptr, 1, None, None, gd.ptr, None, None)}
    for what, a in calls.items():
        assert f(*a) == ADM_ERR_INVALID, what
        assert b'adm_ctfd_fwd_adj' in ctx.lib.adm_last_error(), what
    assert not CM.bits(gd.get()).any()
    h.close()


def test_engine_refine_distances(ctx, A):
    """CTFEngine(refine_distances=True): engine.dists is the parameter; host values are uploaded into it; forward_adjoint hands over
    what the C ABI gives."""
    shape = DM.VARIANT_FIELD
    c = DM.case(*shape)
    base = base_launch(ctx, c, shape)
    eng = A.CTFEngine(ctx, shape[:2], shape[2], CM.ENERGY_EV, CM.PSIZE_CM, raw_data_type='intensity', refine_distances=True, dists_cm=c['dists'])
    assert np.array_equal(eng.dists.get(), np.float32(c['dists']))
    obj, lgk, data = ctx.array(c['obj']), ctx.array(np.array([c['lg_kappa']], np.float32)), ctx.array(c['data'])
    g, gk, gd = ctx.zeros((c['ny'], c['nx'], 2)), ctx.zeros((1,)), ctx.zeros((shape[2],))
    eng.forward_adjoint(obj, c['model_dists'], lgk, data, grad_obj=g, grad_lg_kappa=gk, grad_dists=gd, want_pred=True, overwrite=True)
    assert np.array_equal(eng.dists.get(), np.float32(c['model_dists']))
    assert eng.loss() == base['loss']
    for got, k in ((eng.pred(), 'pred'), (g.get()[..., 0], 'g_obj'), (gk.get(), 'g_kappa'), (gd.get(), 'g_dists')):
        same_bits(got, base[k][..., 0] if k == 'g_obj' else base[k], 'engine ' + k)
    gd2 = ctx.zeros((shape[2],))
    eng.forward_adjoint(obj, eng.dists, lgk, data, grad_obj=g, grad_dists=gd2, overwrite=True)          # (the array itself: nothing is uploaded)
    same_bits(gd2.get(), base['g_dists'], 'engine, its own array')


def test_engine_refusals(ctx, A):
    shape = DM.VARIANT_FIELD
    c = DM.case(*shape)
    obj, lgk, data = ctx.array(c['obj']), ctx.array(np.array([c['lg_kappa']], np.float32)), ctx.array(c['data'])
    g, gd = ctx.zeros((c['ny'], c['nx'], 2)), ctx.zeros((shape[2],))
    plain = A.CTFEngine(ctx, shape[:2], shape[2], CM.ENERGY_EV, CM.PSIZE_CM)
    assert plain.dists is None and not plain.refine_distances
    with pytest.raises(ValueError, match='refine_distances'):
        plain.forward_adjoint(obj, c['dists'], lgk, data, grad_obj=g, grad_dists=gd)
    with pytest.raises(ValueError, match='refine_distances'):
        plain.forward_adjoint(obj, ctx.array(np.float32(c['dists'])), lgk, data, grad_obj=g)
    with pytest.raises(ValueError, match='refine_distances'):
        A.CTFEngine(ctx, shape[:2], shape[2], CM.ENERGY_EV, CM.PSIZE_CM, dists_cm=c['dists'])
    eng = A.CTFEngine(ctx, shape[:2], shape[2], CM.ENERGY_EV, CM.PSIZE_CM, refine_distances=True, dists_cm=c['dists'])
    with pytest.raises(ValueError, match="engine's own array"):
        eng.forward_adjoint(obj, ctx.array(np.float32(c['dists'])), lgk, data, grad_obj=g)
    with pytest.raises(ValueError, match='distances given'):
        eng.forward_adjoint(obj, c['dists'][:2], lgk, data, grad_obj=g)
    with pytest.raises(ValueError, match='grad_dists must be'):
        eng.forward_adjoint(obj, eng.dists, lgk, data, grad_obj=g, grad_dists=ctx.zeros((shape[2] + 1,)))
    assert not CM.bits(gd.get()).any() and not CM.bits(g.get()).any()
