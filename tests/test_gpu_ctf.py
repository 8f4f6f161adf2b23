"""The CTF forward model's kernels (adm_holo_ctf.hip: five line-kernel templates at the eight line lengths of ADM_LINE_SIZES, one
fixed kernel, three ABI entry points) through the C ABI against tests/ctf_ref.py in fp64 (pytest -m gpu).  tests/ctf_matrix.py
holds the fields, the mirror of the launch geometry, the variants and the references; tests/test_ctf_coverage.py ties those tables
to the kernel source, tests/test_ctf_ref_vs_golden.py the reference to golden F26 and every case here to its conditions.

Judged twice.  Whole arrays by the holography path's bars (CM.BARS): loss 5e-5, prediction 5e-6, delta gradient 2e-4 of the norm
and within 3 x the float32 reference's own distance from fp64, kappa gradient max(2e-3, 3 x the float32 reference's).  Then band
by band (holo_matrix.check_bands: 3 x the float32 reference on the same band + the whole-array bar): the rows of every C3 block of
the prediction, the rows of every C5 block of the delta gradient, and every kx line of FFT2 of both.  dL/dbeta is exactly zero.

Every case builds one handle, uploads, launches once and reads back; the reference pair is built once per module (CM.case)."""
import ctypes as C

import numpy as np
import pytest

from tests import ctf_matrix as CM

pytestmark = pytest.mark.gpu
BARS = CM.BARS
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


# ------------------------------------------------------------------------------------------------------------ one launch
class Handle(object):
    def __init__(self, ctx, ny, nx, nd, raw='intensity', energy_ev=CM.ENERGY_EV, psize_cm=CM.PSIZE_CM):
        from adorym_amd._lib import CtfDesc, check
        self.ctx, self.check = ctx, check
        self.h = C.c_void_p()
        desc = CtfDesc(ny=ny, nx=nx, n_dists=nd, raw_intensity=1 if raw == 'intensity' else 0, energy_ev=energy_ev, psize_cm=psize_cm)
        check(ctx.lib.adm_ctf_create(ctx.handle, C.byref(desc), C.byref(self.h)))

    def close(self):
        if self.h:
            self.check(self.ctx.lib.adm_ctf_destroy(self.h))
            self.h = None


def seeds(c, kind, like=None):
    """The gradient buffers before the launch: zeros; 'nan': NaN; 'sentinel': a finite pattern of mixed signs and magnitudes over 2^+-12;
    'seeded': values of mixed signs within a factor of two of the rms of the gradients ``like`` (an earlier launch's)."""
    shapes = dict(g_obj=(c['ny'], c['nx'], 2), g_kappa=(1,))
    if kind is None:
        return {k: np.zeros(s, np.float32) for k, s in shapes.items()}
    if kind == 'nan':
        return {k: np.full(s, np.nan, np.float32) for k, s in shapes.items()}
    if kind == 'sentinel':
        return {k: CM.sentinel(s, 41 + n) for n, (k, s) in enumerate(shapes.items())}
    r = CM.cases.rng(29)
    rms = lambda a: float(np.sqrt(np.mean(np.asarray(a, np.float64)[..., 0] ** 2))) or 1.
    return {k: (r.uniform(0.5, 2, s) * r.choice([-1., 1.], s) * rms(like[k])).astype(np.float32) for k, s in shapes.items()}


def launch(ctx, c, h=None, want_grad=True, overwrite=False, seed=None, like=None, want_pred=True, want_kappa=True, want_loss=True, want_obj=True):
    """One adm_ctf_fwd_adj of the case ``c``; everything it wrote, and the buffers it was given."""
    own = h is None
    h = h or Handle(ctx, c['ny'], c['nx'], c['nd'], c['raw'])
    s0 = seeds(c, seed, like)
    d = {k: ctx.array(v) for k, v in s0.items()}
    obj, data, lgk = ctx.array(c['obj']), ctx.array(c['data']), ctx.array(np.array([c['lg_kappa']], np.float32))
    pred = ctx.array(np.full((c['nd'], c['ny'], c['nx']), -7., np.float32)) if want_pred else None
    loss = ctx.array(np.full((c['nd'],), -7., np.float32)) if want_loss else None
    dists = np.ascontiguousarray(c['dists'], np.float64)
    p = lambda a: a.ptr if a is not None else None
    h.check(ctx.lib.adm_ctf_fwd_adj(h.h, obj.ptr, dists.ctypes.data_as(C.POINTER(C.c_double)), lgk.ptr, data.ptr,
                                    (2 if overwrite else 1) if want_grad else 0, d['g_obj'].ptr if want_obj else None,
                                    p(d['g_kappa']) if want_kappa else None,
                                    p(pred), p(loss)))
    out = dict(pred=pred.get() if want_pred else None, seeds=s0, loss_d=loss.get() if want_loss else None,
               loss=float(loss.get().astype(np.float64).sum() / c['data'].size) if want_loss else None)
    out.update({k: v.get() for k, v in d.items()})
    if own:
        h.close()
    return out


_BASE = {}


def base_launch(ctx, c, key, **kw):
    """The plain accumulating launch into zeros, once per case (what the bit-for-bit relations compare with)."""
    if key not in _BASE:
        _BASE[key] = launch(ctx, c, **kw)
    return _BASE[key]


# ------------------------------------------------------------------------------------------------------------ judgement
def check_whole(res, c, what, grad=True, kappa=True):
    o, s = c['o64'], c['o32']
    if res['loss'] is not None:
        e = abs(res['loss'] / o['loss'] - 1)
        print('%s: loss %.2e' % (what, e))
        assert e < BARS['loss'], (what, 'loss', e)
    if res['pred'] is not None:
        e, e32 = CM.rel(res['pred'], o['pred']), CM.rel(s['pred'], o['pred'])
        print('%s: pred %.2e (fp32 reference %.2e, bar %.0e)' % (what, e, e32, BARS['pred']))
        assert e < BARS['pred'], (what, 'pred', e, e32)
    if grad:
        g = res['g_obj'][..., 0]
        e, e32 = CM.rel(g, o['grad_delta']), CM.rel(s['grad_delta'], o['grad_delta'])
        print('%s: grad_delta %.2e (fp32 reference %.2e, bar %.0e and 3x)' % (what, e, e32, BARS['grad']))
        assert e32 < BARS['grad'] / 3, (what, 'ill-conditioned case', e32)
        assert e < BARS['grad'] and e <= 3 * e32, (what, 'grad_delta', e, e32)
        if kappa:
            e, e32 = abs(res['g_kappa'][0] / o['grad_lg_kappa'] - 1), abs(s['grad_lg_kappa'] / o['grad_lg_kappa'] - 1)
            print('%s: grad_lg_kappa %.2e (fp32 reference %.2e, bar %.1e)' % (what, e, e32, max(BARS['gkappa'], 3 * e32)))
            assert e < max(BARS['gkappa'], 3 * e32), (what, 'grad_lg_kappa', e, e32)


def check_bands(res, c, what, grad=True):
    mine = CM.band_views(c, res['pred'], res['g_obj'][..., 0] if grad else None)
    o, s = CM.band_views(c, c['o64']['pred'], c['o64']['grad_delta']), CM.band_views(c, c['o32']['pred'], c['o32']['grad_delta'])
    worst = {}
    for name, (bands, axis, bar) in CM.band_defs(c).items():
        if name in mine:
            worst[name] = CM.check_bands(mine[name], o[name], s[name], bands, axis, BARS[bar], '%s %s' % (what, name), quiet=True)
    print('%s worst bands (band, of, error, fp32 reference): %s' % (what, {k: '%d/%d %.2e (%.2e)' % v for k, v in worst.items()}))


def same_bits(a, b, what):
    a, b = CM.bits(a), CM.bits(b)
    assert a.shape == b.shape, what
    bad = int((a != b).sum())
    assert bad == 0, (what, '%d of %d elements differ' % (bad, a.size))


def beta_is_plus_zero(res, what):
    assert not CM.bits(res['g_obj'][..., 1]).any(), (what, 'the beta channel of an overwriting launch is not +0')


# ------------------------------------------------------------------------------------------------------------ fields
@pytest.mark.parametrize('shape', CM.FIELDS, ids=ident)
def test_fields_gradient_launch(ctx, shape):
    """C1 ... C5 at every field of CM.FIELDS, accumulating into zeros: loss, prediction, delta and kappa gradients against the fp64
    reference, whole and by bands; the beta channel stays zero."""
    c = CM.case(*shape)
    res = base_launch(ctx, c, shape)
    check_whole(res, c, ident(shape))
    check_bands(res, c, ident(shape))
    assert not CM.bits(res['g_obj'][..., 1]).any()


@pytest.mark.parametrize('shape', CM.FIELDS, ids=ident)
def test_fields_forward_only(ctx, shape):
    """C1, C2, C3<N, false> and ctf_sums_kernel: loss and prediction; sentinel-filled gradient buffers keep their bits."""
    c = CM.case(*shape)
    res = launch(ctx, c, want_grad=False, seed='sentinel')
    check_whole(res, c, ident(shape) + ' forward only', grad=False)
    check_bands(res, c, ident(shape) + ' forward only', grad=False)
    for k in ('g_obj', 'g_kappa'):
        same_bits(res[k], res['seeds'][k], (ident(shape), k, 'written by a forward-only launch'))
    base = base_launch(ctx, c, shape)
    same_bits(res['pred'], base['pred'], 'prediction of the forward-only and the gradient launch')
    assert res['loss'] == base['loss']


# ------------------------------------------------------------------------------------------------------------ variants
@pytest.mark.parametrize('name', list(CM.VARIANTS))
def test_variants(ctx, name):
    """want_grad 0 / 1 / 2; pred, grad_lg_kappa, grad_obj (forward-only, with grad_lg_kappa) and loss_sum each NULL; magnitude data;
    at 128 x 256 x 4.  Bit for bit: prediction and loss are the base launch's; forward-only leaves the gradient buffers alone; accumulated = seeded + overwritten; '+=' keeps the beta channel's sentinel bits, '=' makes it +0."""
    kw = dict(CM.VARIANTS[name])
    raw = kw.pop('raw', 'intensity')
    c = CM.case(*CM.VARIANT_FIELD, raw=raw)
    base = base_launch(ctx, c, CM.VARIANT_FIELD + (raw,))
    res = launch(ctx, c, like=base, **kw)
    grad = kw.get('want_grad', True)
    check_whole(res, c, name, grad=grad and kw.get('seed') is None, kappa=kw.get('want_kappa', True))
    if res['pred'] is not None:
        same_bits(res['pred'], base['pred'], name + ': prediction')
    if res['loss'] is not None:
        assert res['loss'] == base['loss'], name
    if not grad:
        for k in ('g_obj', 'g_kappa'):
            same_bits(res[k], res['seeds'][k], (name, k))
        return
    if not kw.get('want_kappa', True):
        same_bits(res['g_kappa'], res['seeds']['g_kappa'], name + ': grad_lg_kappa not wanted')
    if kw.get('overwrite'):
        same_bits(res['g_obj'][..., 0], base['g_obj'][..., 0], name + ': overwritten = accumulated into zeros')
        same_bits(res['g_kappa'], base['g_kappa'], name + ': grad_lg_kappa')
        beta_is_plus_zero(res, name)
    elif kw.get('seed'):
        same_bits(res['g_obj'][..., 0], res['seeds']['g_obj'][..., 0] + base['g_obj'][..., 0], name + ': accumulated = seeded + overwritten')
        same_bits(res['g_kappa'], res['seeds']['g_kappa'] + base['g_kappa'], name + ': grad_lg_kappa')
        same_bits(res['g_obj'][..., 1], res['seeds']['g_obj'][..., 1], name + ': the beta channel of an accumulating launch')
    else:
        same_bits(res['g_obj'], base['g_obj'], name)
        if kw.get('want_kappa', True):
            same_bits(res['g_kappa'], base['g_kappa'], name)


@pytest.mark.regression
def test_two_launches_give_identical_bits(ctx):
    for shape in (CM.VARIANT_FIELD, (2048, 16, 3), (256, 16, 64)):
        c = CM.case(*shape)
        a, b = launch(ctx, c), launch(ctx, c)
        for k in ('g_obj', 'g_kappa', 'pred'):
            same_bits(a[k], b[k], (shape, k))
        assert a['loss'] == b['loss']


@pytest.mark.regression
def test_one_handle_many_launches(ctx):
    """One handle through differently configured launches equals fresh handles."""
    c = CM.case(*CM.VARIANT_FIELD)
    c2 = CM.case(*CM.VARIANT_FIELD, seed=99)
    h = Handle(ctx, *CM.VARIANT_FIELD)
    seq = [(c, dict(want_grad=False)), (c2, dict(overwrite=True)), (c, dict()), (c2, dict(want_kappa=False, want_pred=False)), (c, dict(overwrite=True))]
    for cc, kw in seq:
        a, b = launch(ctx, cc, h=h, **kw), launch(ctx, cc, **kw)
        for k in ('g_obj', 'g_kappa', 'pred'):
            if a[k] is not None:
                same_bits(a[k], b[k], (kw, k))
        assert a['loss'] == b['loss']
    h.close()


def test_create_refusals(ctx):
    from adorym_amd._lib import CtfDesc, ADM_ERR_UNSUPPORTED
    for ny, nx, nd in ((24, 16, 1), (16, 24, 1), (4096, 16, 1), (16, 4096, 1), (8, 16, 1), (16, 16, 0), (16, 16, 65)):
        h = C.c_void_p()
        desc = CtfDesc(ny=ny, nx=nx, n_dists=nd, raw_intensity=1, energy_ev=CM.ENERGY_EV, psize_cm=CM.PSIZE_CM)
        rc = ctx.lib.adm_ctf_create(ctx.handle, C.byref(desc), C.byref(h))
        assert rc == ADM_ERR_UNSUPPORTED and not h.value, (ny, nx, nd, rc)
        assert b'adm_ctf_create' in ctx.lib.adm_last_error()


def test_engine_matches_the_abi(ctx, A):
    """adorym_amd.CTFEngine: forward_adjoint / loss / pred hand over what the C ABI gives."""
    c = CM.case(*CM.VARIANT_FIELD)
    base = base_launch(ctx, c, CM.VARIANT_FIELD + ('intensity',))
    eng = A.CTFEngine(ctx, CM.VARIANT_FIELD[:2], CM.VARIANT_FIELD[2], CM.ENERGY_EV, CM.PSIZE_CM, raw_data_type='intensity')
    g, gk = ctx.zeros((c['ny'], c['nx'], 2)), ctx.zeros((1,))
    eng.forward_adjoint(ctx.array(c['obj']), c['dists'], ctx.array(np.array([c['lg_kappa']], np.float32)), ctx.array(c['data']),
                        want_grad=True, grad_obj=g, grad_lg_kappa=gk, want_pred=True, overwrite=True)
    assert eng.loss() == base['loss']
    same_bits(eng.pred(), base['pred'], 'engine pred')
    same_bits(g.get()[..., 0], base['g_obj'][..., 0], 'engine grad')
    same_bits(gk.get(), base['g_kappa'], 'engine grad_lg_kappa')


# ------------------------------------------------------------------------------------------------------------ large arguments
@pytest.mark.parametrize('phase', CM.PHASE_RUNGS, ids=lambda v: '%g_rad' % v)
def test_large_phase(ctx, phase):
    """ctf_sincos goes through sincos_fast, as the Fresnel factor of adm_holo.hip does: the distances of 32 x 16 x 2 scaled so that
    xi reaches 100, 1000 and 3000 rad (the rungs of tests/holo_value_matrix.py; the table's own distances reach 103 rad), judged
    by this module's rules whole and by bands."""
    c = CM.case(*CM.PHASE_FIELD, phase=phase)
    what = '%s at %g rad' % (ident(CM.PHASE_FIELD), phase)
    res = launch(ctx, c)
    check_whole(res, c, what)
    check_bands(res, c, what)
    assert not CM.bits(res['g_obj'][..., 1]).any()


# ------------------------------------------------------------------------------------------------------------ the clip
def test_clip(ctx):
    """A quarter of the pixels of at least one distance have I_d <= -0.05 (none lies between -0.05 and 0.05): the prediction is
    exactly 0 there, every gradient is finite and equals ctf_ref's, which defines those pixels' contribution as zero."""
    c = CM.case(*CM.VARIANT_FIELD, clip=True)
    res = launch(ctx, c)
    neg = c['o64']['I'] <= CM.CLIP_I
    assert neg.sum() >= c['ny'] * c['nx'] // 8
    assert not CM.bits(res['pred'][neg]).any() and (res['pred'][~neg] > 0).all()
    assert np.isfinite(res['g_obj']).all() and np.isfinite(res['g_kappa']).all()
    check_whole(res, c, 'clip')
