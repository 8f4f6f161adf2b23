"""Every instantiation of the holography kernels (adm_holo.hip: nine line-kernel templates at the eight line lengths of
ADM_LINE_SIZES, two fixed kernels, seven ABI entry points) against the fp64 oracle (pytest -m gpu).  tests/holo_matrix.py holds
the fields, the mirror of the launch geometry, the variants and the references; tests/test_holo_matrix_coverage.py ties those
tables to the kernel source.

Judged twice.  Whole arrays by the bars of the holography tests of test_gpu_edge_cases.py (HM.BARS).  Then band by band along
the launch geometry, by the rule of test_gpu_streamed_matrix.check_bands: a band's error is at most 3 x the error of the oracle's
float32 run on the same band + the whole-array bar as a floor.  Bands: the rows of every row block of K1 / K5 (prediction of
every distance, object gradient, probe gradient), the jobs of every K3 block (prediction), and -- with a plane probe, where
grad_obj is the inverse transform of K4's output -- every kx line of the two-dimensional spectrum of the object gradient (K4:
one block per line) and every kx block of the spectrum of the prediction (K2).  The spectral gradient bands have a floor of
2e-5, not 2e-4: 2e-5 is the absolute floor the streamed matrix uses for gradient bands (ms_matrix.GENERIC['grad_abs']), the
oracle's float32 run is within 1.3e-6 ... 2.6e-6 on every such line where ny <= 256 and within 9e-6 / 2e-5 / 3.9e-5 at
ny = 512 / 1024 / 2048, where 3 x that figure carries the bar (python -m tests.test_gpu_holo_matrix prints the figures), and
under 2e-4 an error of 5e-5 in one line's transfer function would pass.

The fields that contain a 2048-long axis run kernels no test had launched before this module (global-memory twiddles, one line
per block, TPR = 256): they have test functions of their own (test_new_kernels_*), which pytest runs after the others of the
same kind have passed.

Every case builds one engine, uploads, launches once and reads back; the bit-for-bit relations compare with one more launch
(into zeros), made once per field.  Every oracle pair is built once per module (HM.case)."""
import ctypes as C
import time

import numpy as np
import pytest

from tests import holo_matrix as HM

pytestmark = pytest.mark.gpu
BARS = HM.BARS
SPECTRAL_GRAD_FLOOR = 2e-5
OTHERS = [f for f in HM.FIELDS if f not in HM.NEW_KERNELS]
ident = lambda s: '%dx%d' % s


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
def engine(ctx, c):
    from adorym_amd.holography import HolographyEngine
    return HolographyEngine(ctx, (c['ny'], c['nx']), c['nd'], HM.ENERGY_EV, HM.PSIZE_CM, sign_convention=c['sigma'],
                            unknown_type=c['unknown_type'], raw_data_type=c['raw'])


def ri(z):
    return np.stack([z.real, z.imag], -1).astype(np.float32)


def seeds(c, kind, like=None):
    """The gradient buffers' contents before the launch: zeros; 'sentinel': a finite pattern of mixed signs and magnitudes over
    2^+-12; 'seeded': values of mixed signs within a factor of two of the rms of the gradients ``like`` (an earlier launch's), so
    that the sum keeps bits of both."""
    shapes = dict(g_obj=c['obj'].shape, g_probe=(c['ny'], c['nx'], 2), g_dists=(c['nd'],), g_aff=(c['nd'], 2, 3), g_shifts=(c['nd'], 2))
    if kind is None:
        return {k: np.zeros(s, np.float32) for k, s in shapes.items()}
    if kind == 'sentinel':
        return {k: HM.sentinel(s, 17 + n) for n, (k, s) in enumerate(shapes.items())}
    r = HM.cases.rng(23)
    rms = lambda a: float(np.sqrt(np.mean(np.asarray(a, np.float64) ** 2))) or 1.
    return {k: (r.uniform(0.5, 2, s) * r.choice([-1., 1.], s) * rms(like[k])).astype(np.float32) for k, s in shapes.items()}


def launch(ctx, c, eng=None, want_grad=True, overwrite=False, seed=None, like=None, want=('probe', 'dists', 'affine'), want_pred=True,
           identity_matrices=False, shifted=False, spectrum=None):
    """One forward_adjoint (or forward_adjoint_shifted) of the case ``c``; everything it wrote, and the buffers it was given."""
    eng = eng or engine(ctx, c)
    s0 = seeds(c, seed, like)
    d = {k: ctx.array(v) for k, v in s0.items()}
    obj, probe, dists = ctx.array(c['obj']), ctx.array(ri(c['probe'])), ctx.array(c['dists'])
    g = lambda k, name: d[k] if name in want else None
    if shifted:
        spec = spectrum if spectrum is not None else eng.data_spectrum(ctx.array(c['data']))
        eng.forward_adjoint_shifted(obj, probe, dists, spec, ctx.array(c['shifts']), want_grad=want_grad, grad_obj=d['g_obj'],
                                    grad_probe=g('g_probe', 'probe'), grad_shifts=g('g_shifts', 'shifts'), want_pred=want_pred,
                                    overwrite=overwrite)
    else:
        aff = ctx.array(c['affine']) if (c['has_affine'] or identity_matrices) else None
        eng.forward_adjoint(obj, probe, dists, ctx.array(c['data']), affine=aff, want_grad=want_grad, grad_obj=d['g_obj'],
                            grad_probe=g('g_probe', 'probe'), grad_dists=g('g_dists', 'dists'), grad_affine=g('g_aff', 'affine'),
                            want_pred=want_pred, overwrite=overwrite)
    out = dict(loss=eng.loss(), pred=eng.pred() if want_pred else None, seeds=s0, engine=eng)
    out.update({k: v.get() for k, v in d.items()})
    if shifted:
        out['target'] = eng.shifted_targets()
    return out


_BASE = {}


def base_launch(ctx, c, key, **kw):
    """The plain accumulating launch into zeros, once per case (what the bit-for-bit relations compare with)."""
    if key not in _BASE:
        r = launch(ctx, c, **kw)
        r.pop('engine')
        _BASE[key] = r
    return _BASE[key]


# ------------------------------------------------------------------------------------------------------------ judgement
def check_whole(res, c, what, want=('probe', 'dists', 'affine'), grad=True, oracle_affine=True):
    o, s = c['o64'], c['o32']
    e = abs(res['loss'] / o['loss'] - 1)
    print('%s: loss %.2e' % (what, e))
    assert e < BARS['loss'], (what, 'loss', e)
    arrays = [('pred', 'pred', BARS['pred'])] if res['pred'] is not None else []
    if grad:
        arrays.append(('g_obj', 'g_obj', BARS['grad']))
        if 'probe' in want:
            arrays.append(('g_probe', 'g_probe', BARS['grad']))
    for k, ko, bar in arrays:
        x = HM.complex_of(res[k]) if k == 'g_probe' else res[k]
        e, e32 = HM.rel(x, o[ko]), HM.rel(s[ko], o[ko])
        print('%s: %s %.2e (fp32 oracle %.2e, bar %.0e)' % (what, k, e, e32, bar))
        # the case itself must be well-conditioned: where the oracle's own fp32 run misses a third of the bar, the 3x rule of
        # the bands and the bar contradict each other
        assert e32 < bar / 3, (what, k, 'ill-conditioned case', e32)
        assert e < bar, (what, k, e, e32)
    if grad:
        for k, name, bar in (('g_dists', 'dists', BARS['gdists']), ('g_aff', 'affine', BARS['gaff'])):
            if name in want and (k != 'g_aff' or oracle_affine):
                e, e32 = HM.rel(res[k], o[k]), HM.rel(s[k], o[k])
                print('%s: %s %.2e (fp32 oracle %.2e, bar %.1e)' % (what, k, e, e32, max(bar, 3 * e32)))
                assert e < max(bar, 3 * e32), (what, k, e, e32)


def check_row_bands(res, c, what, want=('probe',), grad=True):
    """Prediction of every distance, object gradient and probe gradient per row block; the prediction per K3 block too."""
    o, s = c['o64'], c['o32']
    g = HM.geometry(c['ny'], c['nx'], c['nd'])
    worst = {}
    if res['pred'] is not None:
        per_d = [HM.check_bands(res['pred'][d], o['pred'][d], s['pred'][d], g['row_blocks'], 0, BARS['pred'], '%s pred[%d] rows' % (what, d),
                                quiet=True) for d in range(c['nd'])]
        worst['pred'] = max(per_d, key=lambda w: w[2] - 3 * w[3])
        flat = lambda a: np.asarray(a).reshape(c['nd'] * c['ny'], c['nx'])
        worst['pred_k3'] = HM.check_bands(flat(res['pred']), flat(o['pred']), flat(s['pred']), g['k3_blocks'], 0, BARS['pred'],
                                          what + ' pred K3 jobs', quiet=True)
    if grad:
        cx = lambda a: HM.complex_of(np.asarray(a)[:, :, 0])
        worst['g_obj'] = HM.check_bands(cx(res['g_obj']), cx(o['g_obj']), cx(s['g_obj']), g['row_blocks'], 0, BARS['grad'], what + ' g_obj rows', quiet=True)
        if 'probe' in want:
            worst['g_probe'] = HM.check_bands(HM.complex_of(res['g_probe']), o['g_probe'], s['g_probe'], g['row_blocks'], 0, BARS['grad'],
                                              what + ' g_probe rows', quiet=True)
    print('%s worst bands (band, of, error, fp32 oracle): %s' % (what, {k: '%d/%d %.2e (%.2e)' % v for k, v in worst.items()}))
    return worst


def untouched(res, keys, what):
    for k in keys:
        assert np.array_equal(HM.bits(res[k]), HM.bits(res['seeds'][k])), (what, k, 'written by a launch that must not')


def same_bits(a, b, what):
    a, b = HM.bits(a), HM.bits(b)
    assert a.shape == b.shape, what
    bad = int((a != b).sum())
    assert bad == 0, (what, '%d of %d elements differ' % (bad, a.size))


# ------------------------------------------------------------------------------------------------------------ fields
def gradient_launch(ctx, shape):
    c = HM.case(*shape, HM.FIELDS[shape])
    res = base_launch(ctx, c, ('field', shape))
    check_whole(res, c, ident(shape))
    check_row_bands(res, c, ident(shape))


def forward_only(ctx, shape):
    c = HM.case(*shape, HM.FIELDS[shape])
    res = launch(ctx, c, want_grad=False, seed='sentinel')
    check_whole(res, c, ident(shape) + ' forward only', grad=False)
    check_row_bands(res, c, ident(shape) + ' forward only', grad=False)
    untouched(res, ('g_obj', 'g_probe', 'g_dists', 'g_aff'), ident(shape))


@pytest.mark.parametrize('shape', OTHERS, ids=ident)
def test_fields_gradient_launch(ctx, shape):
    """K1, K2, K3<N, true>, K4, K5<N, false> at every field of HM.FIELDS with a structured complex probe, affine matrices and
    every gradient: loss, prediction, object / probe / distance / affine gradients against the fp64 oracle, whole and by bands.

    64x512 is the case that found K3 evaluating its sampling coordinates with th[0] * X contracted into the sum: affine gradient
    2.48e-3 of the norm where the fp32 oracle, which rounds every product, reaches 2.1e-5 (bar 2e-3); the oracle with the same
    contraction restated on the host gives 2.48e-3 too.  affine_coords now rounds as the reference's tensors do."""
    gradient_launch(ctx, shape)


@pytest.mark.parametrize('shape', OTHERS, ids=ident)
def test_fields_forward_only(ctx, shape):
    """K1, K2, K3<N, false>, holo_sums_kernel: loss and prediction against the oracle; no gradient buffer is written."""
    forward_only(ctx, shape)


@pytest.mark.parametrize('shape', [f for f in HM.SPECTRUM_FIELDS if f not in HM.NEW_KERNELS], ids=ident)
def test_k4_lines_in_the_spectrum(ctx, shape):
    spectrum_lines(ctx, shape)


def spectrum_lines(ctx, shape):
    """Plane probe, real_imag object, broadband inputs: FFT2(grad_obj) is K4's output, judged per kx line (K4's blocks); FFT2 of
    the prediction of every distance per kx block of K2.  A wrong transfer function in one block of either kernel spreads over
    every pixel; in the spectrum it stays in its lines."""
    c = HM.case(*shape, HM.FIELDS[shape], probe='plane', broadband=True)
    o, s = c['o64'], c['o32']
    res = launch(ctx, c)
    what = ident(shape) + ' spectrum'
    check_whole(res, c, what)
    g = HM.geometry(c['ny'], c['nx'], c['nd'])
    lines = [(k, k + 1) for k in range(c['nx'])]
    w = HM.check_bands(HM.spectrum2(res['g_obj']), HM.spectrum2(o['g_obj']), HM.spectrum2(s['g_obj']), lines, 1, SPECTRAL_GRAD_FLOOR, what + ' K4 lines')
    assert w[1] == c['nx']
    for d in range(c['nd']):
        HM.check_bands(HM.spectrum2(res['pred'][d]), HM.spectrum2(o['pred'][d]), HM.spectrum2(s['pred'][d]), g['col_blocks'], 1, BARS['pred'],
                       what + ' K2 blocks, distance %d' % d, quiet=d > 0)


# ------------------------------------------------------------------------------------------------------------ variants
def variant(ctx, name, shape):
    ckw, lkw, _ = HM.VARIANTS[name]
    c = HM.case(*shape, HM.FIELDS[shape], **ckw)
    what = '%s %s' % (name, ident(shape))
    want = lkw.get('want', ('probe', 'dists', 'affine'))
    grad = lkw.get('want_grad', True)
    key = ('variant', shape, tuple(sorted(ckw.items())))
    if name in ('accumulate', 'accumulate_delta_beta'):
        # += into seeded buffers: seeded + what the launch into zeros gives, ONE rounding (the relation test_gpu_elementwise.py uses);
        # the probe gradient is written, not accumulated
        base = base_launch(ctx, c, key)
        res = launch(ctx, c, like=base, **lkw)
        for k in ('g_obj', 'g_dists', 'g_aff'):
            assert (HM.bits(res[k]) != HM.bits(base[k])).mean() > 0.9 and (HM.bits(res[k]) != HM.bits(res['seeds'][k])).mean() > 0.9, (what, k, 'seed')
            same_bits(res[k], res['seeds'][k] + base[k], (what, k, 'accumulated = seeded + result into zeros'))
        same_bits(res['g_probe'], base['g_probe'], (what, 'g_probe'))
        assert res['loss'] == base['loss']
        check_whole(base, c, what)
        return
    res = launch(ctx, c, **lkw)
    if name == 'overwrite_sentinel':
        base = base_launch(ctx, c, key)
        for k in ('g_obj', 'g_probe', 'g_dists', 'g_aff'):
            same_bits(res[k], base[k], (what, k, 'overwritten sentinel = result into zeros'))
        same_bits(res['pred'], base['pred'], (what, 'pred'))
        assert res['loss'] == base['loss']
    if name == 'grad_affine_without_affine':
        # affine = NULL is the identity: the gradient with respect to the matrices is still formed, and everything equals the
        # launch with identity matrices uploaded.  (Not against the oracle: at the identity the sampling points sit ON pixel
        # centres, where rounding decides which one-sided derivative is taken.)
        same = launch(ctx, c, identity_matrices=True)
        for k in ('g_obj', 'g_probe', 'g_dists', 'g_aff', 'pred'):
            same_bits(res[k], same[k], (what, k, 'affine = NULL equals identity matrices'))
        assert res['loss'] == same['loss'] and np.abs(res['g_aff']).min() > 0
    if name == 'clamped_translation':
        # 0.2 / 0.15 in normalised coordinates: a band of a tenth of the width and 0.075 of the height is sampled at the clamped
        # border, where grid_sampler's backward pass gives zero (HoloArgs mx / my) -- the oracle's affine_sample reproduces it
        cx, cy = HM.clamped_samples(c)
        print('%s: %d samples clamped in x, %d in y, of %d' % (what, cx, cy, c['nd'] * c['ny'] * c['nx']))
        assert cx > 0.05 * c['nd'] * c['ny'] * c['nx'] and cy > 0.05 * c['nd'] * c['ny'] * c['nx']
    check_whole(res, c, what, want=want, grad=grad, oracle_affine=name != 'grad_affine_without_affine')
    check_row_bands(res, c, what, want=want, grad=grad)
    if not grad:
        untouched(res, ('g_obj', 'g_probe', 'g_dists', 'g_aff'), what)
    if name == 'no_pred':
        assert res['pred'] is None and res['engine']._pred is None


@pytest.mark.parametrize('name', list(HM.VARIANTS))
def test_variants(ctx, name):
    """Every argument value of HM.VARIANTS at 128 x 256 (the docstrings of the table's rows say what each is there for)."""
    variant(ctx, name, HM.VARIANT_FIELD)


# ------------------------------------------------------------------------------------------------------------ fused Adam
def fused_adam(ctx, shape, unknown_type='real_imag', pin=False):
    from adorym_amd.optimizers import AdamOptimizer, apply_small_params
    c = HM.case(*shape, HM.FIELDS[shape], unknown_type=unknown_type)
    nd = c['nd']
    step_obj = 1e-2 if unknown_type == 'real_imag' else 1e-8
    probe, data = ctx.array(ri(c['probe'])), ctx.array(c['data'])
    first = ctx.array(np.array([[1., 0, 0], [0, 1., 0]], np.float32)) if pin else None
    out = []
    for fused in (False, True):
        eng = engine(ctx, c)
        obj, dists, aff = ctx.array(c['obj']), ctx.array(c['dists']), ctx.array(c['affine'])
        o_obj = AdamOptimizer('obj', options_dict={'step_size': step_obj}); o_obj.create_param_arrays(list(obj.shape), device=ctx)
        o_d = AdamOptimizer('free_prop_cm', options_dict={'step_size': 1e-1}); o_d.create_param_arrays([nd], device=ctx)
        o_a = AdamOptimizer('prj_affine_ls', options_dict={'step_size': 1e-3}); o_a.create_param_arrays(list(aff.shape), device=ctx)
        mv = lambda o: (o.params_whole_array_dict['m'], o.params_whole_array_dict['v'])
        g, gd, ga = ctx.array(HM.sentinel(obj.shape, 1)), ctx.array(HM.sentinel((nd,), 2)), ctx.array(HM.sentinel(aff.shape, 3))
        losses = []
        for k in range(2):
            if fused:
                eng.forward_adjoint_adam(obj, probe, dists, data, mv(o_obj), step_obj, k, affine=aff, dists_mv=mv(o_d), step_dists=1e-1,
                                         affine_mv=mv(o_a), step_affine=1e-3, affine_pin=first)
            else:
                eng.forward_adjoint(obj, probe, dists, data, affine=aff, grad_obj=g, grad_dists=gd, grad_affine=ga, overwrite=True)
                items = [dict(opt=o_obj, x=obj.view(0, (obj.size,)), g=g.view(0, (g.size,))), dict(opt=o_d, x=dists, g=gd),
                         dict(opt=o_a, x=aff, g=ga, pin=first) if pin else dict(opt=o_a, x=aff, g=ga)]
                apply_small_params(ctx, items, k)
            losses.append(eng.loss())
        out.append(dict(obj=obj.get(), d=dists.get(), a=aff.get(), m=[t.get() for o in (o_obj, o_d, o_a) for t in mv(o)], losses=losses))
    sep, fus = out
    what = 'fused Adam %s %s' % (ident(shape), unknown_type)
    assert np.abs(fus['obj'] - c['obj']).max() > 0.5 * step_obj and np.abs(fus['d'] - c['dists']).max() > 1e-3, what
    assert np.abs(fus['a'][-1] - c['affine'][-1]).max() > 1e-4, what
    for k in ('obj', 'd', 'a'):
        same_bits(sep[k], fus[k], (what, k))
    for n, (u, v) in enumerate(zip(sep['m'], fus['m'])):
        same_bits(u, v, (what, 'moment', n))
    assert sep['losses'] == fus['losses'] and sep['losses'][0] != sep['losses'][1], (what, sep['losses'], fus['losses'])
    if pin:
        assert np.array_equal(fus['a'][0], np.array([[1., 0, 0], [0, 1., 0]], np.float32))


@pytest.mark.regression
@pytest.mark.parametrize('shape,unknown_type,pin', [(f, 'real_imag', False) for f in HM.BIG8 if f not in HM.NEW_KERNELS]
                         + [((128, 256), 'delta_beta', False), ((256, 128), 'real_imag', True)],
                         ids=lambda v: ident(v) if isinstance(v, tuple) else str(v))
def test_fused_adam_equals_the_separate_update_bitwise(ctx, shape, unknown_type, pin):
    """adm_holo_fwd_adj_adam (holo_k5<N, true>: Adam of object, distances and matrices inside the last kernel) against
    adm_holo_fwd_adj(overwrite) over sentinels + the one small-parameter launch: two minibatches, every array, moment and loss
    equal bit for bit."""
    fused_adam(ctx, shape, unknown_type, pin)


# ------------------------------------------------------------------------------------------------------------ shift stage
def shift_stage(ctx, shape):
    shift_stage_of(ctx, HM.case(*shape, HM.FIELDS[shape], shifts=True), ident(shape) + ' shifts')


def shift_stage_of(ctx, c, what):
    """The shift stage of the case ``c`` (tests/test_gpu_holo_value_domain.py judges its cases with it too); returns the launch."""
    nd = c['nd']
    o, s = c['o64'], c['o32']
    g = HM.geometry(c['ny'], c['nx'], nd)
    eng = engine(ctx, c)
    spec = eng.data_spectrum(ctx.array(c['data']))
    # D^ [d][kx][ky] against FFT2(|data|): itself a spectrum, so the blocks of SLF<N, 0> are judged directly
    got = HM.complex_of(spec.get()).transpose(0, 2, 1)
    w64, w32 = HM.data_spectrum_pair(c)
    e, e32 = HM.rel(got, w64), HM.rel(w32, w64)
    print('%s: spectrum %.2e (fp32 transform %.2e)' % (what, e, e32))
    assert e < BARS['spectrum'], (what, e)
    HM.check_bands(got, w64, w32, g['col_blocks'], 1, BARS['spectrum'], what + ' spectrum kx blocks')
    res = launch(ctx, c, eng=eng, shifted=True, spectrum=spec, want=('probe', 'shifts'))
    # the registered targets Re IFFT2(D^ Phi) (SLI + SRI), as the loss sees them
    tg = np.sqrt(np.abs(res['target']))
    e, e32 = HM.rel(tg, o['target']), HM.rel(s['target'], o['target'])
    print('%s: targets %.2e (fp32 oracle %.2e)' % (what, e, e32))
    assert e < max(BARS['target'], 3 * e32), (what, 'targets', e, e32)
    for d in range(nd):
        HM.check_bands(tg[d], o['target'][d], s['target'][d], g['row_blocks'], 0, BARS['target'], what + ' targets[%d] rows' % d, quiet=d > 0)
    check_whole(res, c, what, want=('probe',))
    check_row_bands(res, c, what)
    e, e32 = np.linalg.norm(res['g_shifts'] - o['g_shifts']), np.linalg.norm(s['g_shifts'] - o['g_shifts'])
    n = np.linalg.norm(o['g_shifts'])
    print('%s: g_shifts %.2e (fp32 oracle %.2e) of the norm' % (what, e / n, e32 / n))
    assert e < max(BARS['gshift'] * n, 3 * e32), (what, res['g_shifts'], o['g_shifts'], s['g_shifts'])
    # forward only: the same loss, grad_shifts untouched
    fwd = launch(ctx, c, eng=eng, shifted=True, spectrum=spec, want_grad=False, seed='sentinel', want=('probe', 'shifts'), want_pred=False)
    assert abs(fwd['loss'] / o['loss'] - 1) < BARS['loss']
    untouched(fwd, ('g_obj', 'g_probe', 'g_shifts'), what)
    return res


@pytest.mark.parametrize('shape', [f for f in HM.SHIFT_FIELDS if f not in HM.NEW_KERNELS], ids=ident)
def test_shift_stage(ctx, shape):
    """holo_sr, holo_slf<N, 0>, holo_sli, holo_sri, holo_slf<N, 1>, holo_shift_sum_kernel: the data spectrum per kx block against
    np.fft.fft2, the registered targets whole and per row block, loss / prediction / object and probe gradient against the
    oracle (shifts=), the shift gradient by the 3x rule; a forward-only launch leaves grad_shifts as it was."""
    shift_stage(ctx, shape)


# ------------------------------------------------------------------------------------------------------------ handle state
KEYS = ('g_obj', 'g_probe', 'g_dists', 'g_aff', 'g_shifts', 'pred')


def test_one_handle_across_differently_configured_launches(ctx):
    """What a handle keeps between launches -- the affine slots of part3 (zeroed once), cot / direct, part_s (allocated on first
    use), T14 as T1 and T4, Wq and T3 shared with the shift stage -- must not leak from one launch into the next: six differently
    configured launches on one engine, each equal bit for bit to the same launch on a fresh engine."""
    shape = (64, 512)
    a, sh = HM.case(*shape, HM.FIELDS[shape]), HM.case(*shape, HM.FIELDS[shape], shifts=True)
    seq = [('all gradients', a, dict()),
           ('object and probe only', a, dict(want=('probe',))),
           ('forward only', a, dict(want_grad=False, seed='sentinel')),
           ('shifted, grad_shifts', sh, dict(shifted=True, want=('probe', 'shifts'))),
           ('shifted, no grad_shifts', sh, dict(shifted=True, want=('probe',))),
           ('all gradients again', a, dict())]
    eng = engine(ctx, a)
    for what, c, kw in seq:
        used = launch(ctx, c, eng=eng, **kw)
        fresh = launch(ctx, c, **kw)
        assert used['loss'] == fresh['loss'], (what, used['loss'], fresh['loss'])
        for k in KEYS:
            same_bits(used[k], fresh[k], (what, k))
        if kw.get('shifted'):
            same_bits(used['target'], fresh['target'], (what, 'target'))
    # the loss of every one of them against the oracle (a sequence that is wrong twice in the same way would still pass above)
    assert abs(used['loss'] / a['o64']['loss'] - 1) < BARS['loss']


def test_registration_excludes_the_fused_update_and_affine_matrices(ctx):
    from adorym_amd._lib import ADM_ERR_INVALID, ADM_OK, HoloAdam
    c = HM.case(16, 16, 1)
    eng = engine(ctx, c)
    lib = ctx.lib
    obj, probe, dists, data, aff = (ctx.array(c['obj']), ctx.array(ri(c['probe'])), ctx.array(c['dists']), ctx.array(c['data']),
                                    ctx.array(c['affine']))
    g, m, v = ctx.zeros(obj.shape), ctx.zeros(obj.shape), ctx.zeros(obj.shape)
    loss = eng._pinned[0].handle
    assert lib.adm_holo_set_registration(eng.handle, None, 1) == ADM_OK
    o = HoloAdam(m_obj=m.ptr, v_obj=v.ptr, step_obj=1e-2, i_batch=0, b1=0.9, b2=0.999, eps=1e-7)
    assert lib.adm_holo_fwd_adj_adam(eng.handle, obj.ptr, probe.ptr, dists.ptr, None, data.ptr, C.byref(o), None, loss) == ADM_ERR_INVALID
    assert lib.adm_holo_fwd_adj(eng.handle, obj.ptr, probe.ptr, dists.ptr, aff.ptr, data.ptr, 1, g.ptr, None, None, None, None, loss) == ADM_ERR_INVALID
    assert lib.adm_holo_set_registration(eng.handle, None, 0) == ADM_OK
    ctx.sync()
    assert not m.get().any() and not g.get().any() and np.array_equal(obj.get(), c['obj'])       # nothing was launched
    # a cotangent buffer alone excludes the fused update too
    cot = ctx.zeros((1, 16, 16))
    assert lib.adm_holo_set_registration(eng.handle, cot.ptr, 0) == ADM_OK
    assert lib.adm_holo_fwd_adj_adam(eng.handle, obj.ptr, probe.ptr, dists.ptr, None, data.ptr, C.byref(o), None, loss) == ADM_ERR_INVALID
    assert lib.adm_holo_set_registration(eng.handle, None, 0) == ADM_OK
    assert lib.adm_holo_fwd_adj_adam(eng.handle, obj.ptr, probe.ptr, dists.ptr, None, data.ptr, C.byref(o), None, loss) == ADM_OK
    ctx.sync()
    assert m.get().any()


# ------------------------------------------------------------------------------------------------------------ refusals
def test_refusals_of_create(ctx):
    """Error codes only; nothing is launched."""
    from adorym_amd._lib import ADM_ERR_INVALID, ADM_ERR_UNSUPPORTED, ADM_OK, HoloDesc
    lib = ctx.lib

    def create(ny=32, nx=32, nd=3, sign=1, ctx_h=ctx.handle, null_desc=False, null_out=False):
        d = HoloDesc(ny=ny, nx=nx, n_dists=nd, lambda_nm=0.07, voxel_nm_y=1000., voxel_nm_x=1000., sign_convention=sign, unknown_type=1,
                     raw_intensity=1, k1=1.)
        h = C.c_void_p()
        rc = lib.adm_holo_create(ctx_h, None if null_desc else C.byref(d), None if null_out else C.byref(h))
        if rc == ADM_OK:
            assert lib.adm_holo_destroy(h) == ADM_OK
        else:
            assert not h.value
        return rc

    assert create() == ADM_OK
    for n in (8, 48, 4096, 0, -16, 2047):
        assert create(ny=n) == ADM_ERR_UNSUPPORTED, n
        assert create(nx=n) == ADM_ERR_UNSUPPORTED, n
    for n in (HM.MIN_SIDE, HM.MAX_SIDE):
        assert create(ny=n, nd=1) == ADM_OK and create(nx=n, nd=1) == ADM_OK
    for nd in (0, HM.MAX_DISTS + 1, -1):
        assert create(nd=nd) == ADM_ERR_INVALID, nd
    assert create(ny=16, nx=16, nd=HM.MAX_DISTS) == ADM_OK
    for sign in (0, 2):
        assert create(sign=sign) == ADM_ERR_INVALID
    assert create(sign=-1) == ADM_OK
    assert create(ctx_h=None) == ADM_ERR_INVALID
    assert create(null_desc=True) == ADM_ERR_INVALID
    assert create(null_out=True) == ADM_ERR_INVALID


# ------------------------------------------------------------------------------------------------------------ the 2048-long axis
# Kernels no test had launched before this module; every function below runs after the others of its kind above.
@pytest.mark.parametrize('shape', HM.NEW_KERNELS, ids=ident)
def test_new_kernels_gradient_launch(ctx, shape):
    gradient_launch(ctx, shape)


@pytest.mark.parametrize('shape', HM.NEW_KERNELS, ids=ident)
def test_new_kernels_forward_only(ctx, shape):
    forward_only(ctx, shape)


def test_new_kernels_lines_in_the_spectrum(ctx):
    """2048 x 16: holo_k2<2048> and holo_k4<2048>, one line per block, 16 blocks each; K4 in three rounds of one distance."""
    assert HM.geometry(2048, 16, 3)['k4_rounds'] == 3 and HM.line_geo(2048)['LPB'] == 1
    spectrum_lines(ctx, (2048, 16))


@pytest.mark.parametrize('name', [n for n, v in HM.VARIANTS.items() if v[2]])
def test_new_kernels_variants(ctx, name):
    """The variants that touch K2 or K4, again at 2048 x 16."""
    variant(ctx, name, HM.VARIANT_FIELD_K4)


@pytest.mark.regression
@pytest.mark.parametrize('shape', HM.NEW_KERNELS, ids=ident)
def test_new_kernels_fused_adam(ctx, shape):
    fused_adam(ctx, shape)


@pytest.mark.parametrize('shape', HM.NEW_KERNELS, ids=ident)
def test_new_kernels_shift_stage(ctx, shape):
    shift_stage(ctx, shape)


@pytest.mark.regression
@pytest.mark.parametrize('shape', HM.NEW_KERNELS, ids=ident)
def test_new_kernels_two_launches_give_identical_bits(ctx, shape):
    """The fixed order of every sum (adm_holo.hip: "bit-reproducible") where a line spans four waves and the sums go through LDS."""
    c = HM.case(*shape, HM.FIELDS[shape])
    a, b = launch(ctx, c), launch(ctx, c)
    assert a['loss'] == b['loss']
    for k in KEYS:
        same_bits(a[k], b[k], (ident(shape), k))
    sh = HM.case(*shape, HM.FIELDS[shape], shifts=True)
    a, b = (launch(ctx, sh, shifted=True, want=('probe', 'shifts')) for _ in range(2))
    for k in KEYS + ('target',):
        same_bits(a[k], b[k], (ident(shape), 'shifted', k))


if __name__ == '__main__':      # the CPU time of the module's oracle pairs, and the band conditions from the oracle pair alone
    total = 0.
    for shape, nd in HM.FIELDS.items():
        t = time.time()
        c = HM.case(*shape, nd)
        dt = time.time() - t
        total += dt
        print('%-10s nd %2d  %5.2f s  %s' % (ident(shape), nd, dt, HM.oracle_conditions(c)), flush=True)
        if shape in HM.SPECTRUM_FIELDS:
            t = time.time()
            c = HM.case(*shape, nd, probe='plane', broadband=True)
            total += time.time() - t
            print('%-10s spectrum     %s' % (ident(shape), HM.oracle_conditions(c, spectral=True)), flush=True)
        if shape in HM.SHIFT_FIELDS:
            t = time.time()
            c = HM.case(*shape, nd, shifts=True)
            total += time.time() - t
            print('%-10s shifts       %s' % (ident(shape), HM.oracle_conditions(c)), flush=True)
    for name, (ckw, _, k4) in HM.VARIANTS.items():
        for shape in (HM.VARIANT_FIELD,) + ((HM.VARIANT_FIELD_K4,) if k4 else ()):
            t = time.time()
            HM.case(*shape, HM.FIELDS[shape], **ckw)
            total += time.time() - t
    print('oracle pairs of the module: %.1f s' % total)
