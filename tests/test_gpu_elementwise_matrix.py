"""The element-wise matrix (pytest -m gpu): the optimiser steps of adm_optim.h / adm_optimize.hip and the regularisers of
adm_regularize.hip through the C ABI, against references that do not come from the library.  Tables, inputs, mirrors and
references are in tests/ew_matrix.py; tests/test_elementwise_coverage.py (CPU) holds the tables to the sources.

  optimiser steps   x, m, v equal a float32 NumPy mirror (the oracle in float32 + O.apply_constraints) as uint32 views; x is within
                    2e-6 (relative L2) of the same oracle in fp64; every word outside [lo, hi) keeps its seeded bits.  All 8 flag
                    combinations x mask x {Adam, GD, momentum}; odd and even range ends, lengths around one workgroup, empty
                    ranges, 4096 x 256 + 257 elements; i_batch 0 ... 100000; adm_axpy with a = 1 (bits) and a = -0.375 (1 ulp).
  small Adam        one call with ADM_SMALL_PARAMS_MAX arrays (one element, 2 x 2048, 17 x 256, a pin across chunks, both drift
                    guards with a pin), reversed, and with a zero-length array in the middle: x, g, m, v of every array as bits
                    against Adam mirror -> center_rows_mirror -> pin -> zero fill; the host refusals with their messages.
  delta_beta        the relations and the fp64 comparison of tests/test_gpu_elementwise.py at Z = 257 and 300 (the second trip of
                    the z loop), 95 / 191 / 192 (reg_threads' thresholds), 33 x 32 rows (the second trip of the value reduction),
                    adm_reg_grad_range with both ends in the second trip.
  real_imag         gradient (set, and add into a seeded buffer minus the seed), value and reproducibility against the fp64 oracle
                    on a lattice object, 1 ... 1 058 840 voxels; reweighted L1 weights, gradient and value on both unknown types.
"""
import numpy as np
import pytest

from tests import ew_matrix as EM
from tests import test_gpu_elementwise as E

pytestmark = pytest.mark.gpu


@pytest.fixture(scope='module')
def A():
    import adorym_amd
    return adorym_amd


@pytest.fixture(scope='module')
def ctx(A):
    c = A.Context(0)
    yield c
    c.close()


@pytest.fixture(scope='module')
def plans(A, ctx):
    """Plan handle of (shape, unknown_type), built once."""
    engines = {}

    def get(shape, unknown_type='delta_beta'):
        key = (tuple(shape), unknown_type)
        if key not in engines:
            engines[key] = A.MultisliceEngine(ctx, shape, (12, 12), np.array([(0, 0)]), 5000., 1e-7, unknown_type=unknown_type)
        return engines[key].plan.handle
    return get


check, bits, same_bits = E.check, EM.bits, E.same_bits


# ---- 1. optimiser steps ---------------------------------------------------------------------------------------------------------
_inputs = {}


def inputs_of(n):
    if n not in _inputs:
        _inputs[n] = EM.opt_inputs(n)
    return _inputs[n]


def launch_step(ctx, opt, d, lo, hi, flags, mask, i_batch):
    h, lib = EM.HYPER, ctx.lib
    mp = mask.ptr if mask is not None else None
    if opt == 'adam':
        return lib.adm_adam_step(ctx.handle, d['x'].ptr, d['g'].ptr, d['m'].ptr, d['v'].ptr, lo, hi, i_batch, h['step'], h['b1'], h['b2'],
                                 h['eps'], flags, mp)
    if opt == 'momentum':
        return lib.adm_momentum_step(ctx.handle, d['x'].ptr, d['g'].ptr, d['v'].ptr, lo, hi, h['step'], h['gamma'], flags, mp)
    return lib.adm_gd_step(ctx.handle, d['x'].ptr, d['g'].ptr, lo, hi, h['step'], flags, mp)


@pytest.mark.parametrize('case', EM.OPT_CASES, ids=EM.case_id)
def test_optimiser_step(ctx, case):
    opt, n, lo, hi, flags, with_mask, i_batch = case
    inp = inputs_of(n)
    d = {k: ctx.array(inp[k]) for k in ('x', 'g', 'm', 'v')}
    mask = ctx.array(inp['mask']) if with_mask else None
    check(launch_step(ctx, opt, d, lo, hi, flags, mask, i_batch))
    got = {k: d[k].get() for k in ('x', 'g', 'm', 'v')}
    mirror = EM.step_reference(opt, inp, lo, hi, flags, with_mask, i_batch, np.float32)
    ref = EM.step_reference(opt, inp, lo, hi, flags, with_mask, i_batch, np.float64)
    e = np.arange(n)
    inside = (e >= lo) & (e < hi)
    for k in ('x', 'g', 'm', 'v'):                          # what the step does not own keeps its seeded bits
        same_bits(got[k][~inside], inp[k][~inside], '%s outside [%d, %d)' % (k, lo, hi))
        if k not in mirror:
            same_bits(got[k], inp[k], k + ' (not an output of this optimiser)')
    for k in ('m', 'v', 'x'):
        if k in mirror:
            same_bits(got[k], mirror[k], k + ' vs the float32 mirror')
    err, e32 = EM.rel(got['x'], ref['x']), EM.rel(mirror['x'], ref['x'])
    print('x vs fp64: %.3e (the float32 oracle: %.3e), bar 2e-6' % (err, e32))
    assert err < 2e-6
    if inside.any():
        assert (bits(got['x'])[inside] != bits(inp['x'])[inside]).any()
        still = [i for i in inp['still'] if lo <= i < hi]
        if still:                                           # g = m = v = 0: a zero step; x keeps its bits apart from the constraints
            kept = EM.constrain_mirror(inp['x'], flags, inp['mask'] if with_mask else None)
            same_bits(got['x'][still], kept[still], 'x where g = m = v = 0')


@pytest.mark.parametrize('a,n', EM.AXPY_CASES)
def test_axpy(ctx, a, n):
    x, y = EM.seeded(n, 61), EM.seeded(n, 62)
    d_x, d_y = ctx.array(x), ctx.array(y)
    check(ctx.lib.adm_axpy(ctx.handle, d_y.ptr, d_x.ptr, a, n))
    got = d_y.get()
    same_bits(d_x.get(), x, 'x is read only')
    if a == 1.0:
        same_bits(got, y + x, 'y + 1 * x')                  # 1 * x is exact, contracted or not: one rounding
        return
    ref = y.astype(np.float64) + a * x.astype(np.float64)   # a = -3/8: the product is exact in fp64
    ulp = np.spacing(np.abs(ref).astype(np.float32)).astype(np.float64)
    worst = float(np.max(np.abs(got.astype(np.float64) - ref) / ulp))
    print('axpy a = %g, n = %d: worst error %.3f ulp' % (a, n, worst))
    assert worst <= 1.0


# ---- 2. adm_adam_step_small -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('call', list(EM.SMALL_CALLS))
def test_small_adam_with_the_most_arrays_of_one_call(ctx, call):
    from adorym_amd._lib import SmallParam
    order = EM.SMALL_CALLS[call]
    assert len(order) == EM.SMALL_PARAMS_MAX
    arr = (SmallParam * len(order))()
    held = []
    for pos, k in enumerate(order):
        spec = k if isinstance(k, dict) else EM.SMALL_ARRAYS[k]
        inp = EM.small_inputs(pos if isinstance(k, dict) else k, spec)
        zero_grad = pos % 2
        d = {name: ctx.array(inp[name] if spec['n'] else np.zeros(1, np.float32)) for name in ('x', 'g', 'm', 'v')}
        d_pin = ctx.array(inp['pin']) if spec['pin_n'] else None
        arr[pos] = SmallParam(x=d['x'].ptr, g=d['g'].ptr, m=d['m'].ptr, v=d['v'].ptr, n=spec['n'], step_size=spec['step'],
                              center_cols=spec['center_cols'], zero_grad=zero_grad, pin=d_pin.ptr if d_pin else None, pin_n=spec['pin_n'])
        held.append((spec, inp, zero_grad, d, d_pin))
    h = EM.HYPER
    check(ctx.lib.adm_adam_step_small(ctx.handle, arr, len(order), EM.SMALL_I_BATCH, h['b1'], h['b2'], h['eps']))
    for pos, (spec, inp, zero_grad, d, d_pin) in enumerate(held):
        if not spec['n']:
            for name in ('x', 'g', 'm', 'v'):
                same_bits(d[name].get(), np.zeros(1, np.float32), 'array %d (empty), %s' % (pos, name))
            continue
        want = EM.small_mirror(spec, inp, zero_grad)
        for name in ('x', 'g', 'm', 'v'):
            same_bits(d[name].get(), want[name], 'array %d (n = %d, center_cols = %d, pin_n = %d), %s'
                      % (pos, spec['n'], spec['center_cols'], spec['pin_n'], name))
        if d_pin:
            same_bits(d_pin.get(), inp['pin'], 'the pin is read only')
        assert (bits(want['x']) != bits(inp['x'])).any()


def test_small_adam_refusals(ctx):
    from adorym_amd._lib import SmallParam, ADM_ERR_INVALID
    lib, h = ctx.lib, EM.HYPER
    x0 = EM.seeded(12, 70)
    d = [ctx.array(x0) for _ in range(5)]

    def refused(count, message, **kw):
        arr = (SmallParam * count)()
        for k in range(count):
            f = dict(x=d[0].ptr, g=d[1].ptr, m=d[2].ptr, v=d[3].ptr, n=12, step_size=1e-2, center_cols=0, zero_grad=1, pin=None, pin_n=0)
            f.update(kw)
            arr[k] = SmallParam(**f)
        rc = lib.adm_adam_step_small(ctx.handle, arr, count, 3, h['b1'], h['b2'], h['eps'])
        assert rc == ADM_ERR_INVALID and lib.adm_last_error().decode() == message, (rc, lib.adm_last_error())
    refused(EM.SMALL_PARAMS_MAX + 1, 'adm_adam_step_small: too many arrays in one call')
    refused(1, 'adm_adam_step_small: n is not a multiple of center_cols', center_cols=5)
    refused(1, 'adm_adam_step_small: pin_n exceeds n', pin=d[4].ptr, pin_n=13)
    ctx.sync()
    for a in d:                                            # a refused call launches nothing
        same_bits(a.get(), x0, 'arrays of a refused call')


# ---- 3. delta_beta regulariser --------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('alphas', EM.DB_ALPHAS)
@pytest.mark.parametrize('shape', EM.DB_SHAPES)
def test_delta_beta_launch_shapes(ctx, plans, shape, alphas):
    """The relations and the fp64 comparison of tests/test_gpu_elementwise.py (bars unchanged: gradient 1e-6 relative L2, value
    1e-5).  The inputs are float32 and the kernel only subtracts them, so the fp64 signs are the kernel's: no voxel is excluded."""
    E.test_delta_beta_set_add_and_value_are_one_computation(ctx, plans, shape, alphas)
    E.test_delta_beta_vs_fp64(ctx, plans, shape, alphas)


@pytest.mark.parametrize('window', list(EM.DB_WINDOWS))
@pytest.mark.parametrize('alphas', EM.DB_ALPHAS)
def test_delta_beta_range_in_the_second_trip(ctx, plans, alphas, window):
    shape = EM.DB_RANGE_SHAPE
    r = E.Reg.of(ctx, plans, shape, alphas)
    gref, _ = E.l1_tv_fp64(r.obj, *alphas)
    assert EM.rel(r.set_g, gref) < 1e-6
    (lo, hi), (a_lo, a_hi) = EM.DB_RANGE, EM.DB_WINDOWS[window]
    n, plane, row = r.obj.size, 2 * shape[1] * shape[2], 2 * shape[2]
    assert lo % 2 == 1 and hi % 2 == 1 and 0 < lo < hi < n and lo % plane and hi % plane
    assert (lo % row) // 2 >= 256 and (hi % row) // 2 >= 256            # both ends at a z of the second trip
    d_obj, d_g = ctx.array(r.obj), ctx.array(r.g0)
    check(ctx.lib.adm_reg_grad_range(plans(shape), d_obj.ptr, alphas[0], alphas[1], alphas[2], d_g.ptr, lo, hi, a_lo, a_hi))
    e = np.arange(n)
    inside = (e >= lo) & (e < hi)
    added = inside & (e >= a_lo) & (e < a_hi)
    want = np.where(added, r.add_g.reshape(-1), np.where(inside, r.set_g.reshape(-1), r.g0.reshape(-1)))
    assert (~inside).sum() > 0 and (added.sum() > 0) == (window != 'empty') and ((inside & ~added).sum() > 0) == (window != 'everything')
    same_bits(d_g.get().reshape(-1), want, 'range [%d, %d), add window %s' % (lo, hi, window))


# ---- 4. real_imag regularisers --------------------------------------------------------------------------------------------------
_lattice = {}


def lattice(shape, reweighted=False):
    """(object, figures of its guards), generated and checked on the host once per shape."""
    key = (shape, reweighted)
    if key not in _lattice:
        obj = EM.lattice_object(shape, reweighted=reweighted)
        assert reweighted or (obj.astype(np.float64) ** 2).sum(-1).min() >= 0.25          # |o| >= 1/2
        _lattice[key] = (obj, EM.lattice_conditions(obj))
    return _lattice[key]


@pytest.mark.parametrize('shape,alphas', EM.RI_CASES, ids=EM.case_id)
def test_real_imag_vs_fp64(ctx, plans, shape, alphas):
    obj, fig = lattice(shape)
    print('lattice guards:', fig)
    assert fig['phase_ties_apart'] == 0
    gref, vref = EM.ri_reference(obj, alphas, np.float64)
    g32, v32 = EM.ri_reference(obj, alphas, np.float32)
    e32 = EM.rel(g32, gref)
    bar = EM.grad_bar(1e-6, e32)
    # the seed of the accumulating launch: the gradient's own scale (a power of two), so that g0 + gradient rounds at 2^-24 of the
    # gradient and (g0 + gradient) - g0, formed in fp64, is the gradient to 6e-8
    scale = np.exp2(np.round(np.log2(np.abs(gref).max()))) if np.abs(gref).max() > 0 else 1.0
    g0 = (EM.seeded(obj.shape, 5, -2, 0) * scale).astype(np.float32)
    plan, lib = plans(shape, 'real_imag'), ctx.lib
    d_obj = ctx.array(obj)

    def run(fn, g_init):
        d_g, d_v = ctx.array(g_init), ctx.zeros((1,))
        check(fn(plan, d_obj.ptr, alphas[0], alphas[1], alphas[2], d_g.ptr, d_v.ptr))
        return d_g.get(), float(d_v.get()[0])
    set_g, set_v = run(lib.adm_reg_grad_set, g0)
    add_g, add_v = run(lib.adm_reg_grad, g0)
    again_g, _ = run(lib.adm_reg_grad_set, g0)
    same_bits(d_obj.get(), obj, 'the object is read only')
    gmax = np.abs(gref).max()
    for what, g, v in (('set', set_g.astype(np.float64), set_v), ('add - seed', add_g.astype(np.float64) - g0.astype(np.float64), add_v)):
        err, worst = EM.rel(g, gref), float(np.abs(g - gref).max())
        print('%s: gradient %.3e of the norm (float32 oracle %.3e, bar %.3e), max|diff| %.3e of max|ref|; value %.9e vs %.9e'
              % (what, err, e32, bar, worst / gmax if gmax else worst, v, vref))
        if gmax == 0:                                      # TV alone on one voxel: zero in fp64 must be zero
            assert not g.any()
        else:
            assert err < bar
            assert worst < 1e-5 * gmax
        assert abs(v - vref) <= 1e-5 * abs(vref)
    same_bits(again_g, set_g, 'a second identical launch')


def rwl1_inputs(shape):
    obj, fig = lattice(shape, reweighted=True)
    assert np.abs(obj).min() >= 1 / 64 and obj.mean() > 0 and obj[..., 0].min() >= 0.25
    w64 = EM.rwl1_weight_reference(obj, np.float64)
    assert w64.max() / w64.min() < 2 ** 8.5
    return obj, w64


@pytest.mark.parametrize('unknown_type', EM.UNKNOWN_TYPES)
@pytest.mark.parametrize('shape', EM.RWL1_SHAPES, ids=EM.case_id)
def test_reweighted_l1_weights_vs_fp64(ctx, plans, shape, unknown_type):
    obj, w64 = rwl1_inputs(shape)
    nb = min(EM.stream_grid(obj.size), EM.BLOCK_CAP)
    d_obj, d_w, d_s = ctx.array(obj), ctx.array(EM.seeded(obj.shape, 6)), ctx.zeros((2 * nb + 2,))
    check(ctx.lib.adm_rwl1_update(plans(shape, unknown_type), d_obj.ptr, d_w.ptr, d_s.ptr))
    err, e32 = EM.rel(d_w.get(), w64), EM.rel(EM.rwl1_weight_reference(obj, np.float32), w64)
    print('weights: %.3e of the norm (float32 oracle %.3e), bar 2e-6; %d blocks of partials' % (err, e32, nb))
    assert err < 2e-6
    same_bits(d_obj.get(), obj, 'the object is read only')


@pytest.mark.parametrize('unknown_type', EM.UNKNOWN_TYPES)
@pytest.mark.parametrize('shape', EM.RWL1_SHAPES, ids=EM.case_id)
def test_reweighted_l1_gradient_vs_fp64(ctx, plans, shape, unknown_type):
    obj, w64 = rwl1_inputs(shape)
    w = w64.astype(np.float32)                              # non-unit weights, the same floats for the kernel and both oracles
    gref, vref = EM.rwl1_reference(obj, w, unknown_type, np.float64)
    g32, _ = EM.rwl1_reference(obj, w, unknown_type, np.float32)
    e32 = EM.rel(g32, gref)
    bar = EM.grad_bar(2e-6, e32)
    d_obj, d_w, d_g, d_v = ctx.array(obj), ctx.array(w), ctx.zeros(obj.shape), ctx.zeros((1,))
    check(ctx.lib.adm_reg_grad_weighted(plans(shape, unknown_type), d_obj.ptr, d_w.ptr, EM.RWL1_ALPHAS[0], EM.RWL1_ALPHAS[1], d_g.ptr, d_v.ptr))
    err, v = EM.rel(d_g.get(), gref), float(d_v.get()[0])
    print('gradient: %.3e of the norm (float32 oracle %.3e, bar %.3e); value %.9e vs %.9e' % (err, e32, bar, v, vref))
    assert err < bar
    assert abs(v - vref) <= 1e-5 * abs(vref)
