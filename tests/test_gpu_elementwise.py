"""The element-wise kernels -- the regularisers (adm_regularize.hip) and the optimiser steps with a drift guard (adm_optimize.hip)
-- called through the C ABI (pytest -m gpu).  Except for the comparison with an fp64 NumPy L1 + TV, every assertion is a relation
between two results of the library, or between a result and a float32 NumPy mirror of its order of additions, that arithmetic
guarantees BIT FOR BIT: equalities of uint32 views, no tolerance.

  delta_beta   adm_reg_grad_set = adm_reg_grad into zeros; adm_reg_grad into g0 = g0 + set (one rounding per element); the value
               beside set, beside add and alone is the same float and is ADDED to what the scalar held; gradient and value agree with
               fp64 within the bounds of tests/test_gpu_parity.py::test_reg_grad_vs_reference; adm_reg_grad_range writes its range
               only, adding inside the add window and writing elsewhere.
  real_imag    one workgroup (V <= 256: the value's atomic add has one contribution): set = add into zeros;
               adm_reg_grad_weighted with weights 1 + 0i = adm_reg_grad with gamma = 0.
  drift guard  adm_center_rows against a mirror of block_sum_f32 (adm_block_sum.h): rows t, t + 256, ... per thread, the tree
               32 ... 1 inside each wave of 64, the waves ascending; adm_adam_step_small = adm_adam_step + adm_center_rows on both
               sides of its register-resident limit.

Shapes: every wrap of the periodic neighbours (extent 1 and 2), a partial wave, the 64-, 128- and 256-thread launches of the row
kernels.  The whole module takes a few seconds.
"""
import numpy as np
import pytest

from tests.ew_matrix import block_sum_mirror, center_rows_mirror          # noqa: F401 (the mirrors of block_sum_f32's order)

pytestmark = pytest.mark.gpu

SHAPES = [(1, 1, 1), (3, 4, 5), (2, 3, 96), (2, 2, 200)]
ALPHAS = [(.7, .3, 0.), (0., 0., .5), (.7, .3, .5)]


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
    """Plan handle of (shape, unknown_type), built once (like tests/test_gpu_parity.py::test_reg_grad_vs_reference builds its own)."""
    engines = {}

    def get(shape, unknown_type='delta_beta'):
        key = (tuple(shape), unknown_type)
        if key not in engines:
            engines[key] = A.MultisliceEngine(ctx, shape, (12, 12), np.array([(0, 0)]), 5000., 1e-7, unknown_type=unknown_type)
        return engines[key].plan.handle
    return get


def check(rc):
    from adorym_amd._lib import check as c
    c(rc)


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def same_bits(got, ref, what):
    d = bits(got) != bits(ref)
    n = int(d.sum())
    print('%s: %d of %d words differ' % (what, n, d.size))
    assert n == 0, (what, n, [tuple(int(v) for v in i) for i in np.argwhere(d)[:4]])


def db_object(shape, seed=3):
    r = np.random.default_rng(seed)
    return (r.standard_normal(tuple(shape) + (2,)) * np.array([1e-3, 1e-4])).astype(np.float32)


def seeded(shape, seed):
    """Non-zero values of mixed sign spread over a few binades."""
    r = np.random.default_rng(seed)
    return (r.standard_normal(shape) * np.exp2(r.integers(-6, 3, shape))).astype(np.float32)


def l1_tv_fp64(obj, ad, ab, gm):
    """alpha_c * mean|x_c| + gamma * sum_axes sum|roll(a, 1) - a| / V and its (sub)gradient, float64."""
    x = np.asarray(obj, np.float64)
    V = x[..., 0].size
    grad = np.zeros_like(x)
    val = 0.0
    for c, a in ((0, ad), (1, ab)):
        grad[..., c] += a * np.sign(x[..., c]) / V
        val += a * np.abs(x[..., c]).sum() / V
    for ax in range(3):
        back, fwd = np.roll(x, 1, ax), np.roll(x, -1, ax)
        val += gm * np.abs(back - x).sum() / V
        grad += gm * (np.sign(x - fwd) - np.sign(back - x)) / V
    return grad, val


class Reg(object):
    """The three forms of the delta_beta regulariser on one object, each run once and shared by the tests below."""
    cache = {}

    def __init__(self, ctx, plan, shape, alphas):
        self.obj = db_object(shape)
        self.g0 = seeded(self.obj.shape, 5)
        self.v0 = np.float32(0.375)
        lib, d_obj = ctx.lib, ctx.array(self.obj)
        ad, ab, gm = alphas

        def run(fn, g_init, v_init):
            d_g = ctx.array(g_init) if g_init is not None else None
            d_v = ctx.array(np.array([v_init], np.float32))
            check(fn(plan, d_obj.ptr, ad, ab, gm, d_g.ptr if d_g is not None else None, d_v.ptr))
            return (d_g.get() if d_g is not None else None), d_v.get()[0]
        zeros = np.zeros_like(self.obj)
        self.set_g, self.set_v = run(lib.adm_reg_grad_set, self.g0, 0.)          # (over a seeded buffer: set ignores what it held)
        self.add0_g, self.add0_v = run(lib.adm_reg_grad, zeros, 0.)
        self.add_g, self.add_v = run(lib.adm_reg_grad, self.g0, 0.)
        _, self.only_v = run(lib.adm_reg_grad, None, 0.)
        _, self.seeded_v = run(lib.adm_reg_grad, None, self.v0)

    @classmethod
    def of(cls, ctx, plans, shape, alphas):
        key = (shape, alphas)
        if key not in cls.cache:
            cls.cache[key] = cls(ctx, plans(shape), shape, alphas)
        return cls.cache[key]


@pytest.mark.parametrize('alphas', ALPHAS)
@pytest.mark.parametrize('shape', SHAPES)
def test_delta_beta_set_add_and_value_are_one_computation(ctx, plans, shape, alphas):
    r = Reg.of(ctx, plans, shape, alphas)
    same_bits(r.set_g, r.add0_g, 'set vs add into zeros')
    same_bits(r.add_g, r.g0 + r.set_g, 'add vs g0 + set')                  # float32 + float32: one rounding
    for what, v in (('beside add into zeros', r.add0_v), ('beside add', r.add_v), ('alone', r.only_v)):
        same_bits(v, r.set_v, 'value ' + what)
    same_bits(r.seeded_v, r.v0 + np.float32(r.set_v), 'value added to a seeded scalar')


@pytest.mark.parametrize('alphas', ALPHAS)
@pytest.mark.parametrize('shape', SHAPES)
def test_delta_beta_vs_fp64(ctx, plans, shape, alphas):
    """The bounds of tests/test_gpu_parity.py::test_reg_grad_vs_reference: relative L2 error of the gradient below 1e-6, the value
    within 1e-5 of its magnitude (a gradient that is zero in fp64 -- TV alone on one voxel -- must be zero)."""
    r = Reg.of(ctx, plans, shape, alphas)
    gref, vref = l1_tv_fp64(r.obj, *alphas)
    err, nref = np.linalg.norm(r.set_g.astype(np.float64) - gref), np.linalg.norm(gref)
    print('gradient: |err| %.3e, |ref| %.3e; value %.9e vs %.9e' % (err, nref, r.set_v, vref))
    assert err < 1e-6 * nref or (nref == 0 and err == 0)
    assert abs(float(r.set_v) - vref) <= 1e-5 * abs(vref)


RANGE_SHAPE = (3, 4, 5)             # 120 floats, planes of 40
RANGE = (7, 93)                     # odd, odd: begins and ends on a beta element, cuts the first and the last plane
WINDOWS = {'empty': (0, 0), 'interior': (21, 60), 'everything': (0, 120)}


@pytest.mark.parametrize('window', list(WINDOWS))
@pytest.mark.parametrize('alphas', ALPHAS)
def test_range_adds_inside_the_window_and_writes_elsewhere(ctx, plans, alphas, window):
    r = Reg.of(ctx, plans, RANGE_SHAPE, alphas)
    plan, lib = plans(RANGE_SHAPE), ctx.lib
    d_obj = ctx.array(r.obj)
    (lo, hi), (a_lo, a_hi) = RANGE, WINDOWS[window]
    n = r.obj.size
    assert lo % 2 == 1 and hi % 2 == 1 and 0 < lo < hi < n and lo % 40 and hi % 40          # odd ends inside planes
    if window == 'interior':
        assert lo < a_lo < a_hi < hi

    def run(lo, hi):
        d_g = ctx.array(r.g0)
        check(lib.adm_reg_grad_range(plan, d_obj.ptr, alphas[0], alphas[1], alphas[2], d_g.ptr, lo, hi, a_lo, a_hi))
        return d_g.get().reshape(-1)
    got = run(lo, hi)
    e = np.arange(n)
    inside = (e >= lo) & (e < hi)
    added = inside & (e >= a_lo) & (e < a_hi)
    want = np.where(added, r.add_g.reshape(-1), np.where(inside, r.set_g.reshape(-1), r.g0.reshape(-1)))
    print('%s: %d added, %d written, %d untouched' % (window, added.sum(), (inside & ~added).sum(), (~inside).sum()))
    assert (~inside).sum() > 0 and (added.sum() > 0) == (window != 'empty') and ((inside & ~added).sum() > 0) == (window != 'everything')
    same_bits(got, want, 'range [%d, %d), add window %s' % (lo, hi, window))
    # an empty range changes nothing; an end beyond the object is clipped
    same_bits(run(hi, lo), r.g0.reshape(-1), 'lo >= hi')
    same_bits(run(lo, lo), r.g0.reshape(-1), 'lo == hi')
    inside = e >= lo
    added = inside & (e >= a_lo) & (e < a_hi)
    want = np.where(added, r.add_g.reshape(-1), np.where(inside, r.set_g.reshape(-1), r.g0.reshape(-1)))
    same_bits(run(lo, n + 50), want, 'hi beyond the object')


def ri_object(shape, seed=9):
    r = np.random.default_rng(seed)
    mag, ph = 1 + 0.2 * r.standard_normal(shape), r.uniform(-1.5, 1.5, shape)
    return np.stack([mag * np.cos(ph), mag * np.sin(ph)], -1).astype(np.float32)


@pytest.mark.parametrize('alphas', ALPHAS)
@pytest.mark.parametrize('shape', [(3, 4, 5), (4, 8, 8)])
def test_real_imag_set_equals_add_into_zeros(ctx, plans, shape, alphas):
    assert np.prod(shape) <= 256                       # one workgroup: the value is one atomic add onto the scalar
    plan, lib = plans(shape, 'real_imag'), ctx.lib
    obj = ri_object(shape)
    d_obj = ctx.array(obj)
    out = []
    for fn, g_init in ((lib.adm_reg_grad_set, seeded(obj.shape, 5)), (lib.adm_reg_grad, np.zeros_like(obj))):
        d_g, d_v = ctx.array(g_init), ctx.zeros((1,))
        check(fn(plan, d_obj.ptr, alphas[0], alphas[1], alphas[2], d_g.ptr, d_v.ptr))
        out.append((d_g.get(), d_v.get()))
    assert np.isfinite(out[0][0]).all() and np.abs(out[0][0]).max() > 0
    same_bits(out[0][0], out[1][0], 'real_imag set vs add into zeros')
    same_bits(out[0][1], out[1][1], 'real_imag value')


@pytest.mark.parametrize('alphas', [(.7, .3), (.7, 0.), (0., .3)])
@pytest.mark.parametrize('shape', [(3, 4, 5), (4, 8, 8)])
def test_real_imag_unit_weights_are_the_unweighted_l1(ctx, plans, shape, alphas):
    """wm = 1 * 1 + 0 * 0 = 1 exactly, and a product with 1 is exact: the reweighted L1 with unit weights makes the additions of the
    plain L1 in the same order."""
    assert np.prod(shape) <= 256
    plan, lib = plans(shape, 'real_imag'), ctx.lib
    obj = ri_object(shape)
    g0 = seeded(obj.shape, 5)
    w = np.zeros_like(obj)
    w[..., 0] = 1
    d_obj, d_w = ctx.array(obj), ctx.array(w)
    d_g, d_v = ctx.array(g0), ctx.zeros((1,))
    check(lib.adm_reg_grad(plan, d_obj.ptr, alphas[0], alphas[1], 0., d_g.ptr, d_v.ptr))
    d_gw, d_vw = ctx.array(g0), ctx.zeros((1,))
    check(lib.adm_reg_grad_weighted(plan, d_obj.ptr, d_w.ptr, alphas[0], alphas[1], d_gw.ptr, d_vw.ptr))
    assert (bits(d_g.get()) != bits(g0)).any() and d_v.get()[0] != 0
    same_bits(d_gw.get(), d_g.get(), 'weighted (1 + 0i) vs plain, gradient')
    same_bits(d_vw.get(), d_v.get(), 'weighted (1 + 0i) vs plain, value')


# ---- the drift guard ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('n_cols', [1, 2, 3])
@pytest.mark.parametrize('n_rows', [1, 63, 64, 257, 1000])
def test_center_rows_is_the_mirrored_sum(ctx, n_rows, n_cols):
    x = seeded((n_rows, n_cols), 100 + n_rows)
    d_x = ctx.array(x)
    check(ctx.lib.adm_center_rows(ctx.handle, d_x.ptr, n_rows, n_cols))
    ref = center_rows_mirror(x)
    if n_rows == 1000:                                 # the test can see an order change: the waves added backwards give other bits
        assert (bits(center_rows_mirror(x, descending=True)) != bits(ref)).any()
    same_bits(d_x.get(), ref, 'center_rows %d x %d' % (n_rows, n_cols))


@pytest.mark.parametrize('center_cols', [1, 2])
@pytest.mark.parametrize('n_rows', [1, 255, 2048, 2049])         # 2048 rows: the register-resident limit; 2049: the generic path
def test_small_adam_with_drift_guard_is_adam_then_center_rows(ctx, n_rows, center_cols):
    from adorym_amd._lib import SmallParam
    n = n_rows * center_cols
    x, g, m = seeded(n, 1), seeded(n, 2), seeded(n, 3)
    v = np.abs(seeded(n, 4))
    i_batch, step, b1, b2, eps = 3, 1e-2, 0.9, 0.999, 1e-7
    lib = ctx.lib
    a = [ctx.array(h) for h in (x, g, m, v)]
    check(lib.adm_adam_step(ctx.handle, a[0].ptr, a[1].ptr, a[2].ptr, a[3].ptr, 0, n, i_batch, step, b1, b2, eps, 0, None))
    check(lib.adm_center_rows(ctx.handle, a[0].ptr, n_rows, center_cols))
    s = [ctx.array(h) for h in (x, g, m, v)]
    arr = (SmallParam * 1)()
    arr[0] = SmallParam(x=s[0].ptr, g=s[1].ptr, m=s[2].ptr, v=s[3].ptr, n=n, step_size=step, center_cols=center_cols, zero_grad=0,
                        pin=None, pin_n=0)
    check(lib.adm_adam_step_small(ctx.handle, arr, 1, i_batch, b1, b2, eps))
    assert (bits(a[0].get()) != bits(x)).any()
    for k, what in enumerate(('x', 'g', 'm', 'v')):
        same_bits(s[k].get(), a[k].get(), 'small Adam vs Adam + center_rows, %s (%d x %d)' % (what, n_rows, center_cols))
