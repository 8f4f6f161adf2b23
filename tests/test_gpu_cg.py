"""The conjugate-gradient kernels (adm_cg.hip) through the C ABI, and CGOptimizer.apply_gradient step by step against tests/cg_ref.py.
Bars and sizes: tests/cg_matrix.py.

Kernels, at n = 1 ... 2^20 + 3 and on views that start at an odd element: every sum against NumPy's float64 sum of the same float32
inputs within 1e-12 sum |terms|; beta from those sums; s_new, x_trial within a fused multiply-add of NumPy's float32; d_old bit-equal
to -g; the accepted point bit-equal to adm_gd_step's constraints (step 0) at every flag combination with and without a mask; two
calls bit-equal; the branches i_batch = 0, A < 0, B = 0, C >= 0.

Optimiser: through the driver, every update of golden F33's runs restarted from the state the fp64 restatement holds there (object,
gradient and the two state arrays, rounded to float32): the same decisions, alpha and beta within 3 x the reference's own fp32
distance for that quantity, every trial loss within 3 x the stored fp32-fp64 trial-loss distance."""
import os

import numpy as np
import pytest

import cases
from tests import cg_matrix as CM
from tests import cg_ref as R

pytestmark = pytest.mark.gpu
G = os.path.join(os.path.dirname(__file__), 'golden')


@pytest.fixture(scope='module')
def ctx():
    import adorym_amd as A
    c = A.Context(0)
    yield c
    c.close()


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def put(ctx, host, off=0):
    """host (float32) on the device, starting ``off`` elements into its allocation; returns (owner, view)."""
    host = np.ascontiguousarray(host, np.float32)
    own = ctx.zeros((host.size + off,))
    own.set(np.concatenate([np.zeros(off, np.float32), host.reshape(-1)]))
    return own, own.view(off, (host.size,))


class Sums(object):
    def __init__(self, ctx):
        from adorym_amd import _lib
        from adorym_amd.device import MappedArray
        self.ctx, self.L = ctx, _lib
        self.scratch = ctx.empty((_lib.CG_SCRATCH_DOUBLES,), np.float64)
        self.host = MappedArray(ctx, (8,), np.float64)

    def update(self, g, s, d_old, n, i_batch):
        """adm_cg_beta + adm_cg_direction -> the sums block (A, B, beta, C, E, D)."""
        L, ctx = self.L, self.ctx
        L.check(ctx.lib.adm_cg_beta(ctx.handle, g.ptr, d_old.ptr, n, i_batch, self.scratch.ptr, self.host.ptr))
        L.check(ctx.lib.adm_cg_direction(ctx.handle, g.ptr, s.ptr, d_old.ptr, n, self.scratch.ptr, self.host.ptr))
        return self.host.get()[:6]


def sum_ok(got, terms):
    terms = np.asarray(terms, np.float64)
    return abs(got - terms.sum()) <= CM.SUM_REL * np.abs(terms).sum()


def run_update(ctx, sums, inp, off, i_batch, alpha=0.375):
    n = inp['g'].size
    keep = [put(ctx, inp[k], off) for k in ('x', 'g', 's', 'd_old')]
    (_, x), (_, g), (_, s), (_, d_old) = keep
    v = sums.update(g, s, d_old, n, i_batch)
    xt_own, xt = put(ctx, np.zeros(n, np.float32), off)
    from adorym_amd._lib import check
    check(ctx.lib.adm_cg_trial(ctx.handle, x.ptr, s.ptr, alpha, xt.ptr, n))
    return v, s.get(), d_old.get(), xt.get()


# every size on aligned arrays; views that start 1 or 3 elements into an allocation (4-byte alignment only) at a subset
CASES = [(n, 0) for n in CM.SIZES] + [(n, off) for off in (1, 3) for n in (1, 65, 1025, 2 * 16 ** 3, 2 ** 20 + 3)]


@pytest.mark.parametrize('n,off', CASES)
def test_sums_direction_and_trial(ctx, n, off):
    inp = CM.kernel_inputs(n, seed=n % 97)
    sums = Sums(ctx)
    v, s_new, d_new, xt = run_update(ctx, sums, inp, off, i_batch=2)
    A, B, beta, C, E, D = v
    g64, o64, s64 = (inp[k].astype(np.float64) for k in ('g', 'd_old', 's'))
    d64 = -g64
    assert sum_ok(A, d64 * (d64 - o64)) and sum_ok(B, o64 * o64)
    want_beta = max(A / B, 0.) if B > 0 else 0.
    assert abs(beta - want_beta) <= 1e-15 * abs(want_beta)
    b32 = np.float32(beta)
    # the direction: within a fused multiply-add of NumPy's float32, d_old = -g exactly
    ref = -inp['g'] + b32 * inp['s']
    assert (np.abs(s_new.astype(np.float64) - ref) <= CM.FMA_ULP * (np.abs(g64) + np.abs(np.float64(b32) * s64))).all()
    assert (bits(d_new) == bits(-inp['g'])).all()
    sn64 = s_new.astype(np.float64)
    assert sum_ok(C, sn64 * g64) and sum_ok(E, sn64 * sn64) and sum_ok(D, g64 * g64)
    # the trial point, from the new direction
    a32 = np.float32(0.375)
    ref = inp['x'] + a32 * s_new
    assert (np.abs(xt.astype(np.float64) - ref) <= CM.FMA_ULP * (np.abs(inp['x'].astype(np.float64)) + np.abs(0.375 * sn64))).all()
    # the same inputs, the same bits
    v2, s2, d2, xt2 = run_update(ctx, sums, inp, off, i_batch=2)
    assert (v.view(np.uint64) == v2.view(np.uint64)).all()
    assert (bits(s2) == bits(s_new)).all() and (bits(d2) == bits(d_new)).all() and (bits(xt2) == bits(xt)).all()


def test_branches_of_beta_and_the_fallback(ctx):
    from adorym_amd._lib import check
    n = 4099
    inp = CM.kernel_inputs(n, seed=5)
    sums = Sums(ctx)
    d = -inp['g']
    # i_batch = 0: beta = 0 whatever the state holds
    v, s_new, _, _ = run_update(ctx, sums, inp, 0, i_batch=0)
    assert v[2] == 0. and v[1] > 0 and (bits(s_new) == bits(d + np.float32(0.) * inp['s'])).all()
    # A < 0 is clamped: d_old = 2 d gives A = -sum d^2
    v, s_new, _, _ = run_update(ctx, sums, dict(inp, d_old=2 * d), 0, i_batch=3)
    assert v[0] < 0 and v[1] > 0 and v[2] == 0.
    # B = 0: beta = 0, not a NaN
    v, s_new, _, _ = run_update(ctx, sums, dict(inp, d_old=np.zeros(n, np.float32)), 0, i_batch=3)
    assert v[1] == 0. and v[2] == 0. and np.isfinite(v).all() and np.isfinite(s_new).all()
    # C >= 0: d_old = d / 2 gives beta = 2, s = g gives s_new = g, so C = D > 0; the host then takes the fallback and df0 = -D
    crafted = dict(inp, d_old=(0.5 * d).astype(np.float32), s=inp['g'].copy())
    v, s_new, _, _ = run_update(ctx, sums, crafted, 0, i_batch=1)
    assert v[2] == 2.0 and v[3] > 0 and (bits(s_new) == bits(inp['g'])).all()
    assert sum_ok(v[5], inp['g'].astype(np.float64) ** 2) and abs(v[3] - v[5]) <= 1e-12 * v[5]
    (_, g_dev), (_, s_dev) = put(ctx, inp['g']), put(ctx, s_new)
    check(ctx.lib.adm_cg_fallback(ctx.handle, g_dev.ptr, s_dev.ptr, n))
    assert (bits(s_dev.get()) == bits(-inp['g'])).all()
    _, g1 = put(ctx, inp['g'], 1)
    _, s1 = put(ctx, s_new, 1)
    check(ctx.lib.adm_cg_fallback(ctx.handle, g1.ptr, s1.ptr, n))
    assert (bits(s1.get()) == bits(-inp['g'])).all()


def test_the_fallback_through_the_optimiser(ctx):
    """The crafted state above through CGOptimizer.apply_gradient with a host-side quadratic loss: the descent check fails, the
    search runs along -g with df0 = -D and |s| = sqrt(D)."""
    import adorym_amd as A
    n = 2 * 515

    class Quadratic(A.ForwardModel):
        def get_loss_function(self):
            def loss(obj):
                self.current_loss = float(0.5 * np.sum(obj.get().astype(np.float64) ** 2))
                return self.current_loss
            return loss

    x0 = CM.kernel_inputs(n, seed=9)['x']
    g = x0.copy()                               # the gradient of the quadratic
    fm = Quadratic(device=ctx)
    x = ctx.array(x0)
    fm.update_loss_args({'obj': x})
    fm.current_loss = float(0.5 * np.sum(x0.astype(np.float64) ** 2))
    opt = A.CGOptimizer('obj', options_dict={'step_size': 1.}, forward_model=fm)
    opt.create_container((n,), False, ctx)
    opt.params_whole_array_dict['descent_dir_old'].set(-0.5 * g)
    opt.params_whole_array_dict['s'].set(g)
    g_dev = ctx.array(g)
    opt.apply_gradient(x, g_dev, 1, **opt.options_dict)
    D = float(np.sum(g.astype(np.float64) ** 2))
    last = opt.last
    assert not last['descends'] and last['beta'] == 2.0 and last['descent_check'] > 0
    assert abs(last['df0'] + D) <= 1e-12 * D and abs(last['norm'] - np.sqrt(D)) <= 1e-12 * np.sqrt(D)
    assert (bits(opt.params_whole_array_dict['s'].get()) == bits(-g)).all()
    assert last['alpha'] > 0 and last['newf'] < last['f0'] and opt.i_line_search_step == last['step_count'] and opt.i_batch == 1
    # without a forward model: the reference's error
    with pytest.raises(ValueError, match='ForwardModel must be supplied'):
        A.CGOptimizer('obj').apply_gradient(x, g_dev, 0)


@pytest.mark.parametrize('with_mask', [False, True])
@pytest.mark.parametrize('flags', CM.FLAGS)
def test_accept_is_the_constraint_of_the_gd_step(ctx, flags, with_mask):
    from adorym_amd._lib import check
    for n, lo, hi in ((2 * 16 ** 3, 0, 2 * 16 ** 3), (1025, 0, 1025), (4099, 1, 4098), (70001, 4, 70001), (1, 0, 1)):
        inp = CM.kernel_inputs(n, seed=flags + 8 * with_mask)
        src = inp['x'].copy()
        src[::7] = -0.0
        src[3::11] = 0.0
        old = inp['s']
        r = np.random.default_rng(n)
        mask = (r.uniform(size=(n + 1) // 2) > 0.3).astype(np.float32) if with_mask else None
        m_dev = ctx.array(mask) if with_mask else None
        mp = m_dev.ptr if with_mask else None
        mixed = old.copy()
        mixed[lo:hi] = src[lo:hi]
        want, zero_g, got, src_dev = ctx.array(mixed), ctx.zeros((n,)), ctx.array(old), ctx.array(src)
        check(ctx.lib.adm_gd_step(ctx.handle, want.ptr, zero_g.ptr, lo, hi, 0.0, flags, mp))
        check(ctx.lib.adm_cg_accept(ctx.handle, got.ptr, src_dev.ptr, lo, hi, flags, mp))
        assert (bits(got.get()) == bits(want.get())).all(), (n, lo, hi)
        # in place (a failed search: x_src is x)
        same = ctx.array(src)
        check(ctx.lib.adm_cg_accept(ctx.handle, same.ptr, same.ptr, lo, hi, flags, mp))
        assert (bits(same.get())[lo:hi] == bits(want.get())[lo:hi]).all() and (bits(same.get())[:lo] == bits(src)[:lo]).all()
    # an empty range is no launch
    check(ctx.lib.adm_cg_accept(ctx.handle, got.ptr, got.ptr, 5, 5, flags, mp))


# ---- the optimiser, step by step from the fp64 restatement's states --------------------------------------------------------------
@pytest.fixture(scope='module')
def golden():
    return np.load(os.path.join(G, 'F33_cg.npz'))


@pytest.fixture(scope='module')
def prj3d():
    return np.load(os.path.join(G, 'F6_e2e.npz'))['prj']


@pytest.mark.parametrize('name', list(CM.RUNS))
def test_optimiser_step_by_step_against_the_restatement(ctx, golden, prj3d, name, tmp_path):
    import adorym_amd as A
    g = golden
    inp = cases.e2e_inputs()
    states = []
    _, _, recs, _ = R.golden_run(g, name, inp, cases.E2E, CM.RUNS, CM.two_d_inputs, prj3d.astype(np.float64),
                                 on_update=lambda st: states.append({k: (np.array(v, np.float32) if isinstance(v, np.ndarray) and v.dtype == np.float64 else v)
                                                                     for k, v in st.items()}))
    got = []

    class Stepwise(A.CGOptimizer):
        """Every update starts from the restatement's state; the loss at that state is this build's own."""

        def apply_gradient(self, x, gradient, i_batch=None, **kw):
            st = states[len(got)]
            fm = gradient.forward_model
            assert int(fm.loss_args['this_i_theta']) == st['i_theta'] and list(fm.loss_args['this_ind_batch']) == list(st['ind'])
            assert int(i_batch) == st['i_batch']
            x.set(st['x'])
            gradient.arr.set(st['g'])
            self.params_whole_array_dict['descent_dir_old'].set(st['d_old'].reshape(-1))
            self.params_whole_array_dict['s'].set(st['s'].reshape(-1))
            fm.current_loss = fm.get_loss_function()(**fm.loss_args)
            out = super(Stepwise, self).apply_gradient(x, gradient, i_batch, **kw)
            got.append(self.last)
            return out

    params = CM.driver_params(g, name, inp, cases.E2E, prj3d, tmp_path)
    A.reconstruct_ptychography(optimizer=Stepwise('obj', options_dict=CM.options(g, name)), **params)
    assert len(got) == len(recs) == int(g[name + '_n_updates'])
    bar_loss = CM.THREE * float(g[name + '_dist_trial_loss'])
    bar_alpha, bar_beta = CM.THREE * float(g[name + '_dist_alpha']), CM.THREE * float(g[name + '_dist_beta'])
    worst = dict(loss=0., alpha=0., beta=0.)
    for k, (mine, ref) in enumerate(zip(got, recs)):
        # decisions
        assert mine['step_count'] == ref['step_count'], k
        assert (mine['beta_raw'] < 0) == (ref['beta_raw'] < 0) and mine['descends'] == (ref['descent_check'] < 0), k
        assert (mine['alpha'] == 0) == (ref['alpha'] == 0), k
        # values
        worst['beta'] = max(worst['beta'], abs(mine['beta'] - ref['beta']))
        for (a, f), (ar, fr) in zip(mine['trials'], ref['trials']):
            worst['alpha'] = max(worst['alpha'], abs(a - ar) / ar)
            worst['loss'] = max(worst['loss'], abs(f - fr) / ref['f0'])
    print('%s: beta %.2e (bar %.2e), alpha %.2e (bar %.2e), trial loss / f0 %.2e (bar %.2e)'
          % (name, worst['beta'], bar_beta, worst['alpha'], bar_alpha, worst['loss'], bar_loss))
    assert worst['beta'] <= bar_beta and worst['alpha'] <= bar_alpha and worst['loss'] <= bar_loss
