"""tests/cg_ref.py (the NumPy restatement of the conjugate-gradient optimiser and its line search, on the oracle's loss) against
the reference driver's own fp64 runs (golden F33, tests/golden/gen_f33_cg.py): identical decisions at every update, betas, alphas
and losses to 1e-9 relative, the final object to 1e-9 of its largest value.  Also the conditions the generator asserted on the
fixture, re-read from the file, and the two line-search classes of adorym_amd/linesearch.py on scalar functions."""
import os

import numpy as np
import pytest

import cases
from tests import cg_matrix as CM
from tests import cg_ref as R

G = os.path.join(os.path.dirname(__file__), 'golden')


@pytest.fixture(scope='module')
def golden():
    return np.load(os.path.join(G, 'F33_cg.npz'))


def close(a, b, rel=CM.REF_REL):
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    return bool(np.all(np.abs(a - b) <= rel * np.maximum(np.abs(b), 1e-300)))


@pytest.mark.parametrize('name', list(CM.RUNS))
def test_restatement_matches_the_reference_fp64_run(golden, name):
    g = golden
    prj3d = np.load(os.path.join(G, 'F6_e2e.npz'))['prj'].astype(np.float64)
    x, losses, recs, first_grad = R.golden_run(g, name, cases.e2e_inputs(), cases.E2E, CM.RUNS, CM.two_d_inputs, prj3d)
    # decisions
    assert len(recs) == int(g[name + '_n_updates'])
    assert [r['step_count'] for r in recs] == list(g[name + '_n_trials'])
    assert [r['i_batch'] for r in recs] == list(g[name + '_i_batch'])
    assert [r['beta_raw'] < 0 for r in recs] == list(g[name + '_beta_raw'] < 0)
    assert [r['descent_check'] >= 0 for r in recs] == list(g[name + '_descent_check'] >= 0)
    assert [r['alpha'] == 0 for r in recs] == list(g[name + '_alpha'] == 0)
    # values
    for k in ('beta_raw', 'beta', 'f0', 'df0', 'norm', 'alpha'):
        got = [r[k] for r in recs]
        print(name, k, 'max rel distance %.2e' % np.max(np.abs(np.array(got) - g[name + '_' + k]) / np.maximum(np.abs(g[name + '_' + k]), 1e-300)))
        assert close(got, g[name + '_' + k]), k
    assert close([a for r in recs for a, _ in r['trials']], g[name + '_trial_alpha'])
    assert close([f for r in recs for _, f in r['trials']], g[name + '_trial_loss'])
    assert close(losses, g[name + '_losses'])
    ref = g[name + '_obj']
    d = np.abs(CM.sampled(x) - ref).max()
    print(name, 'object: max distance %.2e of max %.2e' % (d, np.abs(ref).max()))
    assert d <= CM.REF_REL * np.abs(ref).max()
    fg = g[name + '_first_grad']
    assert np.abs(CM.sampled(first_grad) - fg).max() <= CM.REF_REL * np.abs(fg).max()


def test_the_fixture_covers_what_it_is_for(golden):
    g = golden
    for name in CM.RUNS:                    # the generator's conditions, as stored
        assert min(g[name + '_min_margin'], g[name + '_min_last']) >= CM.MARGIN_FACTOR * g[name + '_dist_trial_loss'], name
    assert (g['a_n_trials'] == 1).all() and (g['a_beta'][g['a_i_batch'] > 0] > 0).all() and (g['a_i_batch'] > 0).sum() >= 6
    assert (g['b_n_trials'] >= 4).any() and 1e-2 <= g['b_learning_rate'] <= 1
    assert (g['c_alpha'] == 0).any() and (g['c_n_trials'] == 2).all()           # max_backtracking_iter = 1: two trials
    assert (g['d_beta'] == 0).all() and (g['d_i_batch'] == 0).all() and len(g['d_i_batch']) == 8
    assert (np.diff(g['d_losses']) <= 0).all()
    assert g['e_n_clipped'] > 0
    assert os.path.getsize(os.path.join(G, 'F33_cg.npz')) < 2 ** 20


# ---- adorym_amd/linesearch.py on scalar functions (host code: no GPU) -----------------------------------------------------------
def _classes():
    from adorym_amd.linesearch import BackTrackingLineSearch, AdaptiveLineSearch
    return BackTrackingLineSearch, AdaptiveLineSearch


def _quadratic(x):          # f(x) = x^2 / 2 around x0 = 1: g = 1, s = -1, df0 = -1, |s| = 1
    return 0.5 * x * x


def _search(ls, f, x0=1.0):
    calls = []

    def trial(alpha):
        calls.append(alpha)
        return f(x0 - alpha), x0 - alpha
    out = ls.search_values(trial, f(x0), -1.0, 1.0, x0=x0)
    return out, calls


@pytest.mark.parametrize('k', [0, 1])
def test_defaults_and_the_maxiter_cap(k):
    cls = _classes()[k]
    ls = cls()
    assert (ls.contraction_factor, ls.suff_decr, ls.initial_stepsize, ls.stepsize_threshold_low, ls.normalize_alpha) == (0.5, 1e-4, 10.0, 1e-10, True)
    assert ls.optimism == (3., 2.)[k] and ls.maxiter == 23 == R.MACHINE_MAXITER
    assert cls(maxiter=3).maxiter == 3 and cls(maxiter=1000).maxiter == 23


@pytest.mark.parametrize('k', [0, 1])
def test_step_counts_on_a_quadratic(k):
    cls = _classes()[k]
    # Armijo on f = x^2/2 from x0 = 1 along s = -1: alpha^2/2 - alpha <= -1e-4 alpha  <=>  alpha <= 2 - 2e-4
    for step, want_count, want_alpha in ((1.0, 1, 1.0), (2.0, 2, 1.0), (8.0, 4, 1.0), (3.0, 2, 1.5)):
        out, calls = _search(cls(initial_stepsize=step), _quadratic)
        assert (out.step_count, out.alpha, len(calls)) == (want_count, want_alpha, want_count), (step, out)
        assert calls == [step * 0.5 ** j for j in range(want_count)]
        assert out.newf == _quadratic(1.0 - want_alpha) and out.newx == 1.0 - want_alpha
    # normalize_alpha: the first alpha is step / |s|
    ls = cls(initial_stepsize=1.0)
    calls = []
    ls.search_values(lambda a: (calls.append(a) or 0.0, None), 1.0, -4.0, 4.0)
    assert calls == [0.25]
    ls = cls(initial_stepsize=1.0, normalize_alpha=False)
    calls = []
    ls.search_values(lambda a: (calls.append(a) or 0.0, None), 1.0, -4.0, 4.0)
    assert calls == [1.0]


@pytest.mark.parametrize('k', [0, 1])
def test_a_function_that_never_decreases_falls_back_to_x0(k):
    cls = _classes()[k]
    rising = lambda x: 2.0 + abs(x - 1.0)
    out, calls = _search(cls(initial_stepsize=1.0), rising)
    # maxiter = ceil(log 2^-23 / log 0.5) = 23: the loop runs while step_count <= 23, so 24 trials; alpha = 2^-23 is still above 1e-10
    assert len(calls) == 24 == out.step_count and calls[-1] == 2.0 ** -23
    assert (out.newf, out.newx, out.alpha) == (rising(1.0), 1.0, 0.)
    out, calls = _search(cls(initial_stepsize=1.0, maxiter=1), rising)
    assert len(calls) == 2 == out.step_count and out.alpha == 0. and out.newx == 1.0
    # the step threshold ends a search before maxiter does
    out, calls = _search(cls(initial_stepsize=4e-10), rising)
    assert calls == [4e-10, 2e-10, 1e-10] and out.alpha == 0.


def test_the_adaptive_search_carries_its_suggestion_over():
    _, Adaptive = _classes()
    ls = Adaptive(initial_stepsize=8.0)
    out, calls = _search(ls, _quadratic)                # 8, 4, 2, 1: three halvings -> suggestion = optimism * 1
    assert calls == [8.0, 4.0, 2.0, 1.0] and ls._alpha_suggested == 2.0 and ls._alpha == 1.0
    out, calls = _search(ls, _quadratic)                # starts from the suggestion, one halving -> keeps the pace
    assert calls == [2.0, 1.0] and ls._alpha_suggested == 1.0
    out, calls = _search(ls, _quadratic)                # accepted at once -> pushes on
    assert calls == [1.0] and ls._alpha_suggested == 2.0
    # a new object starts from initial_stepsize / |s| again (CGOptimizer builds one per update)
    assert _search(Adaptive(initial_stepsize=8.0), _quadratic)[1][0] == 8.0


def test_the_backtracking_search_carries_its_last_f0_over():
    Back, _ = _classes()
    ls = Back(initial_stepsize=1.0)
    assert ls._oldf0 == -np.inf
    out, calls = _search(ls, _quadratic, x0=1.0)        # f0 = 0.5
    assert calls == [1.0] and ls._oldf0 == 0.5
    # second search at the same f0: oldf0 >= f0 -> alpha = 2 (f0 - oldf0) / df0 * optimism = 0 -> below eps -> initial step again
    out, calls = _search(ls, _quadratic, x0=1.0)
    assert calls[0] == 1.0
    # at a LOWER f0 (0.125 after 0.5): alpha = 2 (0.125 - 0.5) / (-1) * 3 = 2.25
    calls = []
    ls.search_values(lambda a: (calls.append(a) or 0.0, None), 0.125, -1.0, 1.0)
    assert calls[0] == 2.25 and ls._oldf0 == 0.125
    # at a HIGHER f0 the extrapolation is not used
    calls = []
    ls.search_values(lambda a: (calls.append(a) or 0.0, None), 1.0, -1.0, 1.0)
    assert calls[0] == 1.0


def test_the_reference_call_signature_on_host_arrays():
    for cls in _classes():
        x0 = np.array([1.0, -2.0])
        f = lambda x: float(0.5 * np.sum(x * x))
        out = cls(initial_stepsize=1.0, normalize_alpha=False).search(lambda x, step: (f(x + step), x + step), x0, -x0, x0, f0=f(x0))
        assert out.step_count == 1 and out.alpha == 1.0 and np.array_equal(out.newx, np.zeros(2)) and out.newf == 0.0
