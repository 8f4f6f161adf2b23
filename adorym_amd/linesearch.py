"""
Backtracking line searches with the reference's constructor arguments, defaults and arithmetic (adorym/linesearch.py:15-200).

Both classes are host code: they are steered by loss VALUES, which the host holds anyway, and never touch an array.  What they
search along is described by three numbers the caller has already -- ``f0``, the directional derivative ``df0 = <s, g>`` and the
norm ``|s|`` -- and by one callable ``trial(alpha) -> (loss, point)`` that evaluates the objective at ``x0 + alpha * s``
(CGOptimizer: one adm_cg_trial launch and one loss-only forward).  ``search_values`` is that form; ``search`` keeps the reference's
signature for host arrays (NumPy) and reduces to it.

    alpha_0 = initial_stepsize / |s|  (normalize_alpha)  or  initial_stepsize, unless the object carries a better start over
              from its last search (the adaptive class: its suggested alpha; the backtracking class: 2 (f0 - f0_last) / df0 * optimism
              when f0 did not rise)
    while  f(alpha) > f0 + suff_decr * alpha * df0  and  step_count <= maxiter  and  alpha > stepsize_threshold_low:
        alpha *= contraction_factor
    result (newf, newx, alpha, step_count); (f0, x0, 0., step_count) when the last trial is not at or below f0

``maxiter`` is capped at ceil(log eps / log contraction_factor) with the float32 epsilon: 23 halvings for 0.5.
"""
from collections import namedtuple

import numpy as np

__all__ = ['BackTrackingLineSearch', 'AdaptiveLineSearch', 'LSState']

LSState = namedtuple('LSState', ['newf', 'newx', 'alpha', 'step_count'])


class _LineSearch(object):
    """What the two searches share: the options, the Armijo loop and the fallback."""
    _default_optimism = 2.

    def __init__(self, contraction_factor=0.5, optimism=None, suff_decr=1e-4, initial_stepsize=10.0, stepsize_threshold_low=1e-10,
                 dtype=np.float32, maxiter=None, name='backtracking_linesearch', normalize_alpha=True):
        self.contraction_factor = contraction_factor
        self.optimism = self._default_optimism if optimism is None else optimism
        self.suff_decr = suff_decr
        self.initial_stepsize = initial_stepsize
        self.stepsize_threshold_low = stepsize_threshold_low
        self.normalize_alpha = normalize_alpha
        self._dtype = dtype
        self._machine_eps = float(np.finfo(dtype).eps)
        self._name = name
        machine_maxiter = int(np.ceil(np.log(self._machine_eps) / np.log(self.contraction_factor)))
        self.maxiter = machine_maxiter if maxiter is None else int(min(maxiter, machine_maxiter))
        self._alpha = 0.
        self.trials = []            # (alpha, loss) of every trial of the last search, in order

    def _first_alpha(self, descent_norm):
        return self.initial_stepsize / descent_norm if self.normalize_alpha else self.initial_stepsize

    def _start(self, f0, df0, descent_norm):
        raise NotImplementedError

    def _finish(self, f0, state):
        raise NotImplementedError

    def search_values(self, trial, f0, df0, descent_norm, x0=None):
        """``trial(alpha)`` returns (loss, point).  f0, df0, descent_norm: Python floats."""
        f0, df0, descent_norm = float(f0), float(df0), float(descent_norm)
        alpha = float(self._start(f0, df0, descent_norm))
        self.trials = []
        newf, newx = trial(alpha)
        self.trials.append((alpha, float(newf)))
        state = LSState(newf, newx, alpha, 1)
        while (state.newf > f0 + self.suff_decr * state.alpha * df0 and state.step_count <= self.maxiter
               and state.alpha > self.stepsize_threshold_low):
            alpha = self.contraction_factor * state.alpha
            newf, newx = trial(alpha)
            self.trials.append((alpha, float(newf)))
            state = LSState(newf, newx, alpha, state.step_count + 1)
        self._finish(f0, state)
        self._alpha = state.alpha
        if state.newf <= f0:
            return state
        return LSState(f0, x0, 0., state.step_count)

    def search(self, objective_and_update, x0, descent_dir, gradient, f0=None):
        """The reference's call for host arrays: objective_and_update(x0, step) -> (loss, x0 + step)."""
        x0, s, g = np.asarray(x0), np.asarray(descent_dir), np.asarray(gradient)
        if f0 is None:
            f0, _ = objective_and_update(x0, np.zeros_like(x0))
        descent_norm = float(np.sqrt(np.sum(s.astype(np.float64) ** 2)))
        df0 = float(np.sum(s.astype(np.float64) * g))
        return self.search_values(lambda alpha: objective_and_update(x0, alpha * s), f0, df0, descent_norm, x0=x0)


class BackTrackingLineSearch(_LineSearch):
    """adorym/linesearch.py:15-103: the first alpha is extrapolated from the decrease of f0 since the last search of this object."""
    _default_optimism = 3.

    def __init__(self, *args, **kwargs):
        super(BackTrackingLineSearch, self).__init__(*args, **kwargs)
        self._oldf0 = -np.inf

    def _start(self, f0, df0, descent_norm):
        if self._oldf0 >= f0:
            alpha = 2 * (f0 - self._oldf0) / df0 * self.optimism
            if alpha * descent_norm < self._machine_eps:
                alpha = self._first_alpha(descent_norm)
            return alpha
        return self._first_alpha(descent_norm)

    def _finish(self, f0, state):
        self._oldf0 = f0


class AdaptiveLineSearch(_LineSearch):
    """adorym/linesearch.py:106-200: the first alpha is the one the last search of this object suggested."""
    _default_optimism = 2.

    def __init__(self, *args, **kwargs):
        super(AdaptiveLineSearch, self).__init__(*args, **kwargs)
        self._alpha_suggested = 0

    def _start(self, f0, df0, descent_norm):
        return self._alpha_suggested if self._alpha_suggested > 0 else self._first_alpha(descent_norm)

    def _finish(self, f0, state):
        # accepted at once: push on; after one halving: keep the pace; after more: the step has become small, try to recover
        self._alpha_suggested = state.alpha if state.step_count == 2 else self.optimism * state.alpha
