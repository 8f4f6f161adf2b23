"""Generates tests/golden/F33_cg.npz from the reference implementation (data only).

Usage: python tests/golden/gen_f33_cg.py        (needs the reference checkout that gen_goldens.py imports; CPU only)

The reference driver with optimizer='cg' (CGOptimizer, adorym/optimizers.py:594-704; AdaptiveLineSearch, adorym/linesearch.py),
fp64 and fp32, on cases.e2e_inputs() through gen_goldens.run_driver: the runs of tests/cg_matrix.py (a: first-trial acceptances with
beta > 0; b: backtracking; c: a failed search; d: 2-D, one slice; e: non_negativity).  Recorded per update, by wrapping
CGOptimizer._calculate_PR_beta and the search: the raw and the clamped beta, the descent check, f0, df0, |s|, every trial's
(alpha, loss), the accepted alpha; per run the losses, the final object and the first gradient.  fp64 whole -- the two arrays on the
4096 voxels of cg_matrix.obj_sample, five whole float64 objects being larger than a committed file may be; of fp32 only its distances
from fp64.

Conditions on the fixture, asserted here: fp64 and fp32 take the same decision at every branch (trials per update, beta clamped or
not, the descent check, accepted or failed), and at every evaluated trial the Armijo margin |newf - (f0 + 1e-4 alpha df0)|, and
|newf - f0| at the last trial, is at least cg_matrix.MARGIN_FACTOR x the largest fp32-fp64 distance of any trial loss of that run.
Runs b, c and e take the first candidate step that meets this (e: and leaves voxels clipped at 0).
"""
import contextlib
import io
import os
import sys
import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.join(HERE, '..', '..'))
import gen_goldens as G  # noqa: E402  (the I/O shims and the reference on sys.path)
import cases  # noqa: E402
import torch  # noqa: E402
import adorym.optimizers as RO  # noqa: E402
import adorym.linesearch as LS  # noqa: E402
from oracle import adorym_oracle as O  # noqa: E402
from tests import cg_matrix as CM  # noqa: E402

LOG = []            # one dict per update of the run in progress
_PENDING = {}


def _wrap():
    orig_beta = RO.CGOptimizer._calculate_PR_beta

    def beta_rec(self, ss, i_batch):
        p = self._descent_dir_t
        idx = tuple(ss) if isinstance(ss, list) else ss
        p_old = self.params_whole_array_dict['descent_dir_old'][idx]
        s_old = self.params_whole_array_dict['s'][idx]
        raw = float(torch.sum(p * (p - p_old)) / torch.sum(p_old * p_old)) if i_batch > 0 else 0.
        beta = orig_beta(self, ss, i_batch)
        check = float(torch.sum((p + beta * s_old) * (-p)))
        _PENDING.update(beta_raw=raw, beta=float(beta), descent_check=check, i_batch=int(i_batch))
        return beta

    RO.CGOptimizer._calculate_PR_beta = beta_rec

    def wrap_search(cls):
        orig = cls.search

        def search(self, fn, x0, descent_dir, gradient, f0=None):
            fs = []

            def fn2(x, y):
                f, u = fn(x, y)
                fs.append(float(f))
                return f, u
            out = orig(self, fn2, x0, descent_dir, gradient, f0)
            n, last = len(fs), float(self._alpha)
            LOG.append(dict(_PENDING, f0=float(f0), df0=float(torch.sum(descent_dir * gradient)),
                            norm=float(torch.sqrt(torch.sum(descent_dir ** 2))), alphas=[last * 2. ** (n - 1 - k) for k in range(n)],
                            fs=fs, alpha=float(out.alpha)))
            return out
        cls.search = search
    wrap_search(LS.AdaptiveLineSearch)
    wrap_search(LS.BackTrackingLineSearch)
    RO.CGOptimizer.linesearch_map = {'backtracking': LS.BackTrackingLineSearch, 'adaptive': LS.AdaptiveLineSearch}


def run_pair(name, spec, inp, prj3d, lr):
    """The fp64 and the fp32 run of one fixture -> (arrays to store, usable?)."""
    E = cases.E2E
    N = E['N']
    if spec['three_d']:
        n_theta, osz, guess, prj, theta_end = E['n_theta'], [N, N, N], inp['guess'], prj3d, 2 * np.pi
    else:
        truth, guess = CM.two_d_inputs(inp, N)
        n_theta, osz, theta_end = 1, [N, N, 1], 0
        phys = O.Physics((E['P'], E['P']), E['energy_ev'], E['psize_cm'], free_prop_cm='inf')
        probe = inp['probe_mag'] * np.exp(1j * inp['probe_phase'])
        tiles, _ = O.extract_tiles(truth, inp['probe_pos'], (E['P'], E['P']))
        prj = np.abs(O.multislice_forward(tiles, probe, phys, 'float64'))[None].astype(np.float32).astype(np.float64)
    res = {}
    for fp64 in (True, False):
        LOG.clear()
        rec = {}
        ex = dict(minibatch_size=spec['minibatch_size'], initial_guess=[guess[0], guess[1]], probe_type='supplied',
                  probe_initial=[inp['probe_mag'], inp['probe_phase']], two_d_mode=not spec['three_d'], n_epochs=spec['n_epochs'],
                  optimizer='cg', learning_rate=lr, run_float64=fp64, non_negativity=bool(spec.get('non_negativity')))
        if spec.get('options'):
            ex['optimizer'] = RO.CGOptimizer('obj', output_folder='out', options_dict=dict(spec['options'], step_size=lr))
        with contextlib.redirect_stdout(io.StringIO()):
            G.run_driver(prj, osz, inp['probe_pos'], theta_end, n_theta, ex, rec)
        res[fp64] = ([dict(u) for u in LOG], rec)
    (l64, r64), (l32, r32) = res[True], res[False]
    same = (len(l64) == len(l32) and all(len(a['fs']) == len(b['fs']) and (a['beta_raw'] < 0) == (b['beta_raw'] < 0)
                                         and (a['descent_check'] >= 0) == (b['descent_check'] >= 0)
                                         and (a['alpha'] == 0) == (b['alpha'] == 0) for a, b in zip(l64, l32)))
    if not same:
        print(name, 'lr', lr, ': fp32 and fp64 decide differently')
        return None, False
    d_trial = max(abs(fa - fb) / a['f0'] for a, b in zip(l64, l32) for fa, fb in zip(a['fs'], b['fs']))
    margin = min(abs(f - (u['f0'] + 1e-4 * al * u['df0'])) / u['f0'] for u in l64 for al, f in zip(u['alphas'], u['fs']))
    last = min(abs(u['fs'][-1] - u['f0']) / u['f0'] for u in l64)
    counts = [len(u['fs']) for u in l64]
    print('%s lr %g: trials %s, betas %s, failed %d, margin/f0 %.2e, last/f0 %.2e, fp32 trial distance/f0 %.2e'
          % (name, lr, counts, np.round([u['beta_raw'] for u in l64], 3), sum(u['alpha'] == 0 for u in l64), margin, last, d_trial))
    ok = min(margin, last) >= CM.MARGIN_FACTOR * d_trial
    # (objects and the first gradient: on cg_matrix.obj_sample's voxels, to stay within the size of a committed file)
    shape = tuple(osz) + (2,)
    x64, x32 = (CM.sampled(np.stack([r['delta'], r['beta']], -1).reshape(shape)) for r in (r64, r32))
    x0 = CM.sampled(np.stack([guess[0], guess[1]], -1).reshape(shape))
    rel = lambda a, b: abs(a - b) / max(abs(b), 1e-300)
    out = {
        'learning_rate': lr, 'n_updates': len(l64), 'n_trials': np.array(counts),
        'i_batch': np.array([u['i_batch'] for u in l64]), 'beta_raw': np.array([u['beta_raw'] for u in l64]),
        'beta': np.array([u['beta'] for u in l64]), 'descent_check': np.array([u['descent_check'] for u in l64]),
        'f0': np.array([u['f0'] for u in l64]), 'df0': np.array([u['df0'] for u in l64]), 'norm': np.array([u['norm'] for u in l64]),
        'trial_alpha': np.concatenate([u['alphas'] for u in l64]), 'trial_loss': np.concatenate([u['fs'] for u in l64]),
        'alpha': np.array([u['alpha'] for u in l64]), 'losses': r64['losses'], 'obj': x64,
        'first_grad': CM.sampled(r64['first_grad'].reshape(shape)),
        'batches_theta': np.array([b[0] for b in r64['batches']]), 'batches_ind': np.array([b[1] for b in r64['batches']]),
        # ---- of fp32: its distances from fp64 ----
        'dist_trial_loss': d_trial, 'min_margin': margin, 'min_last': last,
        'dist_beta': max(abs(a['beta'] - b['beta']) for a, b in zip(l64, l32)),
        'dist_alpha': max(rel(aa, ab) for a, b in zip(l64, l32) for aa, ab in zip(b['alphas'], a['alphas'])),
        'dist_f0': max(rel(b['f0'], a['f0']) for a, b in zip(l64, l32)),
        'dist_df0': max(rel(b['df0'], a['df0']) for a, b in zip(l64, l32)),
        'dist_norm': max(rel(b['norm'], a['norm']) for a, b in zip(l64, l32)),
        'dist_losses': float(np.max(np.abs(r32['losses'] - r64['losses']) / np.abs(r64['losses']))),
        'dist_obj': float(np.linalg.norm(x32 - x64)), 'update_norm': float(np.linalg.norm(x64 - x0)),
        'n_clipped': int((x64 == 0).sum()),
    }
    if not spec['three_d']:
        out['prj'] = prj.astype(np.float32)
    return out, ok


def main():
    _wrap()
    inp = cases.e2e_inputs()
    prj3d = np.load(os.path.join(HERE, 'F6_e2e.npz'))['prj'].astype(np.float64)
    store = {}
    for name, spec in CM.RUNS.items():
        cands = (spec['learning_rate'],) if spec['learning_rate'] is not None else {'b': CM.B_CANDIDATES, 'c': CM.C_CANDIDATES, 'e': CM.E_CANDIDATES}[name]
        for lr in cands:
            out, ok = run_pair(name, spec, inp, prj3d, lr)
            if out is not None and name == 'b':
                ok = ok and int((out['n_trials'] >= 4).sum()) >= 1        # an update that backtracks three times or more
            if out is not None and name == 'c':
                ok = ok and bool((out['alpha'] == 0).any())               # a search that fails
            if out is not None and name == 'e':
                ok = ok and out['n_clipped'] > 0                          # the constraint binds
            if ok:
                break
            print(name, 'lr', lr, 'dropped')
        assert ok, name
        if name == 'a':
            assert (out['n_trials'] == 1).all() and (out['beta'][out['i_batch'] > 0] > 0).all()
        for k, v in out.items():
            store['%s_%s' % (name, k)] = v
    G.save('F33_cg', **store)


if __name__ == '__main__':
    main()
