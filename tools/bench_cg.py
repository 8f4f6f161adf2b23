#!/usr/bin/env python3
"""
The conjugate-gradient object optimiser's launches (adm_cg.hip) beside adm_adam_step on the same arrays, at 256^3 x 2 and at
512^2 x 2 elements, then whole CG updates through the driver at config 3's shape (256^3 object, 72 x 72 probe, minibatch 32).  Not
the headline metric (bench.py is); prints one JSON object per line.

    python tools/bench_cg.py [--reps 50] [--rounds 7] [--updates 12]        # on a GPU box

Kernel part.  Device events around `reps` launches queued back to back, ms per launch = elapsed / reps; `rounds` such windows per
variant, the variants alternating, after a warm-up window of each; the median over the rounds with the smallest and the largest.
Each variant also as bytes per second on the bytes it MUST move (4-byte elements: sums + direction 2 reads + 2 reads and 2 writes
= 24 n; trial 2 reads and 1 write = 12 n; accept 1 read and 1 write = 8 n; Adam 4 reads and 3 writes = 28 n) and as a fraction of
6.3 TB/s.  At 512^2 x 2 every array (2 MB) stays in the caches and the launches are a few microseconds: that row measures launch
cost, not memory.

Update part.  The driver with CGOptimizer on synthetic data of two angles of config 3's scan; per update the host time from the
call of apply_gradient to a device synchronise behind it, and the number of trials.  An update is one loss-only forward per trial
plus the launches above: the line says how much of it they are.
"""
import argparse
import json
import os
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import adorym_amd as A                      # noqa: E402
from adorym_amd import _lib                 # noqa: E402
from adorym_amd.device import MappedArray   # noqa: E402
from adorym_amd import workloads as W       # noqa: E402

PEAK = 6.3e12
SHAPES = {'256^3x2': 2 * 256 ** 3, '512^2x2': 2 * 512 ** 2}
BYTES = dict(sums_direction=24, trial=12, accept=8, adam=28)


def window(ev, fn, reps):
    ev[0].record()
    for _ in range(reps):
        fn()
    ev[1].record()
    ev[1].synchronize()
    return ev[0].elapsed_ms(ev[1]) / reps


def kernels(ctx, n, reps, rounds):
    r = np.random.default_rng(0)
    mk = lambda: ctx.array((1e-3 * r.standard_normal(n)).astype(np.float32))
    x, g, s, d_old, xt, m, v = mk(), mk(), mk(), mk(), ctx.empty((n,)), ctx.zeros((n,)), ctx.zeros((n,))
    scratch, sums = ctx.empty((_lib.CG_SCRATCH_DOUBLES,), np.float64), MappedArray(ctx, (8,), np.float64)
    lib, h, chk = ctx.lib, ctx.handle, _lib.check

    def sums_direction():
        chk(lib.adm_cg_beta(h, g.ptr, d_old.ptr, n, 1, scratch.ptr, sums.ptr))
        chk(lib.adm_cg_direction(h, g.ptr, s.ptr, d_old.ptr, n, scratch.ptr, sums.ptr))
    runs = dict(sums_direction=sums_direction,
                trial=lambda: chk(lib.adm_cg_trial(h, x.ptr, s.ptr, 1e-3, xt.ptr, n)),
                accept=lambda: chk(lib.adm_cg_accept(h, x.ptr, xt.ptr, 0, n, _lib.FLAG_NONNEG, None)),
                adam=lambda: chk(lib.adm_adam_step(h, x.ptr, g.ptr, m.ptr, v.ptr, 0, n, 3, 1e-7, 0.9, 0.999, 1e-7, _lib.FLAG_NONNEG, None)))
    ev = [ctx.event() for _ in range(2)]
    t = {k: [] for k in runs}
    for fn in runs.values():
        window(ev, fn, max(reps // 4, 5))
    for _ in range(rounds):
        for k, fn in runs.items():
            t[k].append(window(ev, fn, reps))
    out = {}
    for k, tv in t.items():
        ms = float(np.median(tv))
        rate = BYTES[k] * n / (ms * 1e-3)
        out[k] = dict(ms=round(ms, 5), range=[round(min(tv), 5), round(max(tv), 5)], tb_per_s=round(rate / 1e12, 3),
                      of_peak=round(rate / PEAK, 3))
    for k in ('sums_direction', 'trial', 'accept'):
        out[k]['vs_adam_rate'] = round(out[k]['tb_per_s'] / out['adam']['tb_per_s'], 3)
    return out


def synthetic_data(ctx, cfg, obj, probe, n_theta):
    """|exit wave| in the far field of ``obj`` at the first n_theta angles of the scan: [n_theta, n_pos, Py, Px]."""
    pos, mb = cfg['probe_pos'], cfg['minibatch_size']
    eng = A.MultisliceEngine(ctx, cfg['obj_size'], cfg['probe_size'], pos, cfg['energy_ev'], cfg['psize_cm'], free_prop_cm=cfg['free_prop_cm'],
                             max_batch=mb)
    theta = np.linspace(cfg['theta_st'], cfg['theta_end'], cfg['n_theta'], dtype='float32')[:n_theta]
    obj_dev, probe_dev = ctx.array(obj), ctx.array(probe[None])
    out = np.zeros((n_theta, len(pos)) + tuple(cfg['probe_size']), np.float32)
    for it in range(n_theta):
        table = A.RotationTable(ctx, cfg['obj_size'], theta[it])
        for b in range(0, len(pos), mb):
            p = pos[b:b + mb]
            eng.set_batch(p, np.zeros((len(p),) + tuple(cfg['probe_size']), np.float32))
            eng.rotate(obj_dev, table, eng.y_footprint(p))
            eng.multislice(probe_dev, want_grad=False, want_pred=True)
            out[it, b:b + mb] = eng.pred()
    return out, theta


class _Enough(Exception):
    pass


def updates(ctx_index, n_updates, step_size):
    cfg = W.c3_config()
    ctx = A.Context(ctx_index)
    n_theta = 2
    probe = W.probe_array(cfg)
    data, theta = synthetic_data(ctx, cfg, W.foam_object(cfg['obj_size']).astype(np.float32), probe, n_theta)
    ctx.close()
    times, trials = [], []

    class Timed(A.CGOptimizer):
        def apply_gradient(self, x, gradient, i_batch=None, **kw):
            if len(times) >= n_updates:
                raise _Enough()
            x.ctx.sync()
            t0 = time.perf_counter()
            out = super(Timed, self).apply_gradient(x, gradient, i_batch, **kw)
            x.ctx.sync()
            times.append((time.perf_counter() - t0) * 1e3)
            trials.append(self.last['step_count'])
            return out

    guess = W.random_guess(cfg['obj_size'])
    with tempfile.TemporaryDirectory() as td:
        try:
            A.reconstruct_ptychography(
                fname=data, obj_size=list(cfg['obj_size']), probe_pos=cfg['probe_pos'].astype(float), theta_st=0, theta_end=float(theta[-1]),
                n_theta=n_theta, energy_ev=cfg['energy_ev'], psize_cm=cfg['psize_cm'], free_prop_cm=cfg['free_prop_cm'],
                minibatch_size=cfg['minibatch_size'], n_epochs=1, initial_guess=[guess[..., 0], guess[..., 1]], probe_type='supplied',
                probe_initial=[np.hypot(probe[..., 0], probe[..., 1]), np.arctan2(probe[..., 1], probe[..., 0])], gamma=0, alpha_d=0, alpha_b=0,
                optimizer=Timed('obj', options_dict={'step_size': step_size}), save_path=td, output_folder='out', store_checkpoint=False,
                use_checkpoint=False, gpu_index=ctx_index)
        except _Enough:
            pass
    return times, trials


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--reps', type=int, default=50)
    ap.add_argument('--rounds', type=int, default=7)
    ap.add_argument('--updates', type=int, default=12)
    ap.add_argument('--step-size', type=float, default=1e-4)
    a = ap.parse_args()
    ctx = A.Context(0)
    per_shape = {}
    for name, n in SHAPES.items():
        per_shape[name] = kernels(ctx, n, a.reps if n > (1 << 22) else 20 * a.reps, a.rounds)
        print(json.dumps(dict(part='kernels', shape=name, n=n, reps=a.reps, rounds=a.rounds, **per_shape[name])), flush=True)
    ctx.close()
    times, trials = updates(0, a.updates + 2, a.step_size)
    times, trials = times[2:], trials[2:]                   # (the first updates build tables and load code objects)
    k = per_shape['256^3x2']
    launches = [k['sums_direction']['ms'] + n_t * k['trial']['ms'] + k['accept']['ms'] for n_t in trials]
    per_trial = [(t - l) / n_t for t, l, n_t in zip(times, launches, trials)]
    print(json.dumps(dict(part='update', shape='config 3: 256^3 x 2, 72 x 72 probe, minibatch 32', updates=len(times), trials=trials,
                          update_ms=[round(t, 3) for t in times], update_ms_median=round(float(np.median(times)), 3),
                          cg_launches_ms_median=round(float(np.median(launches)), 3),
                          loss_forward_ms_per_trial_median=round(float(np.median(per_trial)), 3),
                          note='an update is one loss-only forward per trial plus the CG launches; the forwards dominate')), flush=True)


if __name__ == '__main__':
    main()
