#!/usr/bin/env python3
"""
One exit wave to D detector planes (adm_plan_set_detector_fanout, adm_ms_multidist.hip) against the path that existed before it:
D single-distance streamed launches of the same object, one per distance, each with a slice sweep of its own.  Not the headline
metric (bench.py is); prints one JSON object per case.

    python tools/bench_multidist3d.py [--reps 15] [--inner 10]          # on a GPU box

Field 256 x 256 (the whole field of view is the one position), S = 16 and 64 slices, D = 2 and 4 distances.  Both legs are the
multislice launch alone (forward, loss, adjoint; no rotation, no overlap-add), timed with events on the plan's stream around
``inner`` back-to-back launches; the two legs alternate within every repetition and the medians over ``reps`` repetitions are
reported with their spread (min, max).  Throughput does not depend on the numbers in the arrays: they are drawn from a seed.
"""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import adorym_amd as A                      # noqa: E402

ENERGY_EV, PSIZE_CM = 8000., 1e-6
FIELD = (256, 256)
DISTS_CM = [1e-4, 2e-4, 3.5e-4, 5e-4]
CASES = [(S, D) for S in (16, 64) for D in (2, 4)]


def bench_case(ctx, S, D, reps, inner, warmup=3):
    Py, Px = FIELD
    r = np.random.default_rng([S, D])
    pos = np.zeros((1, 2), int)
    obj = np.stack([2e-3 / S * r.uniform(size=(Py, Px, S)), 2e-4 / S * r.uniform(size=(Py, Px, S))], -1).astype(np.float32)
    probe = ctx.array(np.stack([np.ones((1, Py, Px)), np.zeros((1, Py, Px))], -1).astype(np.float32))
    data = (1 + 0.05 * np.abs(r.standard_normal((D, Py, Px)))).astype(np.float32)
    dists = DISTS_CM[:D]
    kw = dict(max_batch=1, streamed=True)
    fan = A.MultisliceEngine(ctx, (Py, Px, S), FIELD, pos, ENERGY_EV, PSIZE_CM, free_prop_cm=dists, detector_fanout=True, **kw)
    singles = [A.MultisliceEngine(ctx, (Py, Px, S), FIELD, pos, ENERGY_EV, PSIZE_CM, free_prop_cm=d, **kw) for d in dists]
    d_obj = ctx.array(obj)
    fan.set_batch(pos, data)
    fan.rotate(d_obj, None)
    for d, e in enumerate(singles):
        e.set_batch(pos, data[d:d + 1])
        e.rotate(d_obj, None)
    ev = [ctx.event() for _ in range(2)]

    def run_fan():
        fan.multislice(probe, accumulate=False)

    def run_singles():
        for e in singles:
            e.multislice(probe, accumulate=False)

    def timed(fn):
        ev[0].record()
        for _ in range(inner):
            fn()
        ev[1].record()
        return ev[0].elapsed_ms(ev[1]) / inner          # (blocks until the window has run)

    for _ in range(warmup):
        run_fan()
        run_singles()
    ctx.sync()
    t_fan, t_one = [], []
    for _ in range(reps):
        t_fan.append(timed(run_fan))
        t_one.append(timed(run_singles))
    # same model: the fan-out's losses are the single launches', distance by distance
    run_fan()
    l_fan = fan.loss_sums(D)
    run_singles()
    l_one = np.array([e.loss_sums(1)[0] for e in singles])
    for e in [fan] + singles:
        e.plan.close()
    spread = lambda t: dict(median_ms=float(np.median(t)), min_ms=float(np.min(t)), max_ms=float(np.max(t)))
    return dict(row='multidist3d', field=list(FIELD), n_slices=S, n_dists=D, reps=reps, launches_per_window=inner,
                fanout=spread(t_fan), one_launch_per_distance=spread(t_one), ratio=float(np.median(t_one) / np.median(t_fan)),
                loss_sums_rel_diff=float(np.abs(l_fan / l_one - 1).max()))


if __name__ == '__main__':
    ap = argparse.ArgumentParser()
    ap.add_argument('--reps', type=int, default=15)
    ap.add_argument('--inner', type=int, default=10)
    args = ap.parse_args()
    ctx = A.Context(0)
    for S, D in CASES:
        print(json.dumps(bench_case(ctx, S, D, args.reps, args.inner)), flush=True)
    ctx.close()
