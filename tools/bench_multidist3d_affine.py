#!/usr/bin/env python3
"""
The cost of registering the measured holograms around the detector fan-out launch (adm_register_targets, adm_register_grad:
adm_register.hip).  Not the headline metric (bench.py is); prints one JSON object.

    python tools/bench_multidist3d_affine.py [--reps 15] [--inner 10]          # on a GPU box

Field 256 x 256 (the whole field of view is the one position), S = 16 slices, D = 4 distances: the shape of
tools/bench_multidist3d.py.  Four legs, each ONE evaluation without rotation and overlap-add:
  (0) launch_plain      MultisliceEngine(detector_fanout=True).multislice() with a target that is already on the device, as
                        tools/bench_multidist3d_dist.py times it (its host_table leg): no multislice kernel changed, so the figure
                        is printed beside the parent commit's from DESIGN.md section 5;
  (a) launch            the same with want_pred=True (the predictions stay on the device for the gradient): the yardstick of (b), (c);
  (b) targets           HologramRegistration.targets() in front of the same launch (one kernel, one thread per detector pixel);
  (c) targets_grad      ... and HologramRegistration.grad() behind it (two kernels: the partial sums and their reduction).
Timed with events on the context's stream around ``inner`` back-to-back evaluations; the legs alternate within every repetition
and the medians over ``reps`` repetitions are reported with their spread (min, max).  Throughput does not depend on the numbers in
the arrays: they are drawn from a seed.
"""
import argparse
import json
import os
import subprocess
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import adorym_amd as A                      # noqa: E402

ENERGY_EV, PSIZE_CM = 8000., 1e-6
FIELD = (256, 256)
DISTS_CM = [1e-4, 2e-4, 3.5e-4, 5e-4]
PARENT_LAUNCH_MS = 2.813                    # the same launch on the parent commit (tools/bench_multidist3d_dist.py, host table)


def commit():
    try:
        return subprocess.run(['git', '-C', ROOT, 'rev-parse', '--short', 'HEAD'], capture_output=True, timeout=30).stdout.decode().strip() or None
    except Exception:
        return None


def bench(ctx, S, D, reps, inner, warmup=3):
    Py, Px = FIELD
    r = np.random.default_rng([S, D])
    pos = np.zeros((1, 2), int)
    obj = np.stack([2e-3 / S * r.uniform(size=(Py, Px, S)), 2e-4 / S * r.uniform(size=(Py, Px, S))], -1).astype(np.float32)
    probe = ctx.array(np.stack([np.ones((1, Py, Px)), np.zeros((1, Py, Px))], -1).astype(np.float32))
    data = ctx.array((1 + 0.05 * np.abs(r.standard_normal((D, Py, Px)))).astype(np.float32))
    theta = np.tile(np.array([[1., 0, 0], [0, 1., 0]], np.float32), (D, 1, 1))
    theta[1:] += (0.02 * r.standard_normal((D - 1, 2, 3))).astype(np.float32)
    theta = ctx.array(theta)
    eng = A.MultisliceEngine(ctx, (Py, Px, S), FIELD, pos, ENERGY_EV, PSIZE_CM, free_prop_cm=DISTS_CM[:D], max_batch=1, streamed=True,
                             detector_fanout=True)
    reg = A.HologramRegistration(ctx, D, FIELD, 'magnitude')
    target = reg.targets(data, theta)
    eng.set_batch(pos, target)
    eng.rotate(ctx.array(obj), None)
    g = ctx.zeros((D, 2, 3))
    ev = [ctx.event() for _ in range(2)]

    def launch_plain():
        eng.multislice(probe, accumulate=False)

    def launch():
        eng.multislice(probe, accumulate=False, want_pred=True)

    def with_targets():
        reg.targets(data, theta)
        launch()

    def with_grad():
        with_targets()
        reg.grad(data, theta, eng.pred_device(), g)
    legs = {'launch_plain': launch_plain, 'launch': launch, 'targets': with_targets, 'targets_grad': with_grad}

    def timed(fn):
        ev[0].record()
        for _ in range(inner):
            fn()
        ev[1].record()
        return ev[0].elapsed_ms(ev[1]) / inner          # (blocks until the window has run)

    for _ in range(warmup):
        for fn in legs.values():
            fn()
    ctx.sync()
    t = {k: [] for k in legs}
    for _ in range(reps):
        for k, fn in legs.items():
            t[k].append(timed(fn))
    # same model: the loss sums of the legs
    sums = {}
    for k, fn in legs.items():
        fn()
        sums[k] = eng.loss_sums(D)
    g.zero_()
    with_grad()
    grad_finite = bool(np.all(np.isfinite(g.get())))
    eng.plan.close()
    spread = lambda v: dict(median_ms=float(np.median(v)), min_ms=float(np.min(v)), max_ms=float(np.max(v)))
    med = {k: float(np.median(v)) for k, v in t.items()}
    out = dict(row='multidist3d_affine', commit=commit(), field=list(FIELD), n_slices=S, n_dists=D, reps=reps, launches_per_window=inner)
    out.update({k: spread(v) for k, v in t.items()})
    out.update(parent_launch_ms=PARENT_LAUNCH_MS, launch_plain_over_parent=med['launch_plain'] / PARENT_LAUNCH_MS,
               targets_over_launch=med['targets'] / med['launch'], targets_grad_over_launch=med['targets_grad'] / med['launch'],
               targets_ms=med['targets'] - med['launch'], grad_ms=med['targets_grad'] - med['targets'],
               loss_sums_equal=bool(np.array_equal(sums['launch'], sums['targets']) and np.array_equal(sums['launch'], sums['targets_grad'])
                                    and np.array_equal(sums['launch'], sums['launch_plain'])),
               grad_finite=grad_finite)
    return out


if __name__ == '__main__':
    ap = argparse.ArgumentParser()
    ap.add_argument('--reps', type=int, default=15)
    ap.add_argument('--inner', type=int, default=10)
    ap.add_argument('--slices', type=int, default=16)
    ap.add_argument('--dists', type=int, default=4)
    args = ap.parse_args()
    ctx = A.Context(0)
    print(json.dumps(bench(ctx, args.slices, args.dists, args.reps, args.inner)), flush=True)
    ctx.close()
