#!/usr/bin/env python3
"""
The cost of refining the distances of the detector fan-out (adm_plan_set_fanout_distances; md_fanout_kernel<true> / md_fanin_kernel<true>
of adm_ms_multidist.hip, st_fresnel_table_kernel and st_dd_reduce_kernel of adm_ms_streamed.hip).  Not the headline
metric (bench.py is); prints one JSON object.

    python tools/bench_multidist3d_dist.py [--reps 15] [--inner 10]          # on a GPU box

Field 256 x 256 (the whole field of view is the one position), S = 16 slices, D = 4 distances: the shape of
tools/bench_multidist3d.py.  Three legs, each the multislice launch alone (forward, loss, adjoint; no rotation, no overlap-add):
  (a) host_table       MultisliceEngine(detector_fanout=True): the kernels built on the host once -- the path that existed before
                       and the yardstick of this run;
  (b) device_table     refine_distances=True, multislice(grad_dists=None): the table comes from the device array, the launches are
                       (a)'s, kernel for kernel;
  (c) distance_grad    the same with grad_dists: the twins of the two fan-out kernels (one more store of B M fields, D re-reads of
                       them, D workgroup sums) and one reduce launch.
Timed with events on the plan's stream around ``inner`` back-to-back launches; the legs alternate within every repetition and the
medians over ``reps`` repetitions are reported with their spread (min, max).  Throughput does not depend on the numbers in the
arrays: they are drawn from a seed.
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


def bench(ctx, S, D, reps, inner, warmup=3):
    Py, Px = FIELD
    r = np.random.default_rng([S, D])
    pos = np.zeros((1, 2), int)
    obj = np.stack([2e-3 / S * r.uniform(size=(Py, Px, S)), 2e-4 / S * r.uniform(size=(Py, Px, S))], -1).astype(np.float32)
    probe = ctx.array(np.stack([np.ones((1, Py, Px)), np.zeros((1, Py, Px))], -1).astype(np.float32))
    data = (1 + 0.05 * np.abs(r.standard_normal((D, Py, Px)))).astype(np.float32)
    dists = [float(np.float32(d)) for d in DISTS_CM[:D]]        # (float32-representable: both engines at the same distances)
    kw = dict(max_batch=1, streamed=True, detector_fanout=True)
    host = A.MultisliceEngine(ctx, (Py, Px, S), FIELD, pos, ENERGY_EV, PSIZE_CM, free_prop_cm=dists, **kw)
    dev = A.MultisliceEngine(ctx, (Py, Px, S), FIELD, pos, ENERGY_EV, PSIZE_CM, free_prop_cm=dists, refine_distances=True, **kw)
    d_obj = ctx.array(obj)
    for e in (host, dev):
        e.set_batch(pos, data)
        e.rotate(d_obj, None)
    gd = ctx.zeros((D,))
    ev = [ctx.event() for _ in range(2)]
    legs = {'host_table': lambda: host.multislice(probe, accumulate=False),
            'device_table': lambda: dev.multislice(probe, accumulate=False),
            'distance_grad': lambda: dev.multislice(probe, accumulate=False, grad_dists=gd)}

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
    # same model: the loss sums of the three legs
    sums = {}
    for k, fn in legs.items():
        fn()
        sums[k] = (host if k == 'host_table' else dev).loss_sums(D)
    for e in (host, dev):
        e.plan.close()
    spread = lambda v: dict(median_ms=float(np.median(v)), min_ms=float(np.min(v)), max_ms=float(np.max(v)))
    med = {k: float(np.median(v)) for k, v in t.items()}
    out = dict(row='multidist3d_dist', field=list(FIELD), n_slices=S, n_dists=D, reps=reps, launches_per_window=inner)
    out.update({k: spread(v) for k, v in t.items()})
    out.update(device_table_over_host_table=med['device_table'] / med['host_table'],
               distance_grad_over_host_table=med['distance_grad'] / med['host_table'],
               loss_sums_device_vs_host_rel_diff=float(np.abs(sums['device_table'] / sums['host_table'] - 1).max()),
               loss_sums_grad_vs_device_equal=bool(np.array_equal(sums['distance_grad'], sums['device_table'])))
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
