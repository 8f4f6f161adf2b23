"""Time sub-pixel probe positions on the streamed path (adm_plan_set_probe_shift) against the plain streamed launch of the same
build: rotate -> multislice (forward, loss, adjoint) -> overlap-add with device events after warm-up, the method of
tools/bench_prj_offset.py.  Far field; per shape three variants, each timed `--repeats` times in turn (a, b, c, a, b, c, ...):

    a  the streamed path without the switch, integer positions            (what existed: the yardstick)
    b  with shifts, probe gradient, no shift gradient
    c  with shifts, probe gradient and dL/d shift

By launch count b is a plus two launches over the M probe modes (FFT2 of the probe), one column launch over the batch in the
forward sweep, one column launch and one row launch over the batch in the adjoint, and one more row transform inside the first
forward and the last adjoint row launch; c adds the fp64 sums inside the adjoint column launch and one reduction launch.  Beside
the 4 launches of a far-field S = 1 minibatch that is much, beside 4 * 16 it is little: both are measured.

One JSON line per shape: the median and the spread (max - min) of the repeats in ms per minibatch and the ratios b/a and c/a of
the medians.  Kernel times: run it under `rocprofv3 --kernel-trace --stats -- python tools/bench_probe_shift.py ...`.

    python tools/bench_probe_shift.py [--iters 20] [--warmup 3] [--repeats 3] [--only NAME ...]
"""
import argparse
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np

# name -> (probe side, positions per minibatch, slices)
SHAPES = {'P256_B32_S1': (256, 32, 1), 'P256_B32_S16': (256, 32, 16), 'P512_B16_S1': (512, 16, 1)}
ENERGY_EV, PSIZE_CM = 8000., 1e-6


def make(ctx, A, P, B, S, variant):
    r = np.random.default_rng(0)
    Y = X = P + 40
    pos = r.integers(-4, 40, (B, 2))
    eng = A.MultisliceEngine(ctx, (Y, X, S), (P, P), pos, ENERGY_EV, PSIZE_CM, free_prop_cm='inf', max_batch=B, streamed=True,
                             probe_shift=variant != 'a')
    obj = ctx.array(np.stack([1e-3 * r.uniform(size=(Y, X, S)), 1e-4 * r.uniform(size=(Y, X, S))], -1).astype(np.float32))
    table = A.RotationTable(ctx, (Y, X, S), 0.3)
    probe = ctx.array(np.stack([r.uniform(0.5, 1.5, (1, P, P)), r.uniform(-0.5, 0.5, (1, P, P))], -1).astype(np.float32))
    gp, gs = ctx.zeros((1, P, P, 2)), ctx.zeros((B, 2))
    shifts = ctx.array(r.uniform(-0.5, 0.5, (B, 2)).astype(np.float32))          # one entry per position, no index
    eng.set_batch(pos, r.uniform(0, 30, (B, P, P)).astype(np.float32))

    def step():
        eng.rotate(obj, table)
        if variant == 'a':
            eng.multislice(probe, grad_probe=gp)
        else:
            eng.multislice(probe, grad_probe=gp, shifts=shifts, grad_shifts=gs if variant == 'c' else None)
    return eng, step


def timed(ctx, step, iters):
    e0, e1 = ctx.event(), ctx.event()
    e0.record()
    for _ in range(iters):
        step()
    e1.record()
    return e0.elapsed_ms(e1) / iters


def run(ctx, A, name, iters, warmup, repeats):
    P, B, S = SHAPES[name]
    runs = {v: make(ctx, A, P, B, S, v) for v in 'abc'}
    for v in 'abc':
        for _ in range(warmup):
            runs[v][1]()
    ms = {v: [] for v in 'abc'}
    for _ in range(repeats):
        for v in 'abc':
            ms[v].append(timed(ctx, runs[v][1], iters))
    med = {v: float(np.median(ms[v])) for v in 'abc'}
    out = dict(shape=name, P=P, B=B, S=S, iters=iters, repeats=repeats)
    for v in 'abc':
        out['ms_' + v] = round(med[v], 4)
        out['spread_' + v] = round(max(ms[v]) - min(ms[v]), 4)
        out['loss_' + v] = runs[v][0].loss()
    out.update(ratio_b_over_a=round(med['b'] / med['a'], 4), ratio_c_over_a=round(med['c'] / med['a'], 4),
               launches_a=4 * S + 1, launches_b=4 * S + 1 + 5, launches_c=4 * S + 1 + 6)        # (with probe_grad_reduce)
    for v in 'abc':
        runs[v][0].plan.close()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--iters', type=int, default=20)
    ap.add_argument('--warmup', type=int, default=3)
    ap.add_argument('--repeats', type=int, default=3)
    ap.add_argument('--only', nargs='*', default=None)
    a = ap.parse_args()
    import adorym_amd as A
    ctx = A.Context(0)
    for name in (a.only or list(SHAPES)):
        print(json.dumps(run(ctx, A, name, a.iters, a.warmup, a.repeats)), flush=True)
    ctx.close()


if __name__ == '__main__':
    main()
