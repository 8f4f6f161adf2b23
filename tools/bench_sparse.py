"""Time sparse multislice (slices at arbitrary depths, adm_plan_set_slice_positions) against the equidistant streamed path it is
built on: rotate -> multislice (forward, loss, adjoint) -> overlap-add with device events after warm-up, the method of
tools/bench_large_probe.py.  Per shape three variants, each timed `--repeats` times in turn (a, b, c, a, b, c, ...):

    a  the streamed path with one H for every gap                       (what existed)
    b  sparse, no slice-position gradient: the same launches as a with a table pointer per gap
    c  sparse with dL/dz: the column launches keep / read one spectrum per gap, one reduction launch more

One JSON line per shape: the median and the spread (max - min) of the repeats in ms per minibatch, the ratios b/a and c/b of the
medians, and the ratio c/b of the bytes counted by bench_large_probe.counted_bytes plus one field written and one read per gap
and mode.  Kernel times: run it under `rocprofv3 --kernel-trace --stats -- python tools/bench_sparse.py ...`.

    python tools/bench_sparse.py [--iters 20] [--warmup 3] [--repeats 3] [--only NAME ...]
"""
import argparse
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import numpy as np

from bench_large_probe import counted_bytes

# name -> (probe side, positions per minibatch, slices)
SHAPES = {'P128_B32_S2': (128, 32, 2), 'P128_B32_S8': (128, 32, 8), 'P256_B32_S2': (256, 32, 2), 'P256_B32_S8': (256, 32, 8)}
ENERGY_EV, PSIZE_CM = 8000., 1e-6


def make(ctx, A, P, B, S, variant):
    r = np.random.default_rng(0)
    Y = X = P + 40
    pos = r.integers(-4, 40, (B, 2))
    z = np.concatenate([[0.], np.cumsum(r.uniform(3e-4, 3e-3, S - 1))])
    kw = dict(streamed=True) if variant == 'a' else dict(slice_pos_cm=z)
    eng = A.MultisliceEngine(ctx, (Y, X, S), (P, P), pos, ENERGY_EV, PSIZE_CM, max_batch=B, **kw)
    obj = ctx.array(np.stack([1e-3 * r.uniform(size=(Y, X, S)), 1e-4 * r.uniform(size=(Y, X, S))], -1).astype(np.float32))
    table = A.RotationTable(ctx, (Y, X, S), 0.3)
    probe = ctx.array(np.stack([r.uniform(0.5, 1.5, (1, P, P)), r.uniform(-0.5, 0.5, (1, P, P))], -1).astype(np.float32))
    gp, gz = ctx.zeros((1, P, P, 2)), ctx.zeros((S,))
    eng.set_batch(pos, r.uniform(0, 30, (B, P, P)).astype(np.float32))

    def step():
        eng.rotate(obj, table)
        eng.multislice(probe, grad_probe=gp, grad_slice_pos=gz if variant == 'c' else None)
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
    base = counted_bytes(P, B, S, 1)
    out = dict(shape=name, P=P, B=B, S=S, iters=iters, repeats=repeats)
    for v in 'abc':
        out['ms_' + v] = round(med[v], 4)
        out['spread_' + v] = round(max(ms[v]) - min(ms[v]), 4)
        out['loss_' + v] = runs[v][0].loss()
    out.update(ratio_b_over_a=round(med['b'] / med['a'], 4), ratio_c_over_b=round(med['c'] / med['b'], 4),
               counted_GB_b=round(base / 1e9, 4), counted_ratio_c_over_b=round((base + 2 * (S - 1) * B * 8 * P * P) / base, 4))
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
