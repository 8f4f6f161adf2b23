"""Time the engine loop of the streamed multislice path (adm_ms_streamed.hip) on large probes: rotate -> multislice (forward,
loss, adjoint) -> overlap-add, with device events after warm-up.  One line per shape: ms per minibatch, positions/s, and the
bytes counted by `counted_bytes` below with the effective rate they imply.  Kernel times: run it under
`rocprofv3 --kernel-trace --stats` (tools/kstats.py reads the output).

    python tools/bench_large_probe.py [--iters 20] [--warmup 3] [--only NAME ...]
"""
import argparse
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np

# name -> (probe side, positions per minibatch, slices, probe modes, engine keywords)
SHAPES = {
    'P256_B32_S1_M1': (256, 32, 1, 1, dict(streamed=True)),
    'P256_B32_S1_M5': (256, 32, 1, 5, dict(streamed=True)),
    'P256_B32_S16_M1': (256, 32, 16, 1, dict(streamed=True)),
    'P512_B16_S1_M1': (512, 16, 1, 1, dict(streamed=True)),
    'P128_B32_S16_streamed': (128, 32, 16, 1, dict(streamed=True)),
    'P128_B32_S16_generic': (128, 32, 16, 1, dict(generic=True)),       # the A/B: the one-workgroup any-size kernel
}


def counted_bytes(P, B, S, M):
    """Global-memory traffic of one minibatch of the streamed path, in field-sized transfers (P*P complex fp32 = 8 P^2 bytes):
    forward row launch per step: read + write + stash per mode, the slice once (3M + 1); adjoint row launch per step: read + stash
    + write per mode, the slice, the tile gradient (3M + 2); every convolution (S - 1 each way): read + write + H per mode (3M);
    detector: read + write per mode, the parked fields of several modes twice (2M), target + prediction (one field's worth);
    overlap-add: the S tile-gradient rows.  The rotation and the object-sized arrays are not counted."""
    per_pos = S * (3 * M + 1) + S * (3 * M + 2) + 2 * (S - 1) * 3 * M + 2 * M + (2 * M if M > 1 else 0) + 1 + S
    return per_pos * B * 8 * P * P


def run(ctx, A, name, iters, warmup):
    P, B, S, M, kw = SHAPES[name]
    r = np.random.default_rng(0)
    Y = X = P + 40
    pos = r.integers(-4, 40, (B, 2))
    eng = A.MultisliceEngine(ctx, (Y, X, S), (P, P), pos, 5000., 1e-7, n_probe_modes=M, max_batch=B, **kw)
    obj = ctx.array(np.stack([1e-5 * r.uniform(size=(Y, X, S)), 1e-6 * r.uniform(size=(Y, X, S))], -1).astype(np.float32))
    table = A.RotationTable(ctx, (Y, X, S), 0.3)
    probe = ctx.array(np.stack([r.uniform(0.5, 1.5, (M, P, P)), r.uniform(-0.5, 0.5, (M, P, P))], -1).astype(np.float32))
    gp = ctx.zeros((M, P, P, 2))
    eng.set_batch(pos, r.uniform(0, 30, (B, P, P)).astype(np.float32))

    def step():
        eng.rotate(obj, table)
        eng.multislice(probe, grad_probe=gp)

    for _ in range(warmup):
        step()
    e0, e1 = ctx.event(), ctx.event()
    e0.record()
    for _ in range(iters):
        step()
    e1.record()
    ms = e0.elapsed_ms(e1) / iters
    nbytes = counted_bytes(P, B, S, M) if eng.streamed else None
    out = dict(shape=name, P=P, B=B, S=S, M=M, streamed=eng.streamed, ms_per_minibatch=round(ms, 4), positions_per_s=round(B / (ms * 1e-3), 1),
               counted_GB=round(nbytes / 1e9, 4) if nbytes else None, counted_TBps=round(nbytes / (ms * 1e-3) / 1e12, 3) if nbytes else None,
               loss=eng.loss())
    eng.plan.close()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--iters', type=int, default=20)
    ap.add_argument('--warmup', type=int, default=3)
    ap.add_argument('--only', nargs='*', default=None)
    a = ap.parse_args()
    import adorym_amd as A
    ctx = A.Context(0)
    for name in (a.only or list(SHAPES)):
        print(json.dumps(run(ctx, A, name, a.iters, a.warmup)), flush=True)
    ctx.close()


if __name__ == '__main__':
    main()
