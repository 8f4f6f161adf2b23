#!/usr/bin/env python3
"""
Time per call of the direct CTF inversion (adm_ctfinv_run: I1, I2, I3) at 512 x 512 x 4 distances with 1 and with 16 angles per
launch group and at 2048 x 2048 x 4 with 1 angle, beside the CTF forward / adjoint launch group (adm_ctf_fwd_adj, want_grad = 2:
C1 ... C5) at 512 x 512 x 4 in the same process.  Not the headline metric (bench.py is); prints one JSON object per row.

    python tools/bench_ctf_invert.py [--reps 2000] [--rounds 7]        # on a GPU box

Method: device events around `reps` calls queued back to back (a call is three dependent kernels; nothing is read back inside
the window), ms per call = elapsed / reps; `rounds` such windows per row, the rows alternating, after a warm-up window of each;
the median over the rounds is reported with the smallest and the largest.  The inputs do not influence the time.
`traffic_gb_s` is the memory traffic the three launches need by their shapes -- the holograms read once, T1 written and read, T2
written and read, the phase written: (20 D + 20) bytes per pixel and angle -- over the measured time: a rate of the call, launch
gaps included, not a kernel's share of peak.
"""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import adorym_amd as A                      # noqa: E402

ENERGY_EV, PSIZE_CM = 17050., 1e-4
ROWS = (('ctfinv_512x512x4_B1', (512, 512, 4), 1), ('ctfinv_512x512x4_B16', (512, 512, 4), 16), ('ctfinv_2048x2048x4_B1', (2048, 2048, 4), 1),
        ('ctf_fwd_adj_512x512x4', (512, 512, 4), 0))


def setup(ctx, shape, nb):
    ny, nx, nd = shape
    r = np.random.default_rng(0)
    dists = 40. + 50. * np.arange(nd) / max(nd - 1, 1)
    lgk = ctx.array(np.array([1.7], np.float32))
    data = ctx.array((1 + 0.05 * r.standard_normal((max(nb, 1), nd, ny, nx))).astype(np.float32) ** 2)
    if nb:
        eng = A.CTFInversion(ctx, (ny, nx), nd, ENERGY_EV, PSIZE_CM, max_batch=nb)
        out = ctx.empty((nb, ny, nx))
        return (lambda: eng.retrieve(data, dists, lgk, out=out)), (eng, data, out, lgk)
    eng = A.CTFEngine(ctx, (ny, nx), nd, ENERGY_EV, PSIZE_CM, raw_data_type='intensity')
    obj = ctx.array(np.stack([1e-2 * r.standard_normal((ny, nx)), 1e-3 * r.uniform(size=(ny, nx))], -1).astype(np.float32))
    g, gk = ctx.empty((ny, nx, 2)), ctx.empty((1,))
    one = data.view(0, (nd, ny, nx))
    return (lambda: eng.forward_adjoint(obj, dists, lgk, one, want_grad=True, grad_obj=g, grad_lg_kappa=gk, overwrite=True)), (eng, data, obj, g, gk, lgk)


def window(ev, fn, reps):
    ev[0].record()
    for _ in range(reps):
        fn()
    ev[1].record()
    ev[1].synchronize()
    return ev[0].elapsed_ms(ev[1]) / reps


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--reps', type=int, default=2000)
    ap.add_argument('--rounds', type=int, default=7)
    a = ap.parse_args()
    ctx = A.Context(0)
    ev = [ctx.event() for _ in range(2)]
    runs, keep, reps = {}, [], {}
    for name, shape, nb in ROWS:
        runs[name], k = setup(ctx, shape, nb)
        keep.append(k)
        reps[name] = a.reps if shape[0] * shape[1] * max(nb, 1) <= 512 * 512 else max(a.reps // 8, 10)
    t = {k: [] for k in runs}
    for k, fn in runs.items():
        window(ev, fn, max(reps[k] // 4, 5))          # warm-up: code objects, caches
    for _ in range(a.rounds):
        for k, fn in runs.items():
            t[k].append(window(ev, fn, reps[k]))
    for name, (ny, nx, nd), nb in ROWS:
        med = float(np.median(t[name]))
        row = dict(row=name, shape=[ny, nx, nd], n_batch=nb or None, reps=reps[name], rounds=a.rounds, ms=round(med, 5),
                   ms_range=[round(min(t[name]), 5), round(max(t[name]), 5)])
        if nb:
            row['ms_per_angle'] = round(med / nb, 5)
            row['traffic_gb_s'] = round((20 * nd + 20) * ny * nx * nb / (med * 1e-3) / 1e9, 1)
        print(json.dumps(row), flush=True)
    ctx.sync()


if __name__ == '__main__':
    main()
