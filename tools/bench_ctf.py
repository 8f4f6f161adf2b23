#!/usr/bin/env python3
"""
Time per minibatch of the CTF launch group (adm_ctf_fwd_adj, want_grad = 2: C1 ... C5) beside the Fresnel launch group
(adm_holo_fwd_adj, want_grad = 2, plane probe, no affine matrices, no distance gradient: K1 ... K5) in the same process, at
512 x 512 x 4 and 2048 x 2048 x 2.  Not the headline metric (bench.py is); prints one JSON object per shape.

    python tools/bench_ctf.py [--reps 200] [--rounds 7]        # on a GPU box

Method: device events around `reps` launch groups queued back to back (a group is five dependent kernels; nothing is read back
inside the window), ms per group = elapsed / reps; `rounds` such windows per engine, the two engines alternating, after a warm-up
window of each; the median over the rounds is reported with the smallest and the largest.  The inputs do not influence the time.
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
SHAPES = ((512, 512, 4), (2048, 2048, 2))


def setup(ctx, ny, nx, nd):
    r = np.random.default_rng(0)
    dists = 40. + 50. * np.arange(nd) / max(nd - 1, 1)
    data = ctx.array((1 + 0.05 * r.standard_normal((nd, ny, nx))).astype(np.float32) ** 2)
    # CTF: delta / beta object, lg_kappa on the device, distances as host doubles
    ctf = A.CTFEngine(ctx, (ny, nx), nd, ENERGY_EV, PSIZE_CM, raw_data_type='intensity')
    obj_db = ctx.array(np.stack([1e-2 * r.standard_normal((ny, nx)), 1e-3 * r.uniform(size=(ny, nx))], -1).astype(np.float32))
    lgk, g_db, g_k = ctx.array(np.array([1.7], np.float32)), ctx.empty((ny, nx, 2)), ctx.empty((1,))
    run_ctf = lambda: ctf.forward_adjoint(obj_db, dists, lgk, data, want_grad=True, grad_obj=g_db, grad_lg_kappa=g_k, overwrite=True)
    # Fresnel: real_imag object, plane probe, the object gradient only
    holo = A.HolographyEngine(ctx, (ny, nx), nd, ENERGY_EV, PSIZE_CM, unknown_type='real_imag', raw_data_type='intensity')
    obj_ri = ctx.array(np.stack([1 + 1e-2 * r.standard_normal((ny, nx)), 1e-2 * r.standard_normal((ny, nx))], -1).astype(np.float32))
    probe = ctx.array(np.stack([np.ones((ny, nx)), np.zeros((ny, nx))], -1).astype(np.float32))
    d_dev, g_ri = ctx.array(dists.astype(np.float32)), ctx.empty((ny, nx, 2))
    run_holo = lambda: holo.forward_adjoint(obj_ri, probe, d_dev, data, want_grad=True, grad_obj=g_ri, overwrite=True)
    return dict(ctf=run_ctf, fresnel=run_holo), (ctf, holo)


def window(ctx, ev, fn, reps):
    ev[0].record()
    for _ in range(reps):
        fn()
    ev[1].record()
    ev[1].synchronize()
    return ev[0].elapsed_ms(ev[1]) / reps


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--reps', type=int, default=200)
    ap.add_argument('--rounds', type=int, default=7)
    a = ap.parse_args()
    ctx = A.Context(0)
    ev = [ctx.event() for _ in range(2)]
    for ny, nx, nd in SHAPES:
        runs, keep = setup(ctx, ny, nx, nd)
        reps = a.reps if ny * nx <= 512 * 512 else max(a.reps // 8, 10)
        t = {k: [] for k in runs}
        for k, fn in runs.items():
            window(ctx, ev, fn, max(reps // 4, 5))          # warm-up: code objects, caches
        for _ in range(a.rounds):
            for k, fn in runs.items():
                t[k].append(window(ctx, ev, fn, reps))
        med = {k: float(np.median(v)) for k, v in t.items()}
        print(json.dumps(dict(shape=[ny, nx, nd], reps=reps, rounds=a.rounds,
                              ctf_ms=round(med['ctf'], 5), ctf_range=[round(min(t['ctf']), 5), round(max(t['ctf']), 5)],
                              fresnel_ms=round(med['fresnel'], 5), fresnel_range=[round(min(t['fresnel']), 5), round(max(t['fresnel']), 5)],
                              ctf_over_fresnel=round(med['ctf'] / med['fresnel'], 3))), flush=True)
        del runs, keep
    ctx.sync()


if __name__ == '__main__':
    main()
