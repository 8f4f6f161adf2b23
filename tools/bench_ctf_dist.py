#!/usr/bin/env python3
"""
Time per minibatch of the CTF launch group with the distances on the device and their gradient (adm_ctfd_fwd_adj, want_grad = 2),
beside the group through the old entry (adm_ctf_fwd_adj) and the two registration launches that optimize_prj_affine puts around it
(adm_register_targets in front, adm_register_grad behind), in the same process, at 512 x 512 x 4.  Not the headline metric
(bench.py is); prints one JSON object.

    python tools/bench_ctf_dist.py [--reps 200] [--rounds 7]        # on a GPU box
    ADM_LIB_PATH=adorym_amd/libadm_X.so python tools/bench_ctf_dist.py --old-only        # the old entry of another build, for comparison

Method: tools/bench_ctf.py's -- device events around `reps` launch groups queued back to back, ms per group = elapsed / reps;
`rounds` such windows per variant, the variants alternating, after a warm-up window of each; the median over the rounds is reported
with the smallest and the largest.  The inputs do not influence the time.
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
SHAPE = (512, 512, 4)


def setup(ctx, ny, nx, nd, old_only):
    r = np.random.default_rng(0)
    dists = 40. + 50. * np.arange(nd) / max(nd - 1, 1)
    data = ctx.array((1 + 0.05 * r.standard_normal((nd, ny, nx))).astype(np.float32) ** 2)
    obj = ctx.array(np.stack([1e-2 * r.standard_normal((ny, nx)), 1e-3 * r.uniform(size=(ny, nx))], -1).astype(np.float32))
    lgk, g, gk, gd = ctx.array(np.array([1.7], np.float32)), ctx.empty((ny, nx, 2)), ctx.empty((1,)), ctx.empty((nd,))
    plain = A.CTFEngine(ctx, (ny, nx), nd, ENERGY_EV, PSIZE_CM, raw_data_type='intensity')
    runs = dict(old=lambda: plain.forward_adjoint(obj, dists, lgk, data, want_grad=True, grad_obj=g, grad_lg_kappa=gk, overwrite=True))
    keep = [plain]
    if not old_only:
        eng = A.CTFEngine(ctx, (ny, nx), nd, ENERGY_EV, PSIZE_CM, raw_data_type='intensity', refine_distances=True, dists_cm=dists)
        runs['new'] = lambda: eng.forward_adjoint(obj, eng.dists, lgk, data, want_grad=True, grad_obj=g, grad_lg_kappa=gk, overwrite=True)
        runs['new_grad_dists'] = lambda: eng.forward_adjoint(obj, eng.dists, lgk, data, want_grad=True, grad_obj=g, grad_lg_kappa=gk,
                                                             grad_dists=gd, overwrite=True)
        # the registration launches alone: targets in front of the group, the matrices' gradient from its predictions behind it
        reg = A.HologramRegistration(ctx, nd, (ny, nx), 'intensity')
        theta = ctx.array(np.tile(np.array([[1.01, 0.01, 0.02], [-0.01, 0.99, -0.01]], np.float32), (nd, 1, 1)))
        pred, ga = ctx.array(np.ones((nd, ny, nx), np.float32)), ctx.zeros((nd, 2, 3))

        def registration():
            reg.targets(data, theta)
            reg.grad(data, theta, pred, ga)
        runs['registration'] = registration
        keep += [eng, reg]
    return runs, keep


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
    ap.add_argument('--old-only', action='store_true')
    a = ap.parse_args()
    ctx = A.Context(0)
    ev = [ctx.event() for _ in range(2)]
    ny, nx, nd = SHAPE
    runs, keep = setup(ctx, ny, nx, nd, a.old_only)
    t = {k: [] for k in runs}
    for k, fn in runs.items():
        window(ctx, ev, fn, max(a.reps // 4, 5))          # warm-up: code objects, caches
    for _ in range(a.rounds):
        for k, fn in runs.items():
            t[k].append(window(ctx, ev, fn, a.reps))
    out = dict(shape=[ny, nx, nd], reps=a.reps, rounds=a.rounds, lib=os.path.basename(A._lib.LIB_PATH))
    for k, v in t.items():
        out[k + '_ms'] = round(float(np.median(v)), 5)
        out[k + '_range'] = [round(min(v), 5), round(max(v), 5)]
    print(json.dumps(out), flush=True)
    ctx.sync()


if __name__ == '__main__':
    main()
