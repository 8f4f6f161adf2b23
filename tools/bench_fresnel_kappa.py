#!/usr/bin/env python3
"""
The single-material constraint of Fresnel multi-distance holography (adm_kappa_tie.hip): what the tie and the fold cost alone, beside
adm_adam_step on arrays of the same size, and what they add to a whole evaluation on the two paths that serve them.  Not the headline
metric (bench.py is); prints one JSON object per line.

    python tools/bench_fresnel_kappa.py [--reps 50] [--rounds 7]        # on a GPU box

Kernel part, at 256^3 and 512^2 x 1 voxels.  Device events around `reps` launches queued back to back, ms per launch = elapsed /
reps; `rounds` such windows per variant, the variants alternating, after a warm-up window of each; the median over the rounds with
the smallest and the largest.  Each variant also as bytes per second on the bytes it MUST move per voxel (tie: 8 read + 8 written =
16; fold that adds, with the kappa sum: obj, tied gradient and gradient read, gradient written = 32, + its finishing kernel; fold that
sets: 24; Adam on the 2 floats of a voxel: 56) and as a fraction of 6.3 TB/s.  At 512^2 every array (2 MB) stays in the caches and
a launch is a few microseconds: that row measures launch cost, not memory.

Evaluation part, at the two shapes the README quotes: 256^2, 16 slices, 4 distances on the fan-out path (rotation, launch,
back-rotation) and 512^2, 4 distances on the field path.  Per shape, in one run and alternating: the bare launch (group) as
tools/bench_multidist3d.py and tools/bench_ctf.py time it; MultiDistModel.loss_and_gradients without the constraint; the same with it
(tie in front, fold behind, dL/dlg_kappa returned).  On the 2-D shape a model call is host-bound (its kernels take less time than
Python needs to queue them), so 'device_only' also times the launch group with the tie and the fold queued through the engine
classes alone: the difference of the two device-only rows is what the two passes add on the GPU.
"""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import adorym_amd as A                      # noqa: E402
from adorym_amd import _lib                 # noqa: E402

PEAK = 6.3e12
ENERGY_EV, PSIZE_CM = 8000., 1e-6
DISTS_CM = [1e-4, 2e-4, 3.5e-4, 5e-4]
SHAPES = {'256^3': 256 ** 3, '512^2x1': 512 ** 2}
BYTES = dict(tie=16, fold_add=32, fold_set=24, adam=56)


def window(ev, fn, reps):
    ev[0].record()
    for _ in range(reps):
        fn()
    ev[1].record()
    ev[1].synchronize()
    return ev[0].elapsed_ms(ev[1]) / reps


def alternate(ctx, runs, reps, rounds):
    ev = [ctx.event() for _ in range(2)]
    t = {k: [] for k in runs}
    for fn in runs.values():
        window(ev, fn, max(reps // 4, 5))
    for _ in range(rounds):
        for k, fn in runs.items():
            t[k].append(window(ev, fn, reps))
    return {k: dict(ms=round(float(np.median(tv)), 5), range=[round(min(tv), 5), round(max(tv), 5)]) for k, tv in t.items()}


def kernels(ctx, n_vox, reps, rounds):
    r = np.random.default_rng(0)
    mk = lambda: ctx.array((1e-3 * r.standard_normal((n_vox, 2))).astype(np.float32))
    obj, g, m, v = mk(), mk(), ctx.zeros((n_vox, 2)), ctx.zeros((n_vox, 2))
    ho = A.HomogeneousObject(ctx, (n_vox, 2))
    ho.tied_grad().copy_from(g)
    lg, gk = ctx.array(np.array([-1.5]), np.float32), ctx.zeros((1,))
    lib, h, chk = ctx.lib, ctx.handle, _lib.check
    runs = dict(tie=lambda: ho.tie(obj, lg), fold_add=lambda: ho.fold(obj, lg, g, gk), fold_set=lambda: ho.fold(obj, lg, g, gk, overwrite=True),
                adam=lambda: chk(lib.adm_adam_step(h, obj.ptr, g.ptr, m.ptr, v.ptr, 0, 2 * n_vox, 3, 1e-9, 0.9, 0.999, 1e-7, 0, None)))
    out = alternate(ctx, runs, reps, rounds)
    for k, o in out.items():
        rate = BYTES[k] * n_vox / (o['ms'] * 1e-3)
        o.update(tb_per_s=round(rate / 1e12, 3), of_peak=round(rate / PEAK, 3))
    return out


def evaluation(ctx, two_d, reps, rounds):
    r = np.random.default_rng(1)
    D = 4
    if two_d:
        Y = X = 512
        S = 1
    else:
        Y = X = 256
        S = 16
    obj = ctx.array(np.stack([2e-3 / S * r.uniform(size=(Y, X, S)), 2e-4 / S * r.uniform(size=(Y, X, S))], -1).astype(np.float32))
    data = (1 + 0.05 * np.abs(r.standard_normal((1, D, Y, X)))).astype(np.float32)
    probe = ctx.array(np.stack([np.ones((1, Y, X)), np.zeros((1, Y, X))], -1).astype(np.float32))
    lg = ctx.array(np.array([-1.5]), np.float32)
    ho = A.HomogeneousObject(ctx, (Y, X, S, 2))
    cv = dict(prj=data, forward_algorithm='fresnel', unknown_type='delta_beta', two_d_mode=two_d, theta_ls=np.linspace(0, np.pi, 4, dtype='float32'))
    if two_d:
        holo = A.HolographyEngine(ctx, (Y, X), D, ENERGY_EV, PSIZE_CM, unknown_type='delta_beta', raw_data_type='magnitude')
        eng = A.MultisliceEngine(ctx, (Y, X, 1), (8, 8), np.zeros((1, 2), int), ENERGY_EV, PSIZE_CM, free_prop_cm=0, max_batch=1)
        cv.update(engine=eng, holo_engine=holo)
        dists = ctx.array(np.array(DISTS_CM), np.float32)
        d_data, g = ctx.array(data[0]), ctx.empty((Y, X, S, 2))

        def bare():
            holo.forward_adjoint(obj, probe, dists, d_data, want_grad=True, grad_obj=g, overwrite=True)

        def bare_tied():
            holo.forward_adjoint(ho.tie(obj, lg), probe, dists, d_data, want_grad=True, grad_obj=ho.tied_grad(), overwrite=True)
            ho.fold(obj, lg, g, gk, overwrite=True)
    else:
        eng = A.MultisliceEngine(ctx, (Y, X, S), (Y, X), np.zeros((1, 2), int), ENERGY_EV, PSIZE_CM, free_prop_cm=DISTS_CM, max_batch=1, streamed=True,
                                 detector_fanout=True)
        table = A.RotationTable(ctx, (Y, X, S), float(cv['theta_ls'][1]))
        cv.update(engine=eng, holo_engine=None, rotation_tables=lambda i: table)
        dists = np.array(DISTS_CM)
        eng.set_batch(np.zeros((1, 2), int), data[0])
        eng.rotate(obj, None)
        g = ctx.empty((Y, X, S, 2))

        def bare():
            eng.multislice(probe, accumulate=False)
        bare_tied = None
    gk = ctx.zeros((1,))
    plain = A.MultiDistModel(device=ctx, common_vars_dict=dict(cv), raw_data_type='magnitude')
    tied = A.MultiDistModel(device=ctx, common_vars_dict=dict(cv, optimize_ctf_lg_kappa=True, homogeneous_object=ho), raw_data_type='magnitude')
    # (one angle of data; the fan-out path rotates it with the table of a quarter turn: the cost does not depend on the angle)
    args = (obj, probe, None, 0., None, 0, np.zeros((1, 2), int), None, np.zeros((D, 2)), np.array([0]), dists, 0, None, lg, None)
    i_k = tied.get_argument_index('ctf_lg_kappa')
    runs = dict(launch=bare)
    if bare_tied is not None:
        runs['launch_tie_fold_device_only'] = bare_tied
    runs['model'] = lambda: plain.loss_and_gradients([0], g, *args, _init_grad=True)
    runs['model_constrained'] = lambda: tied.loss_and_gradients([0, i_k], g, *args, _init_grad=True)
    out = alternate(ctx, runs, reps, rounds)
    plain.current_loss, tied.current_loss           # (resolve the pending read-backs)
    eng.plan.close()
    out['added_ms'] = round(out['model_constrained']['ms'] - out['model']['ms'], 5)
    if bare_tied is not None:
        out['added_device_only_ms'] = round(out['launch_tie_fold_device_only']['ms'] - out['launch']['ms'], 5)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--reps', type=int, default=50)
    ap.add_argument('--rounds', type=int, default=7)
    a = ap.parse_args()
    ctx = A.Context(0)
    for name, n_vox in SHAPES.items():
        reps = a.reps if n_vox > (1 << 21) else 20 * a.reps
        print(json.dumps(dict(part='kernels', shape=name, n_vox=n_vox, reps=reps, rounds=a.rounds, **kernels(ctx, n_vox, reps, a.rounds))), flush=True)
    print(json.dumps(dict(part='evaluation', path='fan-out', shape='256^2, 16 slices, 4 distances', reps=a.reps, rounds=a.rounds,
                          **evaluation(ctx, False, a.reps, a.rounds))), flush=True)
    print(json.dumps(dict(part='evaluation', path='field', shape='512^2, 4 distances', reps=10 * a.reps, rounds=a.rounds,
                          **evaluation(ctx, True, 10 * a.reps, a.rounds))), flush=True)
    ctx.close()


if __name__ == '__main__':
    main()
