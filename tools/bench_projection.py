"""Time the projection approximation (pure_projection=True, adorym_amd.ProjectionEngine) at config 3's shape -- 256^3 object, 72 x 72
probe, 32 positions per minibatch, far field -- with device events after warm-up:

    project_z / project_z_adj   the two kernels of adm_project.hip alone, on the minibatch's row footprint and on all 256 rows.  They
                                are timed ALTERNATELY (sum, broadcast, sum, ...), each between its own pair of events: the sum reads
                                obj_rot, the broadcast writes grad_rot, and the two buffers together (2 x 176 MB of rows at 256^3)
                                exceed the 256 MiB Infinity Cache, so neither is served from it.  On the minibatch's footprint
                                (2 x 58 MB) they are: that figure is the one the step sees, and not an HBM rate.
    step_projection             rotate -> sum -> one-slice launch -> overlap-add -> broadcast -> back-rotate of one minibatch
    step_multislice             the same minibatch through MultisliceEngine (255 Fresnel propagations per position): the parent's step

Bytes: the sum reads Z * n and writes n, the broadcast reads n and writes Z * n, n = rows * Xp * 8 bytes.  `frac_of_6.3TBps` is that
over the kernel's time over 6.3 TB/s (the achievable HBM rate).  One JSON line.

    python tools/bench_projection.py [--iters 20] [--warmup 3] [--repeats 3]
"""
import argparse
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np

HBM_ACHIEVABLE = 6.3e12


def kernel_pair_ms(ctx, eng, lo, hi, iters):
    """(ms of adm_project_z, ms of adm_project_z_adj) per call, alternating, each between its own events."""
    from adorym_amd._lib import check
    lib, h = ctx.lib, eng.plan.handle
    ev = [ctx.event() for _ in range(3 * iters)]
    for i in range(iters):
        ev[3 * i].record()
        check(lib.adm_project_z(h, eng.obj_rot.ptr, lo, hi, eng.slab.obj_rot.ptr))
        ev[3 * i + 1].record()
        check(lib.adm_project_z_adj(h, eng.slab.grad_rot.ptr, lo, hi, eng.grad_rot.ptr))
        ev[3 * i + 2].record()
    ctx.sync()
    fwd = [ev[3 * i].elapsed_ms(ev[3 * i + 1]) for i in range(iters)]
    adj = [ev[3 * i + 1].elapsed_ms(ev[3 * i + 2]) for i in range(iters)]
    return float(np.median(fwd)), float(np.median(adj))


def step_ms(ctx, step, iters):
    e0, e1 = ctx.event(), ctx.event()
    e0.record()
    for _ in range(iters):
        step()
    e1.record()
    return e0.elapsed_ms(e1) / iters


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--iters', type=int, default=20)
    ap.add_argument('--warmup', type=int, default=3)
    ap.add_argument('--repeats', type=int, default=3)
    a = ap.parse_args()
    import adorym_amd as A
    from adorym_amd import workloads as W
    cfg = W.c3_config()
    ctx = A.Context(0)
    size, P, B = cfg['obj_size'], cfg['probe_size'], cfg['minibatch_size']
    pos_all = cfg['probe_pos']
    pos = pos_all[230:230 + B]                    # a minibatch from the middle of the scan: 23 positions of one row, 9 of the next
    r = np.random.default_rng(0)
    common = dict(free_prop_cm=cfg['free_prop_cm'], max_batch=B)
    engines = {'projection': A.ProjectionEngine(ctx, size, P, pos_all, cfg['energy_ev'], cfg['psize_cm'], **common),
               'multislice': A.MultisliceEngine(ctx, size, P, pos_all, cfg['energy_ev'], cfg['psize_cm'], transmissions_only=True, **common)}
    obj = ctx.array(W.foam_object(size).astype(np.float32))
    grad = ctx.zeros(size + (2,))
    probe = ctx.array(W.probe_array(cfg)[None])
    gp = ctx.zeros((1,) + tuple(P) + (2,))
    table = A.RotationTable(ctx, size, 0.3)
    target = r.uniform(0, 2, (B,) + tuple(P)).astype(np.float32)
    steps = {}
    for name, eng in engines.items():
        eng.set_batch(pos, target)
        yr = eng.y_footprint(pos)

        def step(eng=eng, yr=yr):
            eng.rotate(obj, table, yr)
            eng.multislice(probe, grad_probe=gp)
            eng.rotate_adjoint(grad, table, yr)
        steps[name] = step
        for _ in range(a.warmup):
            step()
    pe = engines['projection']
    Z, Yp, Xp, _ = pe.plan.rot_shape
    out = dict(shape='C3 256^3, probe 72x72, B=%d, far field' % B, Z=Z, Xp=Xp, footprint=list(yr), iters=a.iters, repeats=a.repeats)
    for tag, (lo, hi) in (('footprint', yr), ('all_rows', (0, size[0]))):
        kernel_pair_ms(ctx, pe, lo, hi, a.warmup)
        runs = [kernel_pair_ms(ctx, pe, lo, hi, a.iters) for _ in range(a.repeats)]
        n = (hi - lo) * Xp * 8
        for k, name in enumerate(('project_z', 'project_z_adj')):
            ms = float(np.median([x[k] for x in runs]))
            out['%s_%s' % (name, tag)] = dict(ms=round(ms, 4), spread_ms=round(max(x[k] for x in runs) - min(x[k] for x in runs), 4),
                                              MB=round((Z + 1) * n / 1e6, 1), TBps=round((Z + 1) * n / (ms * 1e-3) / 1e12, 3),
                                              frac_of_6p3TBps=round((Z + 1) * n / (ms * 1e-3) / HBM_ACHIEVABLE, 3))
    ms = {name: [] for name in steps}
    for _ in range(a.repeats):
        for name, step in steps.items():
            ms[name].append(step_ms(ctx, step, a.iters))
    for name in steps:
        out['step_%s_ms' % name] = round(float(np.median(ms[name])), 4)
        out['step_%s_spread_ms' % name] = round(max(ms[name]) - min(ms[name]), 4)
        out['loss_%s' % name] = engines[name].loss()
    out['step_ratio_multislice_over_projection'] = round(out['step_multislice_ms'] / out['step_projection_ms'], 2)
    print(json.dumps(out), flush=True)
    pe.close()
    engines['multislice'].plan.close()
    ctx.close()


if __name__ == '__main__':
    main()
