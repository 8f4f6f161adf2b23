"""Time the fused rotate-and-project kernels (adm_rotate_project.hip) against the unfused pairs they replace, and the whole
evaluation of the 3-D CTF model (adorym_amd.RotatedProjector + CTFEngine, 4 distances), on N^3 objects, all rows, with device events
after warm-up -- the method of tools/bench_projection.py: `iters` calls per repeat, the kinds interleaved inside every repeat, the
median over the repeats and the spread between them.

    fused_fwd      adm_rotate_project_fwd                        reads the object once, writes one row per plane
    unfused_fwd    adm_rotate_fwd + adm_project_z                reads the object, writes and reads the [Z] rotated frame
    fused_adj      adm_rotate_project_adj                        reads one row per plane and the tables, read-modify-writes the gradient
    unfused_adj    adm_project_z_adj + adm_rotate_adj_staged     writes and reads the [Z] broadcast volume as well
    evaluation     project -> adm_ctf_fwd_adj (want_grad = 2) -> backproject

`MB` is the traffic the algorithm needs (object or gradient, image, tables; the unfused pairs: the [Z] frame written and read as
well), `frac_of_6p3TBps` that over the time over 6.3 TB/s (the achievable HBM rate).  A 256^3 object (134 MB) fits the 256 MiB
Infinity Cache, a 512^3 one (1074 MB) does not.  One JSON line per size.

    python tools/bench_ctf_tomo.py [--sizes 256 512] [--theta 0.3] [--iters 20] [--warmup 3] [--repeats 3]
"""
import argparse
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np

HBM_ACHIEVABLE = 6.3e12


def timed(ctx, fn, iters):
    e0, e1 = ctx.event(), ctx.event()
    e0.record()
    for _ in range(iters):
        fn()
    e1.record()
    ctx.sync()
    return e0.elapsed_ms(e1) / iters


def bench_size(A, ctx, N, theta, a):
    from adorym_amd._lib import check
    from adorym_amd.device import DeviceArray
    size = (N, N, N)
    lib = ctx.lib
    rp = A.RotatedProjector(ctx, size)
    h = rp.plan.handle
    table = A.RotationTable(ctx, size, theta)
    r = np.random.default_rng(0)
    obj = DeviceArray(ctx, size + (2,), np.float32)
    plane = (r.standard_normal((N, N, 2)) * 1e-3 / N).astype(np.float32)
    for y in range(N):          # (one random plane repeated: the timing does not depend on the values)
        obj.view(y * plane.size, plane.shape).set(plane)
    grad = ctx.zeros(size + (2,))
    rot = DeviceArray(ctx, rp.plan.rot_shape, np.float32)          # the [Z] buffer only the unfused pairs need
    img = ctx.zeros((N, N, 2))
    gimg = ctx.array(r.standard_normal((N, N, 2)).astype(np.float32))
    p, s, ls, w, b = [x.ptr for x in table.csr(rp.plan)]
    lanes_x = int(table.lanes_along_x)
    D = 4
    ctf = A.CTFEngine(ctx, (N, N), D, 17000., 1e-4)
    dists = np.array([1., 2., 4., 8.])
    lgk = ctx.array(np.array([1.5], np.float32))
    data = ctx.array(np.ones((D, N, N), np.float32))
    gk = ctx.zeros((1,))

    def fused_fwd():
        check(lib.adm_rotate_project_fwd(h, obj.ptr, table.ptr, img.ptr, 0, N))

    def unfused_fwd():
        check(lib.adm_rotate_fwd(h, obj.ptr, table.ptr, rot.ptr, 0, N))
        check(lib.adm_project_z(h, rot.ptr, 0, N, img.ptr))

    def fused_adj():
        check(lib.adm_rotate_project_adj(h, gimg.ptr, p, s, w, grad.ptr, 0, N, lanes_x))

    def unfused_adj():
        check(lib.adm_project_z_adj(h, gimg.ptr, 0, N, rot.ptr))
        check(lib.adm_rotate_adj_staged(h, rot.ptr, p, s, ls, w, b, grad.ptr, 0, N))

    def evaluation():
        pr = rp.project(obj, table)
        ctf.forward_adjoint(pr, dists, lgk, data, want_grad=True, grad_obj=gimg, grad_lg_kappa=gk, overwrite=True)
        rp.backproject(gimg, table, grad)

    kinds = dict(fused_fwd=fused_fwd, unfused_fwd=unfused_fwd, fused_adj=fused_adj, unfused_adj=unfused_adj, evaluation=evaluation)
    for fn in kinds.values():
        for _ in range(a.warmup):
            fn()
    ctx.sync()
    ms = {k: [] for k in kinds}
    for _ in range(a.repeats):
        for k, fn in kinds.items():
            ms[k].append(timed(ctx, fn, a.iters))
    vol, image, tables = N ** 3 * 8, N * N * 8, N * N * (4 + 4 * 8)
    need = dict(fused_fwd=vol + image, unfused_fwd=3 * vol + image, fused_adj=2 * vol + image + tables, unfused_adj=4 * vol + image + tables)
    out = dict(shape='%d^3, all rows' % N, theta=theta, iters=a.iters, repeats=a.repeats)
    for k in kinds:
        med = float(np.median(ms[k]))
        out[k] = dict(ms=round(med, 4), spread_ms=round(max(ms[k]) - min(ms[k]), 4))
        if k in need:
            out[k].update(MB=round(need[k] / 1e6, 1), frac_of_6p3TBps=round(need[k] / (med * 1e-3) / HBM_ACHIEVABLE, 3))
    for d in ('fwd', 'adj'):
        f, u = out['fused_' + d], out['unfused_' + d]
        out['fused_%s_wins' % d] = bool(u['ms'] - f['ms'] > max(f['spread_ms'], u['spread_ms']))
    print(json.dumps(out), flush=True)
    rp.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--sizes', type=int, nargs='+', default=[256, 512])
    ap.add_argument('--theta', type=float, default=0.3)
    ap.add_argument('--iters', type=int, default=20)
    ap.add_argument('--warmup', type=int, default=3)
    ap.add_argument('--repeats', type=int, default=3)
    a = ap.parse_args()
    import adorym_amd as A
    ctx = A.Context(0)
    for N in a.sizes:
        bench_size(A, ctx, N, a.theta, a)
    ctx.close()


if __name__ == '__main__':
    main()
