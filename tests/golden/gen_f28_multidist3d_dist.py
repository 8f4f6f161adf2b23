"""Generates tests/golden/F28_multidist3d_dist.npz from the reference implementation (data only).

Usage: python tests/golden/gen_f28_multidist3d_dist.py        (needs the reference checkout that gen_goldens.py imports; CPU only)

Multi-distance holography of a 3-D object with the distances as parameters (optimize_free_prop: adorym/propagate.py:272-277, 556-568).

(a) kernel level: F27's four cases (gen_f27_multidist_3d.py: field 12 x 20, S = 5, D = 3, B = 3 over the object's edges; one and two
    modes, both sign conventions, magnitude and intensity data) through multislice_propagate_batch(..., optimize_free_prop=True,
    u_free, v_free) with the three distances as tensors that require grad.  The data are made at DISTS_CM, the model sits at
    DISTS_CM * (1.1, 0.92, 1.05) rounded to float32 (both precisions see the same values).  The fp64 results whole -- prediction,
    loss, gradients w.r.t. object, probe and free_prop_cm --, of the fp32 run only its distances from them.  The reference's own fp32
    dL/d free_prop_cm must lie within 1e-2 of its fp64 value in every case (asserted here: a looser yardstick lets anything pass).
(b) driver level: reconstruct_ptychography on F27's driver inputs with the object started at the truth and the distances at
    truth * (1.10, 0.92, 1.05), optimize_free_prop=True, free_prop_learning_rate=2e-6, learning_rate=1e-10, 8 epochs, fp64 and
    fp32: every loss, the distances after every update and the final object.
"""
import os
import sys
import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.join(HERE, '..', '..'))
import gen_goldens as G  # noqa: E402  (the I/O shims and the reference on sys.path)
import gen_f27_multidist_3d as F27  # noqa: E402
import torch  # noqa: E402
import adorym.global_settings as gs  # noqa: E402
from adorym.propagate import multislice_propagate_batch, gen_freq_mesh  # noqa: E402

ENERGY_EV, PSIZE_CM, PROBE, DISTS_CM = F27.ENERGY_EV, F27.PSIZE_CM, F27.PROBE, F27.DISTS_CM
OFF = (1.10, 0.92, 1.05)
MODEL_DISTS_CM = (np.array(DISTS_CM) * np.array(OFF)).astype(np.float32).astype(np.float64)      # exact in either precision


def ref_forward(obj, pos, pr, pi, sg, dists, uv):
    """gen_f27_multidist_3d.ref_forward with the distances as tensors through fresnel_propagate_wrapped."""
    Py, Px = PROBE
    Y, X = obj.shape[:2]
    py0, px0 = max(0, -int(pos[:, 0].min())), max(0, -int(pos[:, 1].min()))
    py1, px1 = max(0, int(pos[:, 0].max()) + Py - Y), max(0, int(pos[:, 1].max()) + Px - X)
    padded = torch.stack([torch.nn.functional.pad(obj[..., c], (0, 0, px0, px1, py0, py1), value=0.) for c in range(2)], -1)
    tiles = torch.stack([padded[y + py0:y + py0 + Py, x + px0:x + px0 + Px] for y, x in pos])
    mags = []
    for d in dists:
        inten = 0
        for m in range(pr.shape[0]):
            er, ei = multislice_propagate_batch(tiles, pr[m][None], pi[m][None], ENERGY_EV, PSIZE_CM, free_prop_cm=d, type='delta_beta',
                                                sign_convention=sg, optimize_free_prop=True, u_free=uv[0], v_free=uv[1])
            inten = inten + er ** 2 + ei ** 2
        mags.append(torch.sqrt(inten))
    return torch.stack(mags, 1).reshape(len(pos) * len(dists), Py, Px)


def gen_kernel_cases(out):
    rel = lambda a, b: float(np.linalg.norm(np.asarray(a, np.complex128) - b) / np.linalg.norm(b))
    u, v = gen_freq_mesh(np.array([PSIZE_CM * 1e7] * 3), PROBE)
    for name, (sg, M, rdt) in F27.KERNEL_CASES.items():
        inp = F27.kernel_inputs(name)
        res = {}
        for fp64 in (True, False):
            gs.run_fp64 = fp64
            dt = torch.float64 if fp64 else torch.float32
            T = lambda a, g=False: torch.tensor(np.asarray(a, dtype=np.float64), dtype=dt, requires_grad=g)
            uv = (T(u), T(v))
            if fp64:
                with torch.no_grad():       # the data: the truth at the TRUE distances
                    meas = ref_forward(T(inp['truth']), inp['pos'], T(inp['probes'].real), T(inp['probes'].imag), sg,
                                       [T(d) for d in DISTS_CM], uv)
                    meas = meas ** 2 if rdt == 'intensity' else meas
            obj, pr, pi = T(inp['obj'], True), T(inp['probes'].real, True), T(inp['probes'].imag, True)
            dists = [T(d, True) for d in MODEL_DISTS_CM]
            pred = ref_forward(obj, inp['pos'], pr, pi, sg, dists, uv)
            loss = F27.ref_loss(pred, meas.to(dt), rdt)
            g = torch.autograd.grad(loss, [obj, pr, pi] + dists)
            res[fp64] = dict(pred=pred.detach().numpy(), loss=float(loss.detach()), grad=g[0].numpy(), gprobe=g[1].numpy() + 1j * g[2].numpy(),
                             gdists=np.array([float(x) for x in g[3:]]))
        r64, r32 = res[True], res[False]
        for k in ('obj', 'pos', 'probes'):
            out['%s/%s' % (name, k)] = inp[k]
        out[name + '/meas'] = meas.numpy()
        for k in ('pred', 'loss', 'grad', 'gprobe', 'gdists'):
            out['%s/%s' % (name, k)] = np.asarray(r64[k])
        # the reference's own fp32 run, as distances from its fp64 run: pred, loss, grad, gprobe (whole), gdists (whole)
        out[name + '/err32'] = np.array([rel(r32['pred'], r64['pred']), abs(r32['loss'] / r64['loss'] - 1), rel(r32['grad'], r64['grad']),
                                         rel(r32['gprobe'], r64['gprobe']), rel(r32['gdists'], r64['gdists'])])
        print(name, 'loss %.6g  dL/dd' % r64['loss'], r64['gdists'], '; fp32 vs fp64: pred %.1e loss %.1e grad %.1e gprobe %.1e gdists %.1e'
              % tuple(out[name + '/err32']))
        assert out[name + '/err32'][4] < 1e-2, (name, 'the fp32 reference is no yardstick for dL/dd here: choose other seeds')
    out['kernel_cases'] = np.array(sorted(F27.KERNEL_CASES))
    out['kernel_case_params'] = np.array([repr(F27.KERNEL_CASES[k]) for k in sorted(F27.KERNEL_CASES)])
    out['kernel_data_dists_cm'] = np.array(DISTS_CM)
    out['kernel_dists_cm'] = MODEL_DISTS_CM


# ----------------------------------------------------------------------------------------------------------------- (b) the driver
DRV = dict(F27.DRV, n_epochs=8, learning_rate=1e-10, free_prop_learning_rate=2e-6, dists_off=OFF)


def gen_driver(out):
    import adorym.ptychography as PT
    from oracle import adorym_oracle as O
    from tests import multidist3d_ref as MR
    N, n_theta, dists = DRV['N'], DRV['n_theta'], list(DRV['dists_cm'])
    truth, _, pm, pp = F27.driver_inputs()
    theta_ls = np.linspace(0, np.pi, n_theta, dtype='float32')
    phys = O.Physics((N, N), ENERGY_EV, PSIZE_CM, free_prop_cm=dists[0])
    probe = pm * np.exp(1j * pp)
    pos = np.array([(0., 0.)])
    prj = np.zeros((n_theta, len(dists), N, N))
    for it, th in enumerate(theta_ls):
        rot = O.rotate_fwd(truth, O.rotation_coords((N, N, N), th), 'float64')
        tiles, _ = O.extract_tiles(rot, pos.astype(int), (N, N))
        prj[it] = MR.predict(tiles, probe, phys, dists)
    out['drv/prj'] = prj.astype(np.float32)
    out['drv/probe_mag'], out['drv/probe_phase'] = pm, pp
    # the object starts at the truth (float32: exact in either precision), the distances off it
    guess = truth.astype(np.float32).astype(np.float64)
    out['drv/guess_delta'], out['drv/guess_beta'] = guess[..., 0], guess[..., 1]
    out['drv/dists_true_cm'] = np.array(dists)
    out['drv/dists0_cm'] = MODEL_DISTS_CM
    prj = out['drv/prj'].astype(np.float64)
    orig_up = PT.update_parameters
    final, trace = {}, {}
    for fp64 in (True, False):
        gs.run_fp64 = fp64
        rec = {}

        def rec_up(opt_ls, optimizable_params, kw, _rec=rec):
            res = orig_up(opt_ls, optimizable_params, kw)
            _rec.setdefault('dist_trace', []).append(res['free_prop_cm'].detach().numpy().astype(np.float64).copy())
            return res
        PT.update_parameters = rec_up
        extra = dict(minibatch_size=1, n_epochs=DRV['n_epochs'], optimizer='adam', learning_rate=DRV['learning_rate'], energy_ev=ENERGY_EV,
                     psize_cm=PSIZE_CM, free_prop_cm=np.array(MODEL_DISTS_CM), initial_guess=[guess[..., 0], guess[..., 1]],
                     probe_type='supplied', probe_initial=[pm, pp], two_d_mode=False, safe_zone_width=0, n_dp_batch=1, run_float64=fp64,
                     optimize_free_prop=True, free_prop_learning_rate=DRV['free_prop_learning_rate'], forward_model=F27.MultiDistPlugin)
        try:
            G.run_driver(prj, (N, N, N), pos, np.pi, n_theta, extra, rec)
        finally:
            PT.update_parameters = orig_up
        tag = 'drv/%s/' % ('fp64' if fp64 else 'fp32')
        out[tag + 'losses'] = rec['losses']
        trace[fp64] = np.stack(rec['dist_trace'])
        final[fp64] = np.stack([rec['delta'], rec['beta']], -1).astype(np.float64)
        if fp64:
            for i, tl in enumerate(rec['task_lists']):
                for j, t in enumerate(tl):
                    out['drv/tasks_%d_%d' % (i, j)] = t
        print(tag, 'losses', rec['losses'][[0, -1]], 'distances', trace[fp64][-1])
    gs.run_fp64 = False
    out['drv/fp64/dists'] = trace[True]                                     # [updates, D]
    out['drv/fp32/dists_err'] = np.abs(trace[False] - trace[True])         # the fp32 run's distance from it, per update and distance
    out['drv/fp64/obj'] = final[True]
    out['drv/fp32/obj_err'] = np.array(np.abs(final[False] - final[True]).max())
    err = (trace[True][-1] - np.array(dists)) / (MODEL_DISTS_CM - np.array(dists))
    print('final distance errors relative to the starting errors:', err)
    out['drv/params'] = np.array(repr(DRV))


if __name__ == '__main__':
    out = {}
    gen_kernel_cases(out)
    gen_driver(out)
    G.save('F28_multidist3d_dist', **out)
