"""Generates tests/golden/F29_multidist3d_affine.npz from the reference implementation (data only).

Usage: python tests/golden/gen_f29_multidist3d_affine.py        (needs the reference checkout that gen_goldens.py imports; CPU only)

Multi-distance holography of a 3-D object with the affine registration of the measured holograms (optimize_prj_affine:
adorym/forward_model.py:1066-1072, w.affine_transform wrappers.py:1159-1174).

(a) kernel level: F27's four cases (gen_f27_multidist_3d.py: field 12 x 20, S = 5, D = 3, B = 3 over the object's edges; one and two
    modes, both sign conventions, magnitude and intensity data).  The data of distance d go through w.affine_transform with matrix d
    as a tensor that requires grad, as MultiDistModel's loss function does it; matrix 0 is the identity, matrices 1 and 2 a small
    rotation + scale + shift, every entry rounded to float32 (both precisions see the same values).  The fp64 results whole --
    prediction, registered target, loss, gradients w.r.t. object, probe and the matrices --, of the fp32 run only its distances
    from them.  The reference's own fp32 dL/dtheta of every FREE matrix (1, 2) must lie within 1e-2 of its fp64 value in every
    case (asserted here: a looser yardstick lets anything pass; matrices that break it are replaced).  Matrix 0 cannot be held
    to that: at the identity every sampling point sits on a pixel centre, where the last bit of the coordinate decides which
    one-sided derivative grid_sample's backward sees, and the reference's own fp32 and fp64 gradients of matrix 0 are 0.2 to 0.9
    apart on these data.  The identity stays (the reference pins matrix 0 to it and never uses that gradient); the fp32 run's
    gradient is stored whole beside the fp64 one ('gtheta32'), its per-matrix distances in err32[6:], and the GPU tests judge
    matrix 0 against float32 arithmetic.
(b) driver level: reconstruct_ptychography on F27's driver inputs with the object started at the truth, holograms 1 and 2 warped by
    known matrices (tests/multidist3d_affine_ref.warp) and the run started at the identity with optimize_prj_affine=True, fp64 and
    fp32: every loss, the matrices after every update and the final object.  The matrices that undo the warp (the inverse maps)
    are the truth; the fp64 run must bring each free matrix's Frobenius distance from it below 1/4 of the starting one (asserted).
(c) the same with the distances refined as well (optimize_free_prop, F28's starting distances): the reference demo's feature set.

The reference's own driver runs (b) and (c) with a 3-D object through the forward_model= plugin of gen_f27_multidist_3d.py; nothing
in the reference is patched.
"""
import os
import sys
import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.join(HERE, '..', '..'))
import gen_goldens as G  # noqa: E402  (the I/O shims and the reference on sys.path)
import gen_f27_multidist_3d as F27  # noqa: E402
import gen_f28_multidist3d_dist as F28  # noqa: E402
import torch  # noqa: E402
import adorym.global_settings as gs  # noqa: E402
import adorym.wrappers as w  # noqa: E402
from tests import multidist3d_affine_ref as AR  # noqa: E402

ENERGY_EV, PSIZE_CM, PROBE, DISTS_CM = F27.ENERGY_EV, F27.PSIZE_CM, F27.PROBE, F27.DISTS_CM
# matrix 0 the identity (the reference pins it), 1 and 2 rotation + scale + shift (normalised coordinates), float32-representable
KERNEL_THETA = np.stack([AR.IDENTITY, AR.matrix(0.03, 1.04, (0.05, -0.03)), AR.matrix(-0.02, 0.97, (-0.04, 0.06))])


def ref_register(meas, theta, n_dists):
    """forward_model.py:1066-1072 on position-major data [B * D, Py, Px]: all images of distance d through w.affine_transform with
    matrix d; back in position-major order."""
    out = [w.affine_transform(meas[d::n_dists], theta[d], override_backend='pytorch') for d in range(n_dists)]
    return torch.stack(out, 1).reshape(meas.shape)


def gen_kernel_cases(out):
    rel = lambda a, b: float(np.linalg.norm(np.asarray(a, np.complex128) - b) / np.linalg.norm(b))
    D = len(DISTS_CM)
    for name, (sg, M, rdt) in F27.KERNEL_CASES.items():
        inp = F27.kernel_inputs(name)
        res = {}
        for fp64 in (True, False):
            gs.run_fp64 = fp64
            dt = torch.float64 if fp64 else torch.float32
            T = lambda a, g=False: torch.tensor(np.asarray(a, dtype=np.float64), dtype=dt, requires_grad=g)
            if fp64:
                with torch.no_grad():       # the data: the truth's holograms
                    meas = F27.ref_forward(T(inp['truth']), inp['pos'], T(inp['probes'].real), T(inp['probes'].imag), sg)
                    meas = meas ** 2 if rdt == 'intensity' else meas
            obj, pr, pi = T(inp['obj'], True), T(inp['probes'].real, True), T(inp['probes'].imag, True)
            theta = T(KERNEL_THETA, True)
            pred = F27.ref_forward(obj, inp['pos'], pr, pi, sg)
            samp = ref_register(torch.abs(meas.to(dt)), theta, D)
            loss = F27.ref_loss(pred, samp, rdt)
            g = torch.autograd.grad(loss, [obj, pr, pi, theta])
            t = torch.abs(samp.detach())
            res[fp64] = dict(pred=pred.detach().numpy(), loss=float(loss.detach()), grad=g[0].numpy(), gprobe=g[1].numpy() + 1j * g[2].numpy(),
                             gtheta=g[3].numpy(), target=(torch.sqrt(t) if rdt == 'intensity' else t).numpy())
        r64, r32 = res[True], res[False]
        for k in ('obj', 'pos', 'probes'):
            out['%s/%s' % (name, k)] = inp[k]
        out[name + '/meas'] = meas.numpy()
        for k in ('pred', 'target', 'loss', 'grad', 'gprobe', 'gtheta'):
            out['%s/%s' % (name, k)] = np.asarray(r64[k])
        # the reference's own fp32 run, as distances from its fp64 run: pred, loss, grad, gprobe, gtheta of the FREE matrices (1 ...),
        # target, then gtheta per matrix (0 ... D-1)
        out[name + '/err32'] = np.array([rel(r32['pred'], r64['pred']), abs(r32['loss'] / r64['loss'] - 1), rel(r32['grad'], r64['grad']),
                                         rel(r32['gprobe'], r64['gprobe']), rel(r32['gtheta'][1:], r64['gtheta'][1:]),
                                         rel(r32['target'], r64['target'])] + [rel(r32['gtheta'][d], r64['gtheta'][d]) for d in range(D)])
        out[name + '/gtheta32'] = r32['gtheta'].astype(np.float64)          # (matrix 0: the identity's gradient as float32 torch sees it)
        print(name, 'loss %.6g; fp32 vs fp64: pred %.1e loss %.1e grad %.1e gprobe %.1e gtheta[1:] %.1e target %.1e; per matrix'
              % ((r64['loss'],) + tuple(out[name + '/err32'][:6])), out[name + '/err32'][6:])
        assert out[name + '/err32'][4] < 1e-2 and np.all(out[name + '/err32'][7:] < 1e-2), \
            (name, 'the fp32 reference is no yardstick for dL/dtheta here: choose other matrices')
    out['kernel_cases'] = np.array(sorted(F27.KERNEL_CASES))
    out['kernel_case_params'] = np.array([repr(F27.KERNEL_CASES[k]) for k in sorted(F27.KERNEL_CASES)])
    out['kernel_dists_cm'] = np.array(DISTS_CM)
    out['kernel_theta'] = KERNEL_THETA


# ----------------------------------------------------------------------------------------------------------------- (b), (c) the driver
# the warps of holograms 1 and 2 (hologram 0 is the anchor: its matrix is pinned to the identity)
WARP = np.stack([AR.IDENTITY, AR.matrix(0.04, 1.06, (0.22, -0.16)), AR.matrix(-0.05, 0.94, (-0.14, 0.16))])
DRV = dict(F27.DRV, n_epochs=20, learning_rate=1e-10, prj_affine_learning_rate=1e-2)
DRV_BOTH = dict(DRV, n_epochs=8, free_prop_learning_rate=2e-6, dists_off=F28.OFF)      # (F28's epoch count and distance step)


def driver_data():
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
        prj[it] = AR.warp(MR.predict(tiles, probe, phys, dists), WARP)
    return truth, pm, pp, prj.astype(np.float32)


def run_reference(prj, guess, pm, pp, par, dists0, fp64, both):
    import adorym.ptychography as PT
    N, n_theta = par['N'], par['n_theta']
    orig_up = PT.update_parameters
    rec = {}

    def rec_up(opt_ls, optimizable_params, kw, _rec=rec):
        res = orig_up(opt_ls, optimizable_params, kw)
        _rec.setdefault('theta_trace', []).append(res['prj_affine_ls'].detach().numpy().astype(np.float64).copy())
        if both:
            _rec.setdefault('dist_trace', []).append(res['free_prop_cm'].detach().numpy().astype(np.float64).copy())
        return res
    PT.update_parameters = rec_up
    gs.run_fp64 = fp64
    extra = dict(minibatch_size=1, n_epochs=par['n_epochs'], optimizer='adam', learning_rate=par['learning_rate'], energy_ev=ENERGY_EV,
                 psize_cm=PSIZE_CM, free_prop_cm=np.array(dists0), initial_guess=[guess[..., 0], guess[..., 1]],
                 probe_type='supplied', probe_initial=[pm, pp], two_d_mode=False, safe_zone_width=0, n_dp_batch=1, run_float64=fp64,
                 optimize_prj_affine=True, prj_affine_learning_rate=par['prj_affine_learning_rate'], forward_model=F27.MultiDistPlugin)
    if both:
        extra.update(optimize_free_prop=True, free_prop_learning_rate=par['free_prop_learning_rate'])
    try:
        G.run_driver(prj.astype(np.float64), (N, N, N), np.array([(0., 0.)]), np.pi, n_theta, extra, rec)
    finally:
        PT.update_parameters = orig_up
    return rec


def gen_driver(out):
    truth, pm, pp, prj = driver_data()
    out['drv/prj'] = prj
    out['drv/probe_mag'], out['drv/probe_phase'] = pm, pp
    guess = truth.astype(np.float32).astype(np.float64)      # the object starts at the truth (float32: exact in either precision)
    out['drv/guess_delta'], out['drv/guess_beta'] = guess[..., 0], guess[..., 1]
    out['drv/warp'] = WARP
    true = AR.inverse(WARP)
    out['drv/theta_true'] = true
    out['drv/dists_true_cm'] = np.array(DRV['dists_cm'])
    out['both/dists0_cm'] = F28.MODEL_DISTS_CM
    for tag, par, both in (('drv', DRV, False), ('both', DRV_BOTH, True)):
        dists0 = F28.MODEL_DISTS_CM if both else np.array(par['dists_cm'])
        recs = {fp64: run_reference(prj, guess, pm, pp, par, dists0, fp64, both) for fp64 in (True, False)}
        gs.run_fp64 = False
        tr = {k: np.stack(r['theta_trace']) for k, r in recs.items()}
        out[tag + '/fp64/losses'], out[tag + '/fp32/losses'] = recs[True]['losses'], recs[False]['losses']
        out[tag + '/fp64/theta'] = tr[True]                                    # [updates, D, 2, 3]
        out[tag + '/fp32/theta_err'] = np.abs(tr[False] - tr[True])            # the fp32 run's distance from it, per update and entry
        final = {k: np.stack([r['delta'], r['beta']], -1).astype(np.float64) for k, r in recs.items()}
        out[tag + '/fp64/obj'] = final[True]
        out[tag + '/fp32/obj_err'] = np.array(np.abs(final[False] - final[True]).max())
        if both:
            dtr = {k: np.stack(r['dist_trace']) for k, r in recs.items()}
            out[tag + '/fp64/dists'] = dtr[True]
            out[tag + '/fp32/dists_err'] = np.abs(dtr[False] - dtr[True])
            print(tag, 'final distances relative to the truth', dtr[True][-1] / np.array(par['dists_cm']))
        else:
            for i, tl in enumerate(recs[True]['task_lists']):
                for j, t in enumerate(tl):
                    out['drv/tasks_%d_%d' % (i, j)] = t
        fro = lambda a: np.sqrt((a ** 2).sum(axis=(-2, -1)))
        ratio = fro(tr[True][-1] - true) / np.where(fro(AR.IDENTITY - true) > 0, fro(AR.IDENTITY - true), 1)
        print(tag, 'losses', recs[True]['losses'][[0, -1]], 'fp32 theta err %.2e' % out[tag + '/fp32/theta_err'].max(),
              'Frobenius errors / starting errors', ratio)
        print(tr[True][-1], true)
        assert np.array_equal(tr[True][:, 0], np.tile(AR.IDENTITY, (len(tr[True]), 1, 1)))          # the pin
        if not both:
            assert np.all(ratio[1:] < 0.25), (tag, ratio)
        out[tag + '/params'] = np.array(repr(par))


if __name__ == '__main__':
    out = {}
    gen_kernel_cases(out)
    gen_driver(out)
    G.save('F29_multidist3d_affine', **out)
