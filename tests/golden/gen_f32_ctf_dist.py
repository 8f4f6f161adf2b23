"""Generates tests/golden/F32_ctf_dist.npz from the reference implementation (data only).

Usage: python tests/golden/gen_f32_ctf_dist.py        (needs the reference checkout that gen_goldens.py imports; CPU only)

The CTF model of multi-distance holography with the distances as parameters (optimize_free_prop: free_prop_cm goes differentiably
through modulate_and_get_ctf -> pure_phase_ctf, adorym/propagate.py:467-476, 590-606) and with the affine registration of the
measured holograms in front of the loss (optimize_prj_affine: w.affine_transform, adorym/forward_model.py:1066-1072).

(a) model level: F26's golden fields (tests/ctf_matrix.GOLDEN_FIELDS, inputs of ctf_matrix.inputs) through modulate_and_get_ctf, the
    LSQ mean and torch.autograd.grad with the distances as a tensor that requires grad, in fp64 AND fp32.  The data are made at the
    true distances, the model sits at truth * (1.10, 0.92, 1.05) rounded to float32 (both precisions see the same values).  The fp64
    results whole -- prediction, loss, gradients w.r.t. object, ctf_lg_kappa and free_prop_cm --, of the fp32 run only its
    distances from them.  The reference's own fp32 dL/dd must lie within 1e-2 of its fp64 value, element by element relative to the
    largest (asserted here: a looser yardstick lets anything pass).
    'reg/...': the same cases with the holograms through w.affine_transform with F29's matrices (gen_f29_multidist3d_affine.py
    KERNEL_THETA: matrix 0 the identity) as a tensor that requires grad; the registered target and dL/dtheta are stored too.
(b) driver level: reconstruct_ptychography(forward_algorithm='ctf') on F26's driver inputs (16 x 16 x 1 object, three distances,
    minibatch_size = 1, 4 epochs) started at the model distances with optimize_free_prop=True ('drv_dist'), on holograms 1 and 2
    warped by known matrices with optimize_prj_affine=True ('drv_aff'), and with both ('drv_both'), fp64 and fp32: every loss, the
    distances and matrices after every update, the final object.  Where the reference's driver raises on a combination the
    exception text is the datum ('<tag>/raised'), and the GPU driver is pinned to tests/ctf_dist_ref.py's loop instead.
"""
import contextlib
import io
import os
import sys
import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.join(HERE, '..', '..'))
import gen_goldens as G  # noqa: E402  (the I/O shims and the reference on sys.path)
import torch  # noqa: E402
import adorym  # noqa: E402,F401
import adorym.global_settings as gs  # noqa: E402
import adorym.wrappers as w  # noqa: E402
from adorym.propagate import modulate_and_get_ctf, gen_freq_mesh  # noqa: E402
from tests import ctf_matrix as CM  # noqa: E402
from tests import multidist3d_affine_ref as AR  # noqa: E402

OFF = np.array([1.10, 0.92, 1.05])
# gen_f29_multidist3d_affine.KERNEL_THETA
KERNEL_THETA = np.stack([AR.IDENTITY, AR.matrix(0.03, 1.04, (0.05, -0.03)), AR.matrix(-0.02, 0.97, (-0.04, 0.06))])
# the warps of the driver's holograms 1 and 2 (hologram 0 is the anchor)
WARP = np.stack([AR.IDENTITY, AR.matrix(0.02, 1.03, (0.06, -0.05)), AR.matrix(-0.02, 0.97, (-0.05, 0.06))])
DRV = dict(field=(16, 16, 3), n_epochs=4, learning_rate=1e-3, free_prop_learning_rate=0.5, prj_affine_learning_rate=5e-3)


def model_dists(d):
    return (np.asarray(d) * OFF[:len(d)]).astype(np.float32).astype(np.float64)


def ref_run(c, dists, fp64, theta=None):
    gs.run_fp64 = fp64
    dt = torch.float64 if fp64 else torch.float32
    ny, nx = c['ny'], c['nx']
    obj = torch.tensor(c['obj'].astype(np.float64)[None, :, :, None, :], dtype=dt, requires_grad=True)      # [1, ny, nx, 1, 2]
    lgk = torch.tensor([float(c['lg_kappa'])], dtype=torch.float64, requires_grad=True)
    fp = torch.tensor(np.asarray(dists, np.float64), dtype=dt, requires_grad=True)
    u, v = gen_freq_mesh(np.array([CM.PSIZE_CM * 1e7] * 3), [ny, nx])
    u, v = torch.tensor(u, dtype=dt), torch.tensor(v, dtype=dt)
    mags = []
    with contextlib.redirect_stdout(io.StringIO()):          # (pure_phase_ctf prints kappa)
        for this_dist in fp:                                 # (forward_model.py:999: 0-dim tensors)
            re, im = modulate_and_get_ctf(obj, CM.ENERGY_EV, this_dist, u, v, kappa=10 ** lgk[0])
            mags.append(torch.sqrt(re ** 2 + im ** 2))
    pred = torch.cat(mags, 0)
    meas = torch.abs(torch.tensor(c['data'].astype(np.float64), dtype=dt))
    wrt = [obj, lgk, fp]
    if theta is not None:
        th = torch.tensor(np.asarray(theta, np.float64), dtype=dt, requires_grad=True)
        meas = torch.cat([w.affine_transform(meas[d:d + 1], th[d], override_backend='pytorch') for d in range(len(dists))], 0)
        meas = torch.abs(meas)
        wrt.append(th)
    tgt = torch.sqrt(meas) if c['raw'] == 'intensity' else meas
    loss = torch.mean((pred - tgt) ** 2)
    g = torch.autograd.grad(loss, wrt)
    out = dict(pred=pred.detach().numpy(), loss=float(loss.detach()), grad=g[0].numpy()[0, :, :, 0, :], gkappa=float(g[1][0]),
               gdists=g[2].numpy().astype(np.float64))
    if theta is not None:
        out.update(target=tgt.detach().numpy(), gtheta=g[3].numpy().astype(np.float64))
    return out


def gen_model_cases(out):
    rel = lambda a, b: float(np.linalg.norm(np.asarray(a, np.float64) - b) / np.linalg.norm(b))
    names = []
    for (ny, nx, nd), raw in CM.GOLDEN_FIELDS.items():
        name = '%dx%dx%d_%s' % (ny, nx, nd, raw)
        names.append(name)
        c = CM.inputs(ny, nx, nd, raw=raw)
        md = model_dists(c['dists'])
        for tag, theta in ((name, None), ('reg/' + name, KERNEL_THETA[:nd])):
            r64, r32 = ref_run(c, md, True, theta), ref_run(c, md, False, theta)
            if theta is None:
                for k in ('obj', 'data', 'dists'):
                    out['%s/%s' % (tag, k)] = c[k]
                out[tag + '/model_dists'] = md
            keys = ('pred', 'loss', 'grad', 'gkappa', 'gdists') + (('target', 'gtheta') if theta is not None else ())
            for k in keys:
                out['%s/%s' % (tag, k)] = np.asarray(r64[k])
            assert (r64['pred'] ** 2).min() >= CM.MIN_I
            gd_err = np.abs(r32['gdists'] - r64['gdists']) / np.abs(r64['gdists']).max()
            # the reference's own fp32 run, as distances from its fp64 run: pred, loss, delta gradient, kappa gradient, then dL/dd per distance
            out[tag + '/err32'] = np.array([rel(r32['pred'], r64['pred']), abs(r32['loss'] / r64['loss'] - 1),
                                            rel(r32['grad'][..., 0], r64['grad'][..., 0]), abs(r32['gkappa'] / r64['gkappa'] - 1)] + list(gd_err))
            if theta is not None and nd > 1:
                out[tag + '/gtheta_err32'] = np.array([rel(r32['gtheta'][d], r64['gtheta'][d]) for d in range(1, nd)])
            print(tag, 'loss %.6g gdists' % r64['loss'], r64['gdists'], 'fp32 vs fp64: pred %.1e loss %.1e grad %.1e gkappa %.1e gdists'
                  % tuple(out[tag + '/err32'][:4]), gd_err)
            assert gd_err.max() < 1e-2, (tag, 'the fp32 reference is no yardstick for dL/dd here')
    out['model_cases'] = np.array(names)
    out['kernel_theta'] = KERNEL_THETA


def gen_driver(out):
    import adorym.ptychography as PT
    ny, nx, nd = DRV['field']
    c = CM.inputs(ny, nx, nd)
    md = model_dists(c['dists'])
    warped = AR.warp(c['data'].astype(np.float64), WARP).astype(np.float32)
    out['drv/obj'], out['drv/data'], out['drv/data_warped'] = c['obj'], c['data'], warped
    out['drv/dists_true'], out['drv/model_dists'], out['drv/warp'], out['drv/theta_true'] = c['dists'], md, WARP, AR.inverse(WARP)
    orig_up = PT.update_parameters

    class MultiDistPlugin(adorym.MultiDistModel):
        # (see gen_goldens.gen_f12: the 'auto' selection passes two keywords MultiDistModel.__init__ does not accept)
        def __init__(self, *a, run_bfloat16=False, run_float64=False, **k):
            super().__init__(*a, **k)

    def run(fp64, dist, aff):
        rec = {}

        def rec_up(opt_ls, optimizable_params, kw, _rec=rec):
            res = orig_up(opt_ls, optimizable_params, kw)
            for key, name in (('free_prop_cm', 'dists'), ('prj_affine_ls', 'theta')):
                if key in res:
                    x = res[key]
                    _rec.setdefault(name, []).append(np.asarray(x.detach().numpy() if hasattr(x, 'detach') else x, np.float64).copy())
            return res
        PT.update_parameters = rec_up
        prj = (warped if aff else c['data'])[None].astype(np.float64)
        try:
            with contextlib.redirect_stdout(io.StringIO()):
                G.run_driver(prj, [ny, nx, 1], np.array([[0., 0.]]), 0, 1,
                             dict(minibatch_size=1, n_epochs=DRV['n_epochs'], two_d_mode=True, energy_ev=CM.ENERGY_EV, psize_cm=CM.PSIZE_CM,
                                  free_prop_cm=np.array(md if dist else c['dists']),
                                  initial_guess=[c['obj'][:, :, None, 0].astype(np.float64), c['obj'][:, :, None, 1].astype(np.float64)],
                                  probe_type='plane', raw_data_type='intensity', unknown_type='delta_beta', gamma=0, alpha_d=0, alpha_b=0,
                                  optimizer='adam', learning_rate=DRV['learning_rate'], forward_algorithm='ctf', ctf_lg_kappa=CM.LG_KAPPA,
                                  optimize_ctf_lg_kappa=True, ctf_lg_kappa_learning_rate=0., n_dp_batch=1,
                                  optimize_free_prop=dist, free_prop_learning_rate=DRV['free_prop_learning_rate'],
                                  optimize_prj_affine=aff, prj_affine_learning_rate=DRV['prj_affine_learning_rate'],
                                  run_float64=fp64, randomize_probe_pos=True, safe_zone_width=0, forward_model=MultiDistPlugin), rec)
        finally:
            PT.update_parameters = orig_up
        return rec

    for tag, dist, aff in (('drv_dist', True, False), ('drv_aff', False, True), ('drv_both', True, True)):
        try:
            recs = {fp64: run(fp64, dist, aff) for fp64 in (True, False)}
        except Exception as e:      # noqa: BLE001  (what the reference does is the datum)
            out[tag + '/raised'] = np.array('%s: %s' % (type(e).__name__, e))
            print(tag, 'raised', out[tag + '/raised'])
            continue
        finally:
            gs.run_fp64 = False
        for fp64, r in recs.items():
            t = '%s/%s/' % (tag, 'fp64' if fp64 else 'fp32')
            out[t + 'losses'] = r['losses']
            out[t + 'delta'], out[t + 'beta'] = r['delta'], r['beta']
            for name in ('dists', 'theta'):
                if name in r:
                    out[t + name] = np.stack(r[name])
        print(tag, 'losses', recs[True]['losses'], {k: recs[True][k][-1] for k in ('dists', 'theta') if k in recs[True]})
    out['drv/params'] = np.array(repr(DRV))


if __name__ == '__main__':
    out = {}
    gen_model_cases(out)
    gen_driver(out)
    gs.run_fp64 = False
    G.save('F32_ctf_dist', **out)
