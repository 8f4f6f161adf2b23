"""Generates tests/golden/F30_ctf_tomo.npz from the reference implementation (data only).

Usage: python tests/golden/gen_f30_ctf_tomo.py        (needs the reference checkout that gen_goldens.py imports; CPU only)

(b) driver level: the reference's own reconstruct_ptychography(forward_algorithm='ctf', two_d_mode=False,
    optimize_ctf_lg_kappa=True) through a MultiDistModel plugin, fp64 and fp32: 16^3 object, 4 angles over [0, pi], 3 distances,
    minibatch_size = 1, two epochs, Adam on the object and on ctf_lg_kappa (inputs: tests/ctf_tomo_ref.driver_inputs; the
    measurement is the fp64 model of a second object at lg_kappa 1.5).  Every loss, the final delta and beta, ctf_lg_kappa after
    every update, the first gradient, the angle of every minibatch -- and whether the reference's own fp32 run stays inside the
    cap of check_run (tests/test_gpu_ctf_driver.py), checked and printed here: the GPU test applies the cap only if it does.

(a) model level: what MultiDistModel.predict does to a 3-D object under forward_algorithm='ctf' (adorym/forward_model.py:905-914,
999-1025): apply_rotation with the reference's own lookup table (save_rotation_lookup / read_origin_coords), modulate_and_get_ctf
per distance (adorym/propagate.py:467-476: the rotated object summed along the beam, then pure_phase_ctf), sqrt(re^2 + im^2), the
LSQ mean of get_mismatch_loss and torch.autograd.grad w.r.t. the object and ctf_lg_kappa (a float64 tensor in either run), in fp64
AND fp32.  Cases and inputs are tests/ctf_tomo_ref.py's.  Stored: the inputs, the fp64 prediction / loss / gradients whole, of the
fp32 run only its distances from them (the yardstick of the 3x rule).  The reference returns NaN gradients once a pixel clips, so
every case is asserted to keep min I_d >= ctf_matrix.MIN_I.
"""
import contextlib
import io
import os
import sys
import tempfile
import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.join(HERE, '..', '..'))
import gen_goldens as G  # noqa: E402  (the I/O shims and the reference on sys.path)
import torch  # noqa: E402
import adorym  # noqa: E402,F401
import adorym.global_settings as gs  # noqa: E402
import adorym.util as U  # noqa: E402
from adorym.propagate import modulate_and_get_ctf, gen_freq_mesh  # noqa: E402
from tests import ctf_matrix as CM  # noqa: E402
from tests import ctf_tomo_ref as TR  # noqa: E402


def ref_table(size, theta, tag):
    gs.run_fp64 = False
    U.save_rotation_lookup(list(size), np.array([theta], dtype='float32'), dest_folder='rot_' + tag)
    return U.read_origin_coords('rot_' + tag, theta)


def ref_run(c, coords, fp64):
    gs.run_fp64 = fp64
    dt = torch.float64 if fp64 else torch.float32
    Y, X, Z = c['size']
    obj = torch.tensor(c['obj'].astype(np.float64), dtype=dt, requires_grad=True)                            # [Y, X, Z, 2]
    lgk = torch.tensor([float(c['lg_kappa'])], dtype=torch.float64, requires_grad=True)
    u, v = gen_freq_mesh(np.array([CM.PSIZE_CM * 1e7] * 3), [Y, X])
    u, v = torch.tensor(u, dtype=dt), torch.tensor(v, dtype=dt)
    rot = U.apply_rotation(obj, coords, device=None)
    mags = []
    with contextlib.redirect_stdout(io.StringIO()):          # (pure_phase_ctf prints kappa)
        for d in c['dists']:
            re, im = modulate_and_get_ctf(rot[None], CM.ENERGY_EV, float(d), u, v, kappa=10 ** lgk[0])
            mags.append(torch.sqrt(re ** 2 + im ** 2))
    pred = torch.cat(mags, 0)
    meas = torch.abs(torch.tensor(c['data'].astype(np.float64), dtype=dt))
    loss = torch.mean((pred - torch.sqrt(meas)) ** 2)
    g = torch.autograd.grad(loss, [obj, lgk])
    return dict(pred=pred.detach().numpy(), loss=float(loss.detach()), grad=g[0].numpy(), gkappa=float(g[1][0]))


def gen_model_cases(out):
    rel = lambda a, b: float(np.linalg.norm(np.asarray(a, np.float64) - b) / np.linalg.norm(b))
    cwd = os.getcwd()
    with tempfile.TemporaryDirectory() as td:
        os.chdir(td)
        try:
            for i, name in enumerate(TR.CASES):
                c = TR.inputs(name)
                coords = ref_table(c['size'], c['theta'], str(i))
                r64, r32 = ref_run(c, coords, True), ref_run(c, coords, False)
                for k in ('obj', 'data', 'dists'):
                    out['%s/%s' % (name, k)] = c[k]
                for k in ('pred', 'loss', 'grad', 'gkappa'):
                    out['%s/%s' % (name, k)] = np.asarray(r64[k])
                assert r64['pred'].shape == (c['nd'],) + tuple(c['size'][:2])
                assert not r64['grad'][..., 1].any() and not r32['grad'][..., 1].any()          # beta is never read
                I = r64['pred'] ** 2
                assert I.min() >= CM.MIN_I, (name, I.min())
                out[name + '/err32'] = np.array([rel(r32['pred'], r64['pred']), abs(r32['loss'] / r64['loss'] - 1),
                                                 rel(r32['grad'][..., 0], r64['grad'][..., 0]), abs(r32['gkappa'] / r64['gkappa'] - 1)])
                print(name, 'loss %.6g gkappa %.6g min I %.3f; fp32 vs fp64: pred %.1e loss %.1e grad %.1e gkappa %.1e'
                      % ((r64['loss'], r64['gkappa'], I.min()) + tuple(out[name + '/err32'])))
        finally:
            os.chdir(cwd)
    out['model_cases'] = np.array(list(TR.CASES))


# ----------------------------------------------------------------------------------------------------------------- (b) the driver
DRV = dict(N=16, n_theta=4, n_dists=3, n_epochs=2, learning_rate=2e-5, ctf_lg_kappa_learning_rate=2e-3)


class MultiDistPlugin(adorym.MultiDistModel):
    # the reference's 'auto' selection passes run_bfloat16 / run_float64 to MultiDistModel.__init__, which does not accept them;
    # a forward_model= plugin that drops the two keywords is the way to run it (as for F12, F26, F27)
    def __init__(self, *a, run_bfloat16=False, run_float64=False, **k):
        super().__init__(*a, **k)


def gen_driver(out):
    import adorym.ptychography as PT
    from oracle import adorym_oracle as O
    N, n_theta, nd = DRV['N'], DRV['n_theta'], DRV['n_dists']
    c = TR.driver_inputs(N, n_theta, nd)
    theta_ls = np.linspace(0, np.pi, n_theta, dtype='float32')
    # the measurement: the restatement's fp64 model of the truth at lg_kappa 1.5, per angle (intensities)
    prj = np.zeros((n_theta, nd, N, N))
    for it, th in enumerate(theta_ls):
        p = TR.project(c['truth'], O.rotation_coords((N, N, N), th))
        prj[it] = TR.R.forward_adjoint(p[..., 0], c['dists'], CM.LG_KAPPA_TRUTH, np.ones((nd, N, N)), CM.ENERGY_EV, CM.PSIZE_CM, want_grad=False)['I']
        assert prj[it].min() >= CM.MIN_I
    out['drv/prj'] = prj.astype(np.float32)
    out['drv/obj'], out['drv/dists'] = c['obj'], c['dists']
    prj = out['drv/prj'].astype(np.float64)
    orig_up = PT.update_parameters
    final = {}
    for fp64 in (True, False):
        rec = {'trace': []}

        def rec_up(opt_ls, optimizable_params, kw, _rec=rec):
            res = orig_up(opt_ls, optimizable_params, kw)
            if 'ctf_lg_kappa' in res:
                _rec['trace'].append(float(res['ctf_lg_kappa'].detach().numpy()[0]))
            return res
        PT.update_parameters = rec_up
        try:
            with contextlib.redirect_stdout(io.StringIO()):
                G.run_driver(prj, (N, N, N), np.array([[0., 0.]]), np.pi, n_theta,
                             dict(minibatch_size=1, n_epochs=DRV['n_epochs'], two_d_mode=False, energy_ev=CM.ENERGY_EV, psize_cm=CM.PSIZE_CM,
                                  free_prop_cm=np.array(c['dists']), initial_guess=[c['obj'][..., 0].astype(np.float64), c['obj'][..., 1].astype(np.float64)],
                                  probe_type='plane', raw_data_type='intensity', unknown_type='delta_beta', optimizer='adam',
                                  learning_rate=DRV['learning_rate'], forward_algorithm='ctf', ctf_lg_kappa=CM.LG_KAPPA, optimize_ctf_lg_kappa=True,
                                  ctf_lg_kappa_learning_rate=DRV['ctf_lg_kappa_learning_rate'], n_dp_batch=1, run_float64=fp64,
                                  safe_zone_width=0, forward_model=MultiDistPlugin), rec)
        finally:
            PT.update_parameters = orig_up
        tag = 'drv/%s/' % ('fp64' if fp64 else 'fp32')
        st = np.float64 if fp64 else np.float32
        out[tag + 'losses'] = rec['losses']
        out[tag + 'delta'], out[tag + 'beta'] = rec['delta'].astype(st), rec['beta'].astype(st)
        out[tag + 'lg_kappa_trace'] = np.array(rec['trace'])
        final[fp64] = np.stack([rec['delta'], rec['beta']], -1).astype(np.float64)
        if fp64:
            out['drv/first_grad'] = rec['first_grad']
            out['drv/batches'] = np.array([b[0] for b in rec['batches']])
            assert not rec['first_grad'][..., 1].any()
        print(tag, 'losses', rec['losses'], 'lg_kappa', rec['trace'])
    gs.run_fp64 = False
    # the cap of check_run (tests/test_gpu_ctf_driver.py) on the reference's OWN fp32 run: RMSE < 1e-5, under 1e-3 of the voxels more
    # than half a step from the fp64 run, losses within 1e-5.  The GPU test applies the cap only where this holds.
    d = np.abs(final[False] - final[True])
    rmse, flipped = float(np.sqrt(np.mean(d ** 2))), float((d > 0.5 * DRV['learning_rate']).mean())
    eloss = float(np.abs(out['drv/fp32/losses'] / out['drv/fp64/losses'] - 1).max())
    ok = rmse < 1e-5 and flipped < 1e-3 and eloss < 1e-5
    out['drv/fp32_within_cap'] = np.array([rmse, flipped, eloss, float(ok)])
    print("the reference's fp32 run against check_run's cap: RMSE %.2e, flipped %.2e, losses %.2e -> %s" % (rmse, flipped, eloss, 'within' if ok else 'OUTSIDE'))
    moved = float(np.abs(final[True][..., 0] - c['obj'][..., 0]).max())
    print('delta moved by at most %.2e (%.1f steps)' % (moved, moved / DRV['learning_rate']))
    out['drv/params'] = np.array(repr(DRV))


if __name__ == '__main__':
    out = {}
    gen_model_cases(out)
    gen_driver(out)
    gs.run_fp64 = False
    G.save('F30_ctf_tomo', **out)
