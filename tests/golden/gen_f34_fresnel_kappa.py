"""Generates tests/golden/F34_fresnel_kappa.npz from the reference implementation (data only).

Usage: python tests/golden/gen_f34_fresnel_kappa.py        (needs the reference checkout that gen_goldens.py imports; CPU only)

The single-material constraint of Fresnel multi-distance holography: optimize_ctf_lg_kappa=True with forward_algorithm='fresnel'
makes MultiDistModel.predict hand kappa = 10 ** ctf_lg_kappa[0] to multislice_propagate_batch (adorym/forward_model.py:876-878,
1003-1010), where beta_slice = delta_slice * kappa (adorym/propagate.py:223-225).  (The CTF model of golden F26 DIVIDES by the same
number; nothing here reconciles the two.)

(a) kernel level: multislice_propagate_batch(..., free_prop_cm=d, kappa=10 ** lg_kappa[0]) once per distance on the one undivided
    field of view, + torch.autograd.grad w.r.t. the object and ctf_lg_kappa (a float64 tensor in either run, ptychography.py:733),
    in fp64 AND fp32.  '2d': a 16 x 32 field, S = 1, D = 3;  '3d': F27's 12 x 20 field, S = 5, D = 3.  Each with both sign
    conventions, magnitude and intensity data and lg_kappa in {-2, -0.5, 1.7} (12 cases).  The fp64 results whole, of the fp32 run
    only its distance from them (the yardstick of the 3x rule); 'gkappa_yardstick' is the largest of the fp32 run's relative
    distances of dL/dlg_kappa over the cases, asserted here to be at least 1e-6 (not a lucky draw).
(b) driver level: reconstruct_ptychography with the combination, fp64 and fp32, through a MultiDistModel plugin.  '2d': 32 x 32 x 1,
    D = 3, intensity data, 4 epochs;  '3d': 16^3, 4 angles, D = 3, magnitude data, 2 epochs;  Adam on the object and on
    ctf_lg_kappa.  Every loss, the final object, ctf_lg_kappa after every update; of the fp32 run every loss and its distances.
    Where the reference driver cannot run the combination, the exception text is the datum ('<tag>/ref_error').
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
import cases  # noqa: E402
import torch  # noqa: E402
import adorym  # noqa: E402
import adorym.global_settings as gs  # noqa: E402
from adorym.propagate import multislice_propagate_batch  # noqa: E402

ENERGY_EV, PSIZE_CM = 8000., 1e-6
DISTS_CM = (1e-4, 2e-4, 3.5e-4)
K1 = 2 * np.pi * PSIZE_CM * 1e7 / (1240. / ENERGY_EV)
GEOMETRIES = {'2d': ((16, 32), 1), '3d': ((12, 20), 5)}            # field, slices
LG_KAPPAS = (-2., -0.5, 1.7)
SEED = 3400


def kernel_case_table():
    """name: (geometry, sign_convention, raw_data_type, lg_kappa): every lg_kappa with both sign conventions and both data types."""
    table = {}
    for geo in sorted(GEOMETRIES):
        for i, lg in enumerate(LG_KAPPAS):
            pairs = ((1, 'magnitude'), (-1, 'intensity')) if i % 2 == 0 else ((1, 'intensity'), (-1, 'magnitude'))
            for sg, rdt in pairs:
                table['%s_%s_%s_k%d' % (geo, 'p1' if sg == 1 else 'm1', rdt, i)] = (geo, sg, rdt, lg)
    return table


KERNEL_CASES = kernel_case_table()


def kernel_inputs(name):
    geo, sg, rdt, lg = KERNEL_CASES[name]
    (Y, X), S = GEOMETRIES[geo]
    r = cases.rng(SEED + sorted(KERNEL_CASES).index(name))
    # the tied beta = kappa delta absorbs: the contrast is chosen so that the TRUTH (three times the guess) keeps k1 beta S <= 1.5
    amp = min(2e-3, 0.5 / (K1 * 10. ** lg * S))
    mk = lambda c: np.stack([amp * c * r.uniform(size=(Y, X, S)), 0.1 * amp * c * r.uniform(size=(Y, X, S))], -1)
    obj, truth = mk(1).astype(np.float32), mk(3).astype(np.float32)          # (exact in either precision; beta is there to be ignored)
    probe = ((0.5 + r.uniform(0, 1, (1, Y, X))) * np.exp(1j * r.uniform(-np.pi, np.pi, (1, Y, X)))).astype(np.complex64)
    return dict(obj=obj, truth=truth, probe=probe, lg_kappa=np.array([lg]))


def ref_forward(obj, lgk, pr, pi, sg):
    """One multislice_propagate_batch per distance on the whole field as the one tile; [D, Y, X]."""
    mags = []
    for d in DISTS_CM:
        er, ei = multislice_propagate_batch(obj[None], pr, pi, ENERGY_EV, PSIZE_CM, free_prop_cm=d, type='delta_beta', sign_convention=sg,
                                            kappa=10 ** lgk[0])
        mags.append(torch.sqrt(er ** 2 + ei ** 2))
    return torch.cat(mags, 0)


def ref_loss(pred, meas, rdt):
    """ForwardModel.get_mismatch_loss (adorym/forward_model.py:88-103), LSQ."""
    t = torch.abs(meas)
    return torch.mean((pred - (torch.sqrt(t) if rdt == 'intensity' else t)) ** 2)


def gen_kernel_cases(out):
    rel = lambda a, b: float(np.linalg.norm(np.asarray(a, np.float64) - b) / np.linalg.norm(b))
    yard = 0.
    for name in sorted(KERNEL_CASES):
        geo, sg, rdt, lg = KERNEL_CASES[name]
        inp = kernel_inputs(name)
        res = {}
        for fp64 in (True, False):
            gs.run_fp64 = fp64
            dt = torch.float64 if fp64 else torch.float32
            T = lambda a, g=False: torch.tensor(np.asarray(a, dtype=np.float64), dtype=dt, requires_grad=g)
            lgk = torch.tensor(inp['lg_kappa'], dtype=torch.float64, requires_grad=True)
            if fp64:
                with torch.no_grad():
                    meas = ref_forward(T(inp['truth']), lgk, T(inp['probe'].real), T(inp['probe'].imag), sg)
                    meas = meas ** 2 if rdt == 'intensity' else meas
            obj = T(inp['obj'], True)
            pred = ref_forward(obj, lgk, T(inp['probe'].real), T(inp['probe'].imag), sg)
            loss = ref_loss(pred, meas.to(dt), rdt)
            g = torch.autograd.grad(loss, [obj, lgk])
            res[fp64] = dict(pred=pred.detach().numpy(), loss=float(loss.detach()), grad=g[0].numpy(), gkappa=float(g[1][0]))
        r64, r32 = res[True], res[False]
        assert not r64['grad'][..., 1].any() and not r32['grad'][..., 1].any()          # beta is never read
        for k in ('obj', 'probe', 'lg_kappa'):
            out['%s/%s' % (name, k)] = inp[k]
        out[name + '/meas'] = meas.numpy()
        for k in ('pred', 'loss', 'grad', 'gkappa'):
            out['%s/%s' % (name, k)] = np.asarray(r64[k])
        # the reference's own fp32 run, as distances from its fp64 run: pred, loss, delta gradient, kappa gradient
        out[name + '/err32'] = np.array([rel(r32['pred'], r64['pred']), abs(r32['loss'] / r64['loss'] - 1),
                                         rel(r32['grad'][..., 0], r64['grad'][..., 0]), abs(r32['gkappa'] / r64['gkappa'] - 1)])
        yard = max(yard, out[name + '/err32'][3])
        print(name, 'loss %.6g gkappa %.6g; fp32 vs fp64: pred %.1e loss %.1e grad %.1e gkappa %.1e' % (
            (r64['loss'], r64['gkappa']) + tuple(out[name + '/err32'])))
    assert yard >= 1e-6, ('the pooled fp32 yardstick of dL/dlg_kappa is a lucky draw: change SEED', yard)
    out['gkappa_yardstick'] = np.array(yard)
    out['kernel_cases'] = np.array(sorted(KERNEL_CASES))
    out['kernel_case_params'] = np.array([repr(KERNEL_CASES[k]) for k in sorted(KERNEL_CASES)])
    out['kernel_dists_cm'] = np.array(DISTS_CM)
    print('pooled yardstick of dL/dlg_kappa: %.2e' % yard)


# ----------------------------------------------------------------------------------------------------------------- (b) the driver
DRV = {'2d': dict(N=32, S=1, n_theta=1, n_epochs=4, learning_rate=1e-5, ctf_lg_kappa_learning_rate=2e-3, lg_kappa=-0.5, lg_kappa_true=-0.3,
                  raw_data_type='intensity', dists_cm=DISTS_CM),
       '3d': dict(N=16, S=16, n_theta=4, n_epochs=2, learning_rate=1e-7, ctf_lg_kappa_learning_rate=2e-3, lg_kappa=-2., lg_kappa_true=-1.8,
                  raw_data_type='magnitude', dists_cm=DISTS_CM)}


def driver_inputs(tag):
    p = DRV[tag]
    N, S = p['N'], p['S']
    s0 = SEED + 50 + 10 * sorted(DRV).index(tag)
    truth = np.stack([4e-3 * (0.2 + cases.smooth_field((N, N, S), s0 + 1)), 4e-4 * (0.2 + cases.smooth_field((N, N, S), s0 + 2))], -1)
    guess = [3e-3 * (0.2 + cases.smooth_field((N, N, S), s0 + 3)), 3e-4 * (0.2 + cases.smooth_field((N, N, S), s0 + 4))]
    yy, xx = np.mgrid[:N, :N] - N / 2
    pm, pp = 0.6 + 0.4 * np.exp(-(yy ** 2 + xx ** 2) / (4. * N)), 0.1 * yy / N
    return truth, guess, pm, pp


class MultiDistPlugin(adorym.MultiDistModel):
    # (see gen_goldens.gen_f12: the 'auto' selection passes two keywords MultiDistModel.__init__ does not accept)
    def __init__(self, *a, run_bfloat16=False, run_float64=False, **k):
        super().__init__(*a, **k)


def gen_driver(out, tag):
    import adorym.ptychography as PT
    from oracle import adorym_oracle as O
    from tests import fresnel_kappa_ref as KR
    p = DRV[tag]
    N, S, n_theta, dists = p['N'], p['S'], p['n_theta'], list(p['dists_cm'])
    two_d = S == 1
    truth, guess, pm, pp = driver_inputs(tag)
    theta_ls = np.linspace(0, np.pi, n_theta, dtype='float32')
    phys = O.Physics((N, N), ENERGY_EV, PSIZE_CM, free_prop_cm=dists[0])
    probe = pm * np.exp(1j * pp)
    # the measurement: the restatement's fp64 forward of the truth under the true kappa (no reference data files exist)
    prj = np.zeros((n_theta, len(dists), N, N))
    for it, th in enumerate(theta_ls):
        coords = None if two_d else O.rotation_coords((N, N, S), th)
        mag = KR.forward_adjoint(truth, p['lg_kappa_true'], coords, probe[None], np.zeros((len(dists), N, N)), phys, dists)['pred']
        prj[it] = mag ** 2 if p['raw_data_type'] == 'intensity' else mag
    d = 'drv%s/' % tag
    out[d + 'prj'] = prj.astype(np.float32)
    out[d + 'probe_mag'], out[d + 'probe_phase'] = pm, pp
    out[d + 'guess_delta'], out[d + 'guess_beta'] = guess
    out[d + 'params'] = np.array(repr(p))
    prj = out[d + 'prj'].astype(np.float64)
    orig_up = PT.update_parameters
    final, traces = {}, {}
    try:
        for fp64 in (True, False):
            gs.run_fp64 = fp64
            rec = {'trace': []}

            def rec_up(opt_ls, optimizable_params, kw, _rec=rec):
                res = orig_up(opt_ls, optimizable_params, kw)
                if 'ctf_lg_kappa' in res:
                    _rec['trace'].append(float(res['ctf_lg_kappa'].detach().numpy()[0]))
                return res
            PT.update_parameters = rec_up
            extra = dict(minibatch_size=1, n_epochs=p['n_epochs'], optimizer='adam', learning_rate=p['learning_rate'], energy_ev=ENERGY_EV,
                         psize_cm=PSIZE_CM, free_prop_cm=np.array(dists), initial_guess=[guess[0], guess[1]], probe_type='supplied',
                         probe_initial=[pm, pp], two_d_mode=two_d, safe_zone_width=0, n_dp_batch=1, run_float64=fp64,
                         raw_data_type=p['raw_data_type'], unknown_type='delta_beta', forward_algorithm='fresnel', ctf_lg_kappa=p['lg_kappa'],
                         optimize_ctf_lg_kappa=True, ctf_lg_kappa_learning_rate=p['ctf_lg_kappa_learning_rate'], forward_model=MultiDistPlugin)
            with contextlib.redirect_stdout(io.StringIO()):
                G.run_driver(prj, (N, N, S), np.array([(0., 0.)]), 0 if two_d else np.pi, n_theta, extra, rec)
            t = d + ('fp64/' if fp64 else 'fp32/')
            out[t + 'losses'] = rec['losses']
            final[fp64] = np.stack([rec['delta'], rec['beta']], -1).astype(np.float64 if fp64 else np.float32).reshape(N, N, S, 2)
            traces[fp64] = np.array(rec['trace'])
            print(t, 'losses', rec['losses'], 'lg_kappa', rec['trace'])
    except Exception as e:      # noqa: BLE001  (what the reference does is the datum)
        out[d + 'ref_error'] = np.array('%s: %s' % (type(e).__name__, e))
        print(d, 'the reference driver does not run the combination:', out[d + 'ref_error'])
        return
    finally:
        PT.update_parameters = orig_up
        gs.run_fp64 = False
    x64, x32 = final[True], final[False].astype(np.float64)
    out[d + 'fp64/obj'] = x64
    out[d + 'fp64/lg_kappa_trace'] = traces[True]
    x0 = np.stack(guess, -1)
    out[d + 'fp32/obj_err'] = np.array(np.linalg.norm(x32 - x64) / np.linalg.norm(x64 - x0))      # (in units of the whole update)
    out[d + 'fp32/lg_kappa_err'] = np.abs(traces[False] - traces[True])
    n_off = int((np.abs(x64 - x32) > p['learning_rate']).sum())
    out[d + 'voxels_off'] = np.array([n_off, x64.size])
    print(d, 'fp32 vs fp64: object %.2e of the update, lg_kappa %.2e, voxels more than one step apart %d of %d' % (
        out[d + 'fp32/obj_err'], out[d + 'fp32/lg_kappa_err'].max(), n_off, x64.size))


if __name__ == '__main__':
    out = {}
    gen_kernel_cases(out)
    for tag in sorted(DRV):
        gen_driver(out, tag)
    gs.run_fp64 = False
    G.save('F34_fresnel_kappa', **out)
