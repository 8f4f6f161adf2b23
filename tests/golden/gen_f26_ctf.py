"""Generates tests/golden/F26_ctf.npz from the reference implementation (data only).

Usage: python tests/golden/gen_f26_ctf.py        (needs the reference checkout that gen_goldens.py imports; CPU only)

(a) kernel level: modulate_and_get_ctf (adorym/propagate.py:467-476, 590-606) as MultiDistModel.predict calls it per distance
    (forward_model.py:999-1025: sqrt(re^2 + im^2) of what it returns), the LSQ mean of get_mismatch_loss and torch.autograd.grad
    w.r.t. the object and ctf_lg_kappa (a float64 tensor in either run, ptychography.py:733), in fp64 AND fp32.  Fields and inputs
    are tests/ctf_matrix.py's (GOLDEN_FIELDS; the object's beta channel is non-zero, the measurement is the model of a second
    object at lg_kappa 1.5, evaluated at 1.7).  Stored: the inputs, the fp64 prediction / loss / gradients whole, of the fp32 run
    only its distances from them (the yardstick of the 3x rule).
    Plus the clipped field (ctf_matrix.inputs(clip=True) at 16 x 16 x 2: a quarter of the pixels of a distance have I_d < 0):
    what the reference returns there -- the prediction (0 on those pixels) and how many entries of either gradient are NaN
    (all of them: sqrt(clip(I, 0)) puts inf * 0 into autograd's chain).
(b) driver level: reconstruct_ptychography(forward_algorithm='ctf', optimize_ctf_lg_kappa=True) through a MultiDistModel plugin,
    fp64 and fp32: 16 x 16 x 1 object, three distances, minibatch_size = 1, 4 epochs, Adam on the object and on ctf_lg_kappa.
    Every loss, the final delta and beta, ctf_lg_kappa after every update, the first gradient.
    With optimize_ctf_lg_kappa=False the reference driver does not run this model: 'ctf_lg_kappa' then never enters
    optimizable_params (ptychography.py:732-733), and the outcome of the attempt is recorded as text under 'drv/flag_off'.
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
from adorym.propagate import modulate_and_get_ctf, gen_freq_mesh  # noqa: E402
from tests import ctf_matrix as CM  # noqa: E402

CLIP_FIELD = (16, 16, 2)
DRV = dict(field=(16, 16, 3), n_epochs=4, learning_rate=1e-3, ctf_lg_kappa_learning_rate=2e-3)


def ref_run(c, fp64):
    gs.run_fp64 = fp64
    dt = torch.float64 if fp64 else torch.float32
    ny, nx = c['ny'], c['nx']
    obj = torch.tensor(c['obj'].astype(np.float64)[None, :, :, None, :], dtype=dt, requires_grad=True)      # [1, ny, nx, 1, 2]
    lgk = torch.tensor([float(c['lg_kappa'])], dtype=torch.float64, requires_grad=True)
    u, v = gen_freq_mesh(np.array([CM.PSIZE_CM * 1e7] * 3), [ny, nx])
    u, v = torch.tensor(u, dtype=dt), torch.tensor(v, dtype=dt)
    mags = []
    with contextlib.redirect_stdout(io.StringIO()):          # (pure_phase_ctf prints kappa)
        for d in c['dists']:
            re, im = modulate_and_get_ctf(obj, CM.ENERGY_EV, float(d), u, v, kappa=10 ** lgk[0])
            mags.append(torch.sqrt(re ** 2 + im ** 2))
    pred = torch.cat(mags, 0)
    meas = torch.abs(torch.tensor(c['data'].astype(np.float64), dtype=dt))
    loss = torch.mean((pred - (torch.sqrt(meas) if c['raw'] == 'intensity' else meas)) ** 2)
    g = torch.autograd.grad(loss, [obj, lgk])
    return dict(pred=pred.detach().numpy(), loss=float(loss.detach()), grad=g[0].numpy()[0, :, :, 0, :], gkappa=float(g[1][0]))


def gen_kernel_cases(out):
    rel = lambda a, b: float(np.linalg.norm(np.asarray(a, np.float64) - b) / np.linalg.norm(b))
    names = []
    for (ny, nx, nd), raw in CM.GOLDEN_FIELDS.items():
        name = '%dx%dx%d_%s' % (ny, nx, nd, raw)
        names.append(name)
        c = CM.inputs(ny, nx, nd, raw=raw)
        r64, r32 = ref_run(c, True), ref_run(c, False)
        for k in ('obj', 'data', 'dists'):
            out['%s/%s' % (name, k)] = c[k]
        for k in ('pred', 'loss', 'grad', 'gkappa'):
            out['%s/%s' % (name, k)] = np.asarray(r64[k])
        assert not r64['grad'][..., 1].any() and not r32['grad'][..., 1].any()          # beta is never read
        I = r64['pred'] ** 2
        assert I.min() >= CM.MIN_I
        # the reference's own fp32 run, as distances from its fp64 run: pred, loss, delta gradient, kappa gradient
        out[name + '/err32'] = np.array([rel(r32['pred'], r64['pred']), abs(r32['loss'] / r64['loss'] - 1),
                                         rel(r32['grad'][..., 0], r64['grad'][..., 0]), abs(r32['gkappa'] / r64['gkappa'] - 1)])
        print(name, 'loss %.6g gkappa %.6g min I %.3f; fp32 vs fp64: pred %.1e loss %.1e grad %.1e gkappa %.1e'
              % ((r64['loss'], r64['gkappa'], I.min()) + tuple(out[name + '/err32'])))
    out['kernel_cases'] = np.array(names)
    # the clipped field
    c = CM.inputs(*CLIP_FIELD, clip=True)
    for fp64 in (True, False):
        r = ref_run(c, fp64)
        tag = 'clip/%s/' % ('fp64' if fp64 else 'fp32')
        out[tag + 'pred'] = r['pred']
        out[tag + 'nan_counts'] = np.array([int(np.isnan(r['grad'][..., 0]).sum()), r['grad'][..., 0].size, int(np.isnan(r['gkappa']))])
        print(tag, 'pixels predicted 0: %d; NaN in the delta gradient: %d of %d; kappa gradient %r' % (
            int((r['pred'] == 0).sum()), out[tag + 'nan_counts'][0], out[tag + 'nan_counts'][1], r['gkappa']))
    for k in ('obj', 'data', 'dists'):
        out['clip/' + k] = c[k]


def gen_driver(out):
    import adorym.ptychography as PT
    ny, nx, nd = DRV['field']
    c = CM.inputs(ny, nx, nd)
    out['drv/obj'], out['drv/data'], out['drv/dists'] = c['obj'], c['data'], c['dists']
    prj = c['data'][None].astype(np.float64)                   # [1, n_dists, ny, nx]
    orig_up = PT.update_parameters

    class MultiDistPlugin(adorym.MultiDistModel):
        # (see gen_goldens.gen_f12: the 'auto' selection passes two keywords MultiDistModel.__init__ does not accept)
        def __init__(self, *a, run_bfloat16=False, run_float64=False, **k):
            super().__init__(*a, **k)

    def run(fp64, flag=True):
        rec = {'trace': []}

        def rec_up(opt_ls, optimizable_params, kw, _rec=rec):
            res = orig_up(opt_ls, optimizable_params, kw)
            if 'ctf_lg_kappa' in res:
                _rec['trace'].append(float(res['ctf_lg_kappa'].detach().numpy()[0]))
            return res
        PT.update_parameters = rec_up
        try:
            with contextlib.redirect_stdout(io.StringIO()):
                G.run_driver(prj, [ny, nx, 1], np.array([[0., 0.]]), 0, 1,
                             dict(minibatch_size=1, n_epochs=DRV['n_epochs'], two_d_mode=True, energy_ev=CM.ENERGY_EV, psize_cm=CM.PSIZE_CM,
                                  free_prop_cm=np.array(c['dists']), initial_guess=[c['obj'][:, :, None, 0].astype(np.float64),
                                                                                    c['obj'][:, :, None, 1].astype(np.float64)],
                                  probe_type='plane', raw_data_type='intensity', unknown_type='delta_beta', gamma=0, alpha_d=0, alpha_b=0,
                                  optimizer='adam', learning_rate=DRV['learning_rate'], forward_algorithm='ctf', ctf_lg_kappa=CM.LG_KAPPA,
                                  optimize_ctf_lg_kappa=flag, ctf_lg_kappa_learning_rate=DRV['ctf_lg_kappa_learning_rate'], n_dp_batch=1,
                                  run_float64=fp64, randomize_probe_pos=True, safe_zone_width=0, forward_model=MultiDistPlugin), rec)
        finally:
            PT.update_parameters = orig_up
        return rec

    for fp64 in (True, False):
        rec = run(fp64)
        tag = 'drv/%s/' % ('fp64' if fp64 else 'fp32')
        st = np.float64 if fp64 else np.float32
        out[tag + 'losses'] = rec['losses']
        out[tag + 'delta'], out[tag + 'beta'] = rec['delta'].astype(st), rec['beta'].astype(st)
        out[tag + 'lg_kappa_trace'] = np.array(rec['trace'])
        if fp64:
            out['drv/first_grad'] = rec['first_grad']
        print(tag, 'losses', rec['losses'], 'lg_kappa', rec['trace'])
    gs.run_fp64 = False
    try:
        rec = run(True, flag=False)
        out['drv/flag_off'] = np.array('ran: losses %r' % (list(rec['losses']),))
    except Exception as e:      # noqa: BLE001  (what the reference does is the datum)
        out['drv/flag_off'] = np.array('%s: %s' % (type(e).__name__, e))
    print('optimize_ctf_lg_kappa=False ->', out['drv/flag_off'])
    out['drv/params'] = np.array(repr(DRV))


if __name__ == '__main__':
    out = {}
    gen_kernel_cases(out)
    gen_driver(out)
    gs.run_fp64 = False
    G.save('F26_ctf', **out)
