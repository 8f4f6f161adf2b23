"""Generates tests/golden/F21_sparse_multislice.npz from the reference implementation (data only).

Usage: python tests/golden/gen_f21_sparse.py        (needs the reference checkout that gen_goldens.py imports; CPU only)

(a) kernel level: sparse_multislice_propagate_batch (adorym/propagate.py:479-534) + torch.autograd.grad in fp64 AND fp32 for
    S in {2, 3, 5} with unequal gaps, both unknown types, detector none / far field / Fresnel, sign convention +1 / -1, 1 and 2
    probe modes (summed as forward_model.py:760-779): prediction, loss, and the gradients w.r.t. object, probe and slice
    positions.  The fp64 results are stored whole; of the fp32 run only its distance from them (the yardstick of the 3x rule).
(b) driver level: reconstruct_ptychography with SparseMultisliceModel through a plugin subclass that drops the two keywords the
    'auto' selection passes and the model does not take (the defect gen_goldens.py documents for MultiDistModel), fp64 and
    fp32, optimize_slice_pos off and on (+ optimize_probe); the data are simulated with TRUE slice positions a few per cent
    away from the initial ones.  Task lists, every loss, z after every update, final object and probe.
"""
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
from adorym.propagate import sparse_multislice_propagate_batch, gen_freq_mesh  # noqa: E402

ENERGY_EV, PSIZE_CM = 8000., 1e-6
PROBE = (16, 20)
B, MARGIN = 5, (5, 7)
Z_CM = {2: [0., 10e-4], 3: [0., 10e-4, 35e-4], 5: [0., 4e-4, 10e-4, 25e-4, 31e-4]}
#        name: (S, unknown_type, free_prop_cm, sign_convention, n_modes)
KERNEL_CASES = {
    's2_db_far_p1_m1': (2, 'delta_beta', 'inf', 1, 1),
    's2_ri_none_m1_m2': (2, 'real_imag', None, -1, 2),
    's3_db_fresnel_m1_m2': (3, 'delta_beta', 2e-3, -1, 2),
    's3_ri_far_m1_m1': (3, 'real_imag', 'inf', -1, 1),
    's3_db_none_p1_m1': (3, 'delta_beta', None, 1, 1),
    's3_ri_far_p1_m2': (3, 'real_imag', 'inf', 1, 2),
    's5_ri_fresnel_p1_m1': (5, 'real_imag', 2e-3, 1, 1),
    's5_db_far_m1_m2': (5, 'delta_beta', 'inf', -1, 2),
}


def edge_positions(r, n, Y, X, Py, Px):
    """tests/ms_matrix.py:edge_positions: positions hanging over all four edges of the object."""
    ylo, yhi, xlo, xhi = -3, Y - Py + 3, -3, X - Px + 3
    corners = [(ylo, xlo + 1), (ylo + 1, xhi), (yhi, xlo), (yhi - 1, xhi - 1)]
    return np.array(corners[:n] + [(int(r.integers(ylo, yhi + 1)), int(r.integers(xlo, xhi + 1))) for _ in range(n - 4)])


def kernel_inputs(name):
    S, unknown, free_prop, sg, M = KERNEL_CASES[name]
    r = cases.rng(2100 + sorted(KERNEL_CASES).index(name))
    Py, Px = PROBE
    Y, X = Py + MARGIN[0], Px + MARGIN[1]
    if unknown == 'delta_beta':
        mk = lambda c: np.stack([2e-3 * c * r.uniform(size=(Y, X, S)), 2e-4 * c * r.uniform(size=(Y, X, S))], -1)
    else:
        mk = lambda c: np.stack([1 + 1e-2 * c * r.standard_normal((Y, X, S)), 2e-2 * c * r.standard_normal((Y, X, S))], -1)
    obj, truth = mk(1).astype(np.float32), mk(10).astype(np.float32)          # (exact in either precision)
    pos = edge_positions(r, B, Y, X, Py, Px)
    probes = ((0.5 + r.uniform(0, 1, (M, Py, Px))) * np.exp(1j * r.uniform(-np.pi, np.pi, (M, Py, Px)))).astype(np.complex64)
    z = np.array(Z_CM[S], dtype=np.float32)
    z_true = (z * np.float32(1.03)).astype(np.float32)
    return dict(obj=obj, truth=truth, pos=pos, probes=probes, z=z, z_true=z_true)


def ref_forward(obj, pos, pr, pi, z, unknown, free_prop, sg, dt):
    """Pad (util.py:1327-1351: zeros, or 1 + 0i for real_imag), cut the tiles, propagate every mode, sum the intensities."""
    Py, Px = PROBE
    Y, X = obj.shape[:2]
    py0, px0 = max(0, -int(pos[:, 0].min())), max(0, -int(pos[:, 1].min()))
    py1, px1 = max(0, int(pos[:, 0].max()) + Py - Y), max(0, int(pos[:, 1].max()) + Px - X)
    ch = []
    for c in range(2):
        fill = 1. if (unknown == 'real_imag' and c == 0) else 0.
        ch.append(torch.nn.functional.pad(obj[..., c], (0, 0, px0, px1, py0, py1), value=fill))
    padded = torch.stack(ch, -1)
    tiles = torch.stack([padded[y + py0:y + py0 + Py, x + px0:x + px0 + Px] for y, x in pos])
    u, v = gen_freq_mesh(np.array([PSIZE_CM * 1e7] * 3), (Py, Px))
    ut, vt = torch.tensor(u, dtype=dt), torch.tensor(v, dtype=dt)
    inten = 0
    for m in range(pr.shape[0]):
        er, ei = sparse_multislice_propagate_batch(ut, vt, tiles, pr[m], pi[m], ENERGY_EV, PSIZE_CM, z, free_prop_cm=free_prop,
                                                   type=unknown, sign_convention=sg)
        inten = inten + er ** 2 + ei ** 2
    return torch.sqrt(inten)


def gen_kernel_cases(out):
    rel = lambda a, b: float(np.linalg.norm(np.asarray(a, np.complex128) - b) / np.linalg.norm(b))
    for name, (S, unknown, free_prop, sg, M) in KERNEL_CASES.items():
        inp = kernel_inputs(name)
        res = {}
        for fp64 in (True, False):
            gs.run_fp64 = fp64
            dt = torch.float64 if fp64 else torch.float32
            T = lambda a, g=False: torch.tensor(np.asarray(a, dtype=np.float64), dtype=dt, requires_grad=g)
            with torch.no_grad():
                meas = ref_forward(T(inp['truth']), inp['pos'], T(inp['probes'].real), T(inp['probes'].imag), T(inp['z_true']),
                                   unknown, free_prop, sg, dt) if fp64 else meas
            obj, pr, pi, z = T(inp['obj'], True), T(inp['probes'].real, True), T(inp['probes'].imag, True), T(inp['z'], True)
            pred = ref_forward(obj, inp['pos'], pr, pi, z, unknown, free_prop, sg, dt)
            loss = torch.mean((pred - meas.to(dt)) ** 2)
            g = torch.autograd.grad(loss, [obj, pr, pi, z])
            res[fp64] = dict(pred=pred.detach().numpy(), loss=float(loss), grad=g[0].numpy(), gprobe=g[1].numpy() + 1j * g[2].numpy(),
                             gz=g[3].numpy())
        r64, r32 = res[True], res[False]
        for k in ('obj', 'pos', 'probes', 'z'):
            out['%s/%s' % (name, k)] = inp[k]
        out[name + '/meas'] = meas.numpy()
        for k in ('pred', 'loss', 'grad', 'gprobe', 'gz'):
            out['%s/%s' % (name, k)] = np.asarray(r64[k])
        # the reference's own fp32 run, as distances from its fp64 run: pred, loss, grad, gprobe per mode (and whole), gz
        out[name + '/err32'] = np.array([rel(r32['pred'], r64['pred']), abs(r32['loss'] / r64['loss'] - 1), rel(r32['grad'], r64['grad']),
                                         rel(r32['gprobe'], r64['gprobe']), rel(r32['gz'], r64['gz'])]
                                        + [rel(r32['gprobe'][m], r64['gprobe'][m]) for m in range(M)])
        print(name, 'fp32 vs fp64: pred %.1e loss %.1e grad %.1e gprobe %.1e gz %.1e' % tuple(out[name + '/err32'][:5]), 'gz', r64['gz'])
    out['kernel_cases'] = np.array(sorted(KERNEL_CASES))
    out['kernel_case_params'] = np.array([repr(KERNEL_CASES[k]) for k in sorted(KERNEL_CASES)])


# ----------------------------------------------------------------------------------------------------------------- (b) the driver
DRV = dict(N=36, P=16, S=3, z0=[0., 2e-3, 5e-3], z_true=[0., 2.08e-3, 4.85e-3], n_epochs=2, minibatch_size=8, learning_rate=1e-3,
           probe_learning_rate=1e-3, slice_pos_learning_rate=1e-5)


def driver_inputs():
    N, P, S = DRV['N'], DRV['P'], DRV['S']
    pos = np.array([(y, x) for y in (0, 6, 13, 20) for x in (0, 7, 13, 20)], dtype=float)
    mag = 1 - 0.15 * cases.smooth_field((N, N, S), 2151)
    ph = 0.4 * cases.smooth_field((N, N, S), 2152)
    truth = np.stack([mag * np.cos(ph), mag * np.sin(ph)], -1)
    yy, xx = np.mgrid[:P, :P] - P / 2
    pm, pp = np.exp(-(yy ** 2 + xx ** 2) / 30.), 0.1 * yy / P
    # the guess has structure of its own: through a uniform object the far-field magnitudes do not depend on z at all, dL/dz would
    # be rounding noise and Adam would turn its sign into a full step
    g_mag = (1 - 0.06 * cases.smooth_field((N, N, S), 2153)).astype(np.float32)
    g_ph = (0.15 * cases.smooth_field((N, N, S), 2154)).astype(np.float32)
    return pos, truth, pm, pp, g_mag, g_ph


def gen_driver(out):
    import adorym.optimizers as OPT
    import adorym.ptychography as PT
    N, P, S = DRV['N'], DRV['P'], DRV['S']
    pos, truth, pm, pp, g_mag, g_ph = driver_inputs()
    gs.run_fp64 = True
    T = lambda a: torch.tensor(np.asarray(a, dtype=np.float64))
    global PROBE
    keep = PROBE
    PROBE = (P, P)
    with torch.no_grad():
        prj = ref_forward(T(truth), pos.astype(int), T((pm * np.cos(pp))[None]), T((pm * np.sin(pp))[None]), T(DRV['z_true']), 'real_imag',
                          'inf', 1, torch.float64).numpy()[None]
    PROBE = keep
    # NB: ref_forward above used this file's ENERGY_EV / PSIZE_CM; the driver runs with the same two numbers
    trace = []
    orig = OPT.update_parameters

    def rec_update(opt_ls, optimizable_params, kwargs):
        res = orig(opt_ls, optimizable_params, kwargs)
        if 'slice_pos_cm_ls' in optimizable_params:
            trace.append(optimizable_params['slice_pos_cm_ls'].detach().numpy().copy())
        return res

    class SparsePlugin(adorym.SparseMultisliceModel):
        # the reference's 'auto' selection passes run_bfloat16 / run_float64 to SparseMultisliceModel.__init__, which does not
        # take them (TypeError): the plugin route with a subclass that drops them, as for MultiDistModel in gen_goldens.py
        def __init__(self, *a, run_bfloat16=False, run_float64=False, **k):
            super().__init__(*a, **k)

    OPT.update_parameters = PT.update_parameters = rec_update
    out['drv/prj'] = prj.astype(np.float32)
    out['drv/pos'], out['drv/probe_mag'], out['drv/probe_phase'] = pos, pm, pp
    out['drv/guess_mag'], out['drv/guess_phase'] = g_mag, g_ph
    prj = out['drv/prj'].astype(np.float64)
    try:
        for fp64 in (True, False):
            for opt_sp in (False, True):
                gs.run_fp64 = fp64
                rec = {}
                del trace[:]
                G.run_driver(prj, (N, N, S), pos, 0, 1,
                             dict(two_d_mode=True, minibatch_size=DRV['minibatch_size'], n_epochs=DRV['n_epochs'], optimizer='adam',
                                  learning_rate=DRV['learning_rate'], unknown_type='real_imag', energy_ev=ENERGY_EV, psize_cm=PSIZE_CM,
                                  initial_guess=[g_mag.astype(np.float64), g_ph.astype(np.float64)], probe_type='supplied', probe_initial=[pm, pp],
                                  slice_pos_cm_ls=np.array(DRV['z0']), forward_model=SparsePlugin, optimize_slice_pos=opt_sp,
                                  slice_pos_learning_rate=DRV['slice_pos_learning_rate'], optimize_probe=True,
                                  probe_learning_rate=DRV['probe_learning_rate'], run_float64=fp64,
                                  random_guess_means_sigmas=(1., 0., 0.001, 0.002)), rec, ri=True)
                tag = 'drv/%s_%s/' % ('zopt' if opt_sp else 'zfix', 'fp64' if fp64 else 'fp32')
                pk = {k.split('/')[-1]: v for k, v in G.TIFFS.items() if 'probe' in k}
                out[tag + 'losses'] = rec['losses']
                out[tag + 'z_trace'] = np.array(trace)
                st = np.float64 if fp64 else np.float32
                out[tag + 'mag'], out[tag + 'phase'] = rec['mag'].astype(st), rec['phase'].astype(st)
                for k, v in pk.items():
                    out[tag + k] = np.asarray(v).astype(st)
                if fp64 and not opt_sp:
                    for i, tl in enumerate(rec['task_lists']):
                        for j, t in enumerate(tl):
                            out['drv/tasks_%d_%d' % (i, j)] = t
                print(tag, 'losses', rec['losses'], 'z', trace[-1] if trace else None, 'probe files', sorted(pk))
    finally:
        OPT.update_parameters = PT.update_parameters = orig
    # Adam moves a voxel whose gradient is at rounding level by a full step of either sign: how many voxels of the reference's own
    # fp32 run end more than one step away from its fp64 run, and whether any slice position does (the caps: 1e-3 of the voxels, none)
    for t in ('zfix', 'zopt'):
        x64 = out['drv/%s_fp64/mag' % t] * np.exp(1j * out['drv/%s_fp64/phase' % t])
        x32 = out['drv/%s_fp32/mag' % t].astype(np.float64) * np.exp(1j * out['drv/%s_fp32/phase' % t].astype(np.float64))
        n_off = int((np.abs(x64 - x32) > DRV['learning_rate']).sum())
        out['drv/%s_voxels_off' % t] = np.array([n_off, x64.size])
        print(t, 'voxels more than one step apart:', n_off, 'of', x64.size)
        assert n_off <= 1e-3 * x64.size
    z64, z32 = out['drv/zopt_fp64/z_trace'], out['drv/zopt_fp32/z_trace']
    n_z_off = int((np.abs(z64 - z32) > DRV['slice_pos_learning_rate']).sum())
    out['drv/z_off'] = np.array([n_z_off])
    assert n_z_off == 0
    out['drv/params'] = np.array(repr(DRV))


if __name__ == '__main__':
    out = {}
    gen_kernel_cases(out)
    gen_driver(out)
    G.save('F21_sparse_multislice', **out)
