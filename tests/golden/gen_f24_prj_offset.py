"""Generates tests/golden/F24_prj_offset.npz from the reference implementation (data only).

Usage: python tests/golden/gen_f24_prj_offset.py        (needs the reference checkout that gen_goldens.py imports; CPU only)

(a) kernel level: multislice_propagate_batch(..., shift_exit_wave=s) (adorym/propagate.py:131-288, util.py:380-397) +
    torch.autograd.grad in fp64 AND fp32.  The reference shifts a whole batch by ONE offset, so every position is propagated on
    its own with the offset of its entry and the results are stacked; two positions share an entry.  Field 12 x 20, B = 5 over all
    four edges of the object, offsets of mixed sign up to about 2 px.  Prediction, loss and the gradients w.r.t. object, probe and
    offsets; the fp64 results whole, of the fp32 run only its distance from them (the yardstick of the 3x rule).
(b) driver level: reconstruct_ptychography with optimize_prj_pos_offset=True, fp64 and fp32, 16^3 object, full field (one
    position), 4 angles, 2 epochs, Fresnel detector; the data are simulated with TRUE offsets of a few tenths of a pixel.  With
    the default optimiser of the offsets (GD, optimizers.py:863-875) and with a supplied AdamOptimizer.  Task lists, every loss,
    the offsets after every update, the final object.
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
from adorym.propagate import multislice_propagate_batch  # noqa: E402

ENERGY_EV, PSIZE_CM = 8000., 1e-6
PROBE = (12, 20)
B, MARGIN = 5, (5, 7)
FREE_PROP_CM = 2e-4
SHIFTS = np.array([[1.3, -0.7], [-2.1, 0.45], [0.25, 1.9], [-0.6, -1.15]])       # (s_y, s_x) per entry
INDEX = np.array([0, 1, 2, 1, 3])                                                  # positions 1 and 3 share entry 1
#        name: (S, unknown_type, free_prop_cm, sign_convention, n_modes)
KERNEL_CASES = {
    's3_fresnel_p1': (3, 'delta_beta', FREE_PROP_CM, 1, 1),
    's3_fresnel_m1_modes2': (3, 'delta_beta', FREE_PROP_CM, -1, 2),
    's1_fresnel': (1, 'delta_beta', FREE_PROP_CM, 1, 1),
    's3_exit_wave': (3, 'delta_beta', None, 1, 1),
    's3_far_field': (3, 'delta_beta', 'inf', 1, 1),
    's3_fresnel_real_imag': (3, 'real_imag', FREE_PROP_CM, 1, 1),
}


def edge_positions(r, n, Y, X, Py, Px):
    """tests/ms_matrix.py:edge_positions: positions hanging over all four edges of the object."""
    ylo, yhi, xlo, xhi = -3, Y - Py + 3, -3, X - Px + 3
    corners = [(ylo, xlo + 1), (ylo + 1, xhi), (yhi, xlo), (yhi - 1, xhi - 1)]
    return np.array(corners[:n] + [(int(r.integers(ylo, yhi + 1)), int(r.integers(xlo, xhi + 1))) for _ in range(n - 4)])


def kernel_inputs(name):
    S, unknown, free_prop, sg, M = KERNEL_CASES[name]
    r = cases.rng(2400 + sorted(KERNEL_CASES).index(name))
    Py, Px = PROBE
    Y, X = Py + MARGIN[0], Px + MARGIN[1]
    if unknown == 'delta_beta':
        mk = lambda c: np.stack([2e-3 * c * r.uniform(size=(Y, X, S)), 2e-4 * c * r.uniform(size=(Y, X, S))], -1)
    else:
        mk = lambda c: np.stack([1 + 1e-2 * c * r.standard_normal((Y, X, S)), 2e-2 * c * r.standard_normal((Y, X, S))], -1)
    obj, truth = mk(1).astype(np.float32), mk(10).astype(np.float32)          # (exact in either precision)
    pos = edge_positions(r, B, Y, X, Py, Px)
    probes = ((0.5 + r.uniform(0, 1, (M, Py, Px))) * np.exp(1j * r.uniform(-np.pi, np.pi, (M, Py, Px)))).astype(np.complex64)
    shifts = SHIFTS.astype(np.float32)
    shifts_true = (SHIFTS + r.uniform(-0.3, 0.3, SHIFTS.shape)).astype(np.float32)
    return dict(obj=obj, truth=truth, pos=pos, probes=probes, shifts=shifts, shifts_true=shifts_true, index=INDEX.astype(np.int32))


def ref_forward(obj, pos, pr, pi, shifts, index, unknown, free_prop, sg, probe_size=PROBE):
    """Pad (util.py:1327-1351: zeros, or 1 + 0i for real_imag), cut the tiles, propagate every position with the offset of its
    entry and every mode, sum the intensities."""
    Py, Px = probe_size
    Y, X = obj.shape[:2]
    py0, px0 = max(0, -int(pos[:, 0].min())), max(0, -int(pos[:, 1].min()))
    py1, px1 = max(0, int(pos[:, 0].max()) + Py - Y), max(0, int(pos[:, 1].max()) + Px - X)
    ch = []
    for c in range(2):
        fill = 1. if (unknown == 'real_imag' and c == 0) else 0.
        ch.append(torch.nn.functional.pad(obj[..., c], (0, 0, px0, px1, py0, py1), value=fill))
    padded = torch.stack(ch, -1)
    out = []
    for b, (y, x) in enumerate(pos):
        tile = padded[y + py0:y + py0 + Py, x + px0:x + px0 + Px][None]
        inten = 0
        for m in range(pr.shape[0]):
            er, ei = multislice_propagate_batch(tile, pr[m][None], pi[m][None], ENERGY_EV, PSIZE_CM, free_prop_cm=free_prop, type=unknown,
                                                sign_convention=sg, shift_exit_wave=shifts[int(index[b])])
            inten = inten + er ** 2 + ei ** 2
        out.append(torch.sqrt(inten)[0])
    return torch.stack(out)


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
                meas = ref_forward(T(inp['truth']), inp['pos'], T(inp['probes'].real), T(inp['probes'].imag), T(inp['shifts_true']),
                                   inp['index'], unknown, free_prop, sg) if fp64 else meas
            obj, pr, pi, sh = T(inp['obj'], True), T(inp['probes'].real, True), T(inp['probes'].imag, True), T(inp['shifts'], True)
            pred = ref_forward(obj, inp['pos'], pr, pi, sh, inp['index'], unknown, free_prop, sg)
            loss = torch.mean((pred - meas.to(dt)) ** 2)
            g = torch.autograd.grad(loss, [obj, pr, pi, sh])
            res[fp64] = dict(pred=pred.detach().numpy(), loss=float(loss), grad=g[0].numpy(), gprobe=g[1].numpy() + 1j * g[2].numpy(),
                             gs=g[3].numpy())
        r64, r32 = res[True], res[False]
        for k in ('obj', 'pos', 'probes', 'shifts', 'index'):
            out['%s/%s' % (name, k)] = inp[k]
        out[name + '/meas'] = meas.numpy()
        for k in ('pred', 'loss', 'grad', 'gprobe', 'gs'):
            out['%s/%s' % (name, k)] = np.asarray(r64[k])
        far = free_prop == 'inf'
        # the reference's own fp32 run, as distances from its fp64 run: pred, loss, grad, gprobe (whole), gs, gprobe per mode.  Far
        # field: the offsets do not reach the magnitudes, both gradients are rounding noise around zero and have no distance
        e_gs = 0. if far else rel(r32['gs'], r64['gs'])
        out[name + '/err32'] = np.array([rel(r32['pred'], r64['pred']), abs(r32['loss'] / r64['loss'] - 1), rel(r32['grad'], r64['grad']),
                                         rel(r32['gprobe'], r64['gprobe']), e_gs] + [rel(r32['gprobe'][m], r64['gprobe'][m]) for m in range(M)])
        print(name, 'fp32 vs fp64: pred %.1e loss %.1e grad %.1e gprobe %.1e gs %.1e' % tuple(out[name + '/err32'][:5]), 'gs', r64['gs'].ravel())
        if far:
            assert np.abs(r64['gs']).max() < 1e-12 * np.abs(r64['grad']).max(), 'a far-field magnitude must not depend on the offsets'
        else:
            # the condition on the inputs: the reference's own fp32 shift gradient is a usable yardstick
            assert e_gs < 1e-4, (name, e_gs)
    out['kernel_cases'] = np.array(sorted(KERNEL_CASES))
    out['kernel_case_params'] = np.array([repr(KERNEL_CASES[k]) for k in sorted(KERNEL_CASES)])


# ----------------------------------------------------------------------------------------------------------------- (b) the driver
DRV = dict(N=16, n_theta=4, free_prop_cm=FREE_PROP_CM, n_epochs=2, learning_rate=1e-7, prj_pos_offset_learning_rate=2e2, adam_step=2e-2,
           true_offsets=[[0.3, -0.2], [-0.25, 0.35], [0.15, 0.3], [-0.35, -0.1]])


def driver_inputs():
    N = DRV['N']
    truth = np.stack([4e-3 * (0.2 + cases.smooth_field((N, N, N), 2451)), 4e-4 * (0.2 + cases.smooth_field((N, N, N), 2452))], -1)
    guess = [3e-3 * (0.2 + cases.smooth_field((N, N, N), 2453)), 3e-4 * (0.2 + cases.smooth_field((N, N, N), 2454))]
    yy, xx = np.mgrid[:N, :N] - N / 2
    pm, pp = 0.6 + 0.4 * np.exp(-(yy ** 2 + xx ** 2) / 60.), 0.1 * yy / N
    return truth, guess, pm, pp


def gen_driver(out):
    import adorym.optimizers as OPT
    import adorym.ptychography as PT
    from oracle import adorym_oracle as O
    from tests import prj_offset_ref as PR
    N, n_theta = DRV['N'], DRV['n_theta']
    truth, guess, pm, pp = driver_inputs()
    theta_ls = np.linspace(0, np.pi, n_theta, dtype='float32')
    phys = O.Physics((N, N), ENERGY_EV, PSIZE_CM, free_prop_cm=DRV['free_prop_cm'])
    probe = pm * np.exp(1j * pp)
    pos = np.array([(0., 0.)])
    # the measurement: the restatement's fp64 forward with the TRUE offsets (no reference data files exist)
    prj = np.zeros((n_theta, 1, N, N))
    for it, th in enumerate(theta_ls):
        rot = O.rotate_fwd(truth, O.rotation_coords((N, N, N), th), 'float64')
        tiles, _ = O.extract_tiles(rot, pos.astype(int), (N, N))
        prj[it] = PR.predict(tiles, probe, phys, np.array(DRV['true_offsets'])[it:it + 1])
    trace = []
    orig = OPT.update_parameters

    def rec_update(opt_ls, optimizable_params, kwargs):
        res = orig(opt_ls, optimizable_params, kwargs)
        trace.append(optimizable_params['prj_pos_offset'].detach().numpy().copy())
        return res

    OPT.update_parameters = PT.update_parameters = rec_update
    out['drv/prj'] = prj.astype(np.float32)
    out['drv/probe_mag'], out['drv/probe_phase'] = pm, pp
    out['drv/guess_delta'], out['drv/guess_beta'] = guess
    prj = out['drv/prj'].astype(np.float64)
    try:
        for fp64 in (True, False):
            for run in ('gd', 'adam'):
                gs.run_fp64 = fp64
                rec = {}
                del trace[:]
                extra = dict(minibatch_size=1, n_epochs=DRV['n_epochs'], optimizer='adam', learning_rate=DRV['learning_rate'],
                             energy_ev=ENERGY_EV, psize_cm=PSIZE_CM, free_prop_cm=DRV['free_prop_cm'], initial_guess=[guess[0], guess[1]],
                             probe_type='supplied', probe_initial=[pm, pp], optimize_prj_pos_offset=True,
                             prj_pos_offset_learning_rate=DRV['prj_pos_offset_learning_rate'], run_float64=fp64)
                if run == 'adam':
                    extra['optimizer_prj_pos_offset'] = OPT.AdamOptimizer('prj_pos_offset', output_folder='out', options_dict={'step_size': DRV['adam_step']})
                G.run_driver(prj, (N, N, N), pos, np.pi, n_theta, extra, rec)
                tag = 'drv/%s_%s/' % (run, 'fp64' if fp64 else 'fp32')
                st = np.float64 if fp64 else np.float32
                out[tag + 'losses'] = rec['losses']
                out[tag + 'offset_trace'] = np.array(trace)
                out[tag + 'delta'], out[tag + 'beta'] = rec['delta'].astype(st), rec['beta'].astype(st)
                if fp64 and run == 'gd':
                    for i, tl in enumerate(rec['task_lists']):
                        for j, t in enumerate(tl):
                            out['drv/tasks_%d_%d' % (i, j)] = t
                print(tag, 'losses', rec['losses'], 'offsets', trace[-1].ravel())
    finally:
        OPT.update_parameters = PT.update_parameters = orig
    # Adam moves a voxel whose gradient is at rounding level by a full step of either sign: how many voxels of the reference's own
    # fp32 run end more than one step away from its fp64 run (the cap: 1e-3 of the voxels), and whether any offset does (none)
    for t in ('gd', 'adam'):
        x64 = np.stack([out['drv/%s_fp64/delta' % t], out['drv/%s_fp64/beta' % t]], -1)
        x32 = np.stack([out['drv/%s_fp32/delta' % t], out['drv/%s_fp32/beta' % t]], -1).astype(np.float64)
        n_off = int((np.abs(x64 - x32) > DRV['learning_rate']).sum())
        out['drv/%s_voxels_off' % t] = np.array([n_off, x64.size])
        print(t, 'voxels more than one step apart:', n_off, 'of', x64.size)
        assert n_off <= 1e-3 * x64.size
    o64, o32 = out['drv/adam_fp64/offset_trace'], out['drv/adam_fp32/offset_trace']
    assert int((np.abs(o64 - o32) > DRV['adam_step']).sum()) == 0
    out['drv/params'] = np.array(repr(DRV))


if __name__ == '__main__':
    out = {}
    gen_kernel_cases(out)
    gen_driver(out)
    G.save('F24_prj_offset', **out)
