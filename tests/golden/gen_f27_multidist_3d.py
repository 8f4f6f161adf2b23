"""Generates tests/golden/F27_multidist_3d.npz from the reference implementation (data only).

Usage: python tests/golden/gen_f27_multidist_3d.py        (needs the reference checkout that gen_goldens.py imports; CPU only)

(a) kernel level: multislice_propagate_batch(..., free_prop_cm=d) (adorym/propagate.py:131-288) once per distance on the same
    tiles, as MultiDistModel.predict does (adorym/forward_model.py:999-1019), + torch.autograd.grad in fp64 AND fp32.  Field
    12 x 20, S = 5 slices, D = 3 distances, B = 3 positions over the edges of the object; one and two probe modes,
    sign_convention +1 and -1, magnitude and intensity data.  Prediction (position-major: entry b * D + d), loss (the mean over all
    B * D entries) and the gradients w.r.t. object and probe; the fp64 results whole, of the fp32 run only its distance from them
    (the yardstick of the 3x rule).
(b) driver level: reconstruct_ptychography on multi-distance data of a 3-D object (two_d_mode=False, one undivided field of view),
    fp64 and fp32, 16^3 object, 4 angles, D = 3, 2 epochs, Adam, minibatch 1.  Every loss and the final object of the fp64
    run; of the fp32 run every loss and the final object's distance from the fp64 one, in units of the fp64 run's whole update.
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
B, S, MARGIN = 3, 5, (5, 7)
DISTS_CM = (1e-4, 2e-4, 3.5e-4)
#       name: (sign_convention, n_modes, raw_data_type)
KERNEL_CASES = {
    'm1_p1_magnitude': (1, 1, 'magnitude'),
    'm1_m1_intensity': (-1, 1, 'intensity'),
    'm2_p1_intensity': (1, 2, 'intensity'),
    'm2_m1_magnitude': (-1, 2, 'magnitude'),
}


def edge_positions(r, n, Y, X, Py, Px):
    """tests/ms_matrix.py:edge_positions: positions hanging over the edges of the object."""
    ylo, yhi, xlo, xhi = -3, Y - Py + 3, -3, X - Px + 3
    corners = [(ylo, xlo + 1), (ylo + 1, xhi), (yhi, xlo), (yhi - 1, xhi - 1)]
    return np.array(corners[:n] + [(int(r.integers(ylo, yhi + 1)), int(r.integers(xlo, xhi + 1))) for _ in range(n - 4)])


def kernel_inputs(name):
    sg, M, rdt = KERNEL_CASES[name]
    r = cases.rng(2700 + sorted(KERNEL_CASES).index(name))
    Py, Px = PROBE
    Y, X = Py + MARGIN[0], Px + MARGIN[1]
    mk = lambda c: np.stack([2e-3 * c * r.uniform(size=(Y, X, S)), 2e-4 * c * r.uniform(size=(Y, X, S))], -1)
    obj, truth = mk(1).astype(np.float32), mk(10).astype(np.float32)          # (exact in either precision)
    pos = edge_positions(r, B, Y, X, Py, Px)
    probes = ((0.5 + r.uniform(0, 1, (M, Py, Px))) * np.exp(1j * r.uniform(-np.pi, np.pi, (M, Py, Px)))).astype(np.complex64)
    return dict(obj=obj, truth=truth, pos=pos, probes=probes)


def ref_forward(obj, pos, pr, pi, sg, probe_size=PROBE):
    """Pad with zeros (util.py:1327-1351), cut the tiles, then one multislice_propagate_batch per distance and mode on the same tiles;
    the intensities of the modes are summed.  Returns [B * D, Py, Px], position-major."""
    Py, Px = probe_size
    Y, X = obj.shape[:2]
    py0, px0 = max(0, -int(pos[:, 0].min())), max(0, -int(pos[:, 1].min()))
    py1, px1 = max(0, int(pos[:, 0].max()) + Py - Y), max(0, int(pos[:, 1].max()) + Px - X)
    padded = torch.stack([torch.nn.functional.pad(obj[..., c], (0, 0, px0, px1, py0, py1), value=0.) for c in range(2)], -1)
    tiles = torch.stack([padded[y + py0:y + py0 + Py, x + px0:x + px0 + Px] for y, x in pos])
    mags = []
    for d in DISTS_CM:
        inten = 0
        for m in range(pr.shape[0]):
            er, ei = multislice_propagate_batch(tiles, pr[m][None], pi[m][None], ENERGY_EV, PSIZE_CM, free_prop_cm=d, type='delta_beta',
                                                sign_convention=sg)
            inten = inten + er ** 2 + ei ** 2
        mags.append(torch.sqrt(inten))
    return torch.stack(mags, 1).reshape(len(pos) * len(DISTS_CM), Py, Px)


def ref_loss(pred, meas, rdt):
    """ForwardModel.get_mismatch_loss (adorym/forward_model.py:88-103), LSQ."""
    t = torch.abs(meas)
    return torch.mean((pred - (torch.sqrt(t) if rdt == 'intensity' else t)) ** 2)


def gen_kernel_cases(out):
    rel = lambda a, b: float(np.linalg.norm(np.asarray(a, np.complex128) - b) / np.linalg.norm(b))
    for name, (sg, M, rdt) in KERNEL_CASES.items():
        inp = kernel_inputs(name)
        res = {}
        for fp64 in (True, False):
            gs.run_fp64 = fp64
            dt = torch.float64 if fp64 else torch.float32
            T = lambda a, g=False: torch.tensor(np.asarray(a, dtype=np.float64), dtype=dt, requires_grad=g)
            if fp64:
                with torch.no_grad():
                    meas = ref_forward(T(inp['truth']), inp['pos'], T(inp['probes'].real), T(inp['probes'].imag), sg)
                    meas = meas ** 2 if rdt == 'intensity' else meas
            obj, pr, pi = T(inp['obj'], True), T(inp['probes'].real, True), T(inp['probes'].imag, True)
            pred = ref_forward(obj, inp['pos'], pr, pi, sg)
            loss = ref_loss(pred, meas.to(dt), rdt)
            g = torch.autograd.grad(loss, [obj, pr, pi])
            res[fp64] = dict(pred=pred.detach().numpy(), loss=float(loss.detach()), grad=g[0].numpy(), gprobe=g[1].numpy() + 1j * g[2].numpy())
        r64, r32 = res[True], res[False]
        for k in ('obj', 'pos', 'probes'):
            out['%s/%s' % (name, k)] = inp[k]
        out[name + '/meas'] = meas.numpy()
        for k in ('pred', 'loss', 'grad', 'gprobe'):
            out['%s/%s' % (name, k)] = np.asarray(r64[k])
        # the reference's own fp32 run, as distances from its fp64 run: pred, loss, grad, gprobe (whole), gprobe per mode
        out[name + '/err32'] = np.array([rel(r32['pred'], r64['pred']), abs(r32['loss'] / r64['loss'] - 1), rel(r32['grad'], r64['grad']),
                                         rel(r32['gprobe'], r64['gprobe'])] + [rel(r32['gprobe'][m], r64['gprobe'][m]) for m in range(M)])
        print(name, 'loss %.6g; fp32 vs fp64: pred %.1e loss %.1e grad %.1e gprobe %.1e' % ((r64['loss'],) + tuple(out[name + '/err32'][:4])))
    out['kernel_cases'] = np.array(sorted(KERNEL_CASES))
    out['kernel_case_params'] = np.array([repr(KERNEL_CASES[k]) for k in sorted(KERNEL_CASES)])
    out['kernel_dists_cm'] = np.array(DISTS_CM)


# ----------------------------------------------------------------------------------------------------------------- (b) the driver
DRV = dict(N=16, n_theta=4, dists_cm=DISTS_CM, n_epochs=2, learning_rate=1e-7, energy_ev=ENERGY_EV, psize_cm=PSIZE_CM)


def driver_inputs():
    N = DRV['N']
    truth = np.stack([4e-3 * (0.2 + cases.smooth_field((N, N, N), 2751)), 4e-4 * (0.2 + cases.smooth_field((N, N, N), 2752))], -1)
    guess = [3e-3 * (0.2 + cases.smooth_field((N, N, N), 2753)), 3e-4 * (0.2 + cases.smooth_field((N, N, N), 2754))]
    yy, xx = np.mgrid[:N, :N] - N / 2
    pm, pp = 0.6 + 0.4 * np.exp(-(yy ** 2 + xx ** 2) / 60.), 0.1 * yy / N
    return truth, guess, pm, pp


class MultiDistPlugin(adorym.MultiDistModel):
    # the reference's 'auto' selection passes run_bfloat16 / run_float64 to MultiDistModel.__init__, which does not accept them
    # (TypeError at ptychography.py:535); a forward_model= plugin that drops the two keywords is the way to run it (as for F12)
    def __init__(self, *a, run_bfloat16=False, run_float64=False, **k):
        super().__init__(*a, **k)


def gen_driver(out):
    from oracle import adorym_oracle as O
    from tests import multidist3d_ref as MR
    N, n_theta, dists = DRV['N'], DRV['n_theta'], list(DRV['dists_cm'])
    truth, guess, pm, pp = driver_inputs()
    theta_ls = np.linspace(0, np.pi, n_theta, dtype='float32')
    phys = O.Physics((N, N), ENERGY_EV, PSIZE_CM, free_prop_cm=dists[0])
    probe = pm * np.exp(1j * pp)
    pos = np.array([(0., 0.)])
    # the measurement: the restatement's fp64 forward of the truth (no reference data files exist)
    prj = np.zeros((n_theta, len(dists), N, N))
    for it, th in enumerate(theta_ls):
        rot = O.rotate_fwd(truth, O.rotation_coords((N, N, N), th), 'float64')
        tiles, _ = O.extract_tiles(rot, pos.astype(int), (N, N))
        prj[it] = MR.predict(tiles, probe, phys, dists)
    out['drv/prj'] = prj.astype(np.float32)
    out['drv/probe_mag'], out['drv/probe_phase'] = pm, pp
    out['drv/guess_delta'], out['drv/guess_beta'] = guess
    prj = out['drv/prj'].astype(np.float64)
    final = {}
    for fp64 in (True, False):
        gs.run_fp64 = fp64
        rec = {}
        extra = dict(minibatch_size=1, n_epochs=DRV['n_epochs'], optimizer='adam', learning_rate=DRV['learning_rate'], energy_ev=ENERGY_EV,
                     psize_cm=PSIZE_CM, free_prop_cm=np.array(dists), initial_guess=[guess[0], guess[1]], probe_type='supplied',
                     probe_initial=[pm, pp], two_d_mode=False, safe_zone_width=0, n_dp_batch=1, run_float64=fp64,
                     forward_model=MultiDistPlugin)
        G.run_driver(prj, (N, N, N), pos, np.pi, n_theta, extra, rec)
        tag = 'drv/%s/' % ('fp64' if fp64 else 'fp32')
        st = np.float64 if fp64 else np.float32
        out[tag + 'losses'] = rec['losses']
        final[fp64] = np.stack([rec['delta'], rec['beta']], -1).astype(st)
        if fp64:
            for i, tl in enumerate(rec['task_lists']):
                for j, t in enumerate(tl):
                    out['drv/tasks_%d_%d' % (i, j)] = t
        print(tag, 'losses', rec['losses'])
    gs.run_fp64 = False
    # Adam moves a voxel whose gradient is at rounding level by a full step of either sign: how many voxels of the reference's own
    # fp32 run end more than one step away from its fp64 run
    # (the final object of the fp64 run whole; of the fp32 run its distance from it)
    x64, x32 = final[True], final[False].astype(np.float64)
    out['drv/fp64/obj'] = x64
    x0 = np.stack(guess, -1)
    out['drv/fp32/obj_err'] = np.array(np.linalg.norm(x32 - x64) / np.linalg.norm(x64 - x0))      # (in units of the whole update)
    n_off = int((np.abs(x64 - x32) > DRV['learning_rate']).sum())
    out['drv/voxels_off'] = np.array([n_off, x64.size])
    print('voxels more than one step apart:', n_off, 'of', x64.size)
    out['drv/params'] = np.array(repr(DRV))


if __name__ == '__main__':
    out = {}
    gen_kernel_cases(out)
    gen_driver(out)
    G.save('F27_multidist_3d', **out)
