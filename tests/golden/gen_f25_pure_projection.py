"""Generates tests/golden/F25_pure_projection.npz from the reference implementation (data only).

Usage: python tests/golden/gen_f25_pure_projection.py        (needs the reference checkout that gen_goldens.py imports; CPU only)

(a) kernel level: multislice_propagate_batch(..., pure_projection=True) (adorym/propagate.py:158-193) + torch.autograd.grad in fp64
    AND fp32.  Field 12 x 20, B = 5 positions over all four edges of the object, S = 7 and S = 1 slices; far field, a Fresnel
    detector with sign_convention = -1 and two probe modes, the exit wave, and the Poisson loss.  Prediction, loss and the
    gradients w.r.t. object and probe; the fp64 results whole, of the fp32 run only its distance from them (the yardstick of
    the 3x rule).
(b) driver level: reconstruct_ptychography(pure_projection=True), fp64 and fp32, 16^3 object, 3 x 3 positions of an 8 x 8 probe
    that hang over the object's edges, 4 angles, 2 epochs, Adam, minibatches of 3 ('immediate').  Task lists, every loss, the
    final object.
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
import adorym  # noqa: E402,F401
import adorym.global_settings as gs  # noqa: E402
from adorym.propagate import multislice_propagate_batch  # noqa: E402

ENERGY_EV, PSIZE_CM = 8000., 1e-6
PROBE = (12, 20)
B, MARGIN = 5, (5, 7)
FREE_PROP_CM = 2e-4
#       name: (free_prop_cm, sign_convention, n_modes, loss)
DETECTORS = {
    'far_field': ('inf', 1, 1, 'lsq'),
    'fresnel_m1_modes2': (FREE_PROP_CM, -1, 2, 'lsq'),
    'exit_wave': (None, 1, 1, 'lsq'),
    'far_field_poisson': ('inf', 1, 1, 'poisson'),
}
#              name: (S, free_prop_cm, sign_convention, n_modes, loss)
KERNEL_CASES = {'s%d_%s' % (S, k): (S,) + v for S in (7, 1) for k, v in DETECTORS.items()}


def edge_positions(r, n, Y, X, Py, Px):
    """tests/ms_matrix.py:edge_positions: positions hanging over all four edges of the object."""
    ylo, yhi, xlo, xhi = -3, Y - Py + 3, -3, X - Px + 3
    corners = [(ylo, xlo + 1), (ylo + 1, xhi), (yhi, xlo), (yhi - 1, xhi - 1)]
    return np.array(corners[:n] + [(int(r.integers(ylo, yhi + 1)), int(r.integers(xlo, xhi + 1))) for _ in range(n - 4)])


def kernel_inputs(name):
    S, free_prop, sg, M, loss = KERNEL_CASES[name]
    r = cases.rng(2500 + sorted(KERNEL_CASES).index(name))
    Py, Px = PROBE
    Y, X = Py + MARGIN[0], Px + MARGIN[1]
    # (the same projected thickness whatever S: 2e-3 * 7 / S per slice)
    mk = lambda c: np.stack([14e-3 / S * c * r.uniform(size=(Y, X, S)), 14e-4 / S * c * r.uniform(size=(Y, X, S))], -1)
    obj, truth = mk(1).astype(np.float32), mk(1.5).astype(np.float32)          # (exact in either precision)
    pos = edge_positions(r, B, Y, X, Py, Px)
    probes = ((0.5 + r.uniform(0, 1, (M, Py, Px))) * np.exp(1j * r.uniform(-np.pi, np.pi, (M, Py, Px)))).astype(np.complex64)
    return dict(obj=obj, truth=truth, pos=pos, probes=probes)


def ref_forward(obj, pos, pr, pi, free_prop, sg, probe_size=PROBE):
    """Pad with zeros (util.py:1327-1351), cut the tiles, propagate every mode through the projection model, sum the intensities."""
    Py, Px = probe_size
    Y, X = obj.shape[:2]
    py0, px0 = max(0, -int(pos[:, 0].min())), max(0, -int(pos[:, 1].min()))
    py1, px1 = max(0, int(pos[:, 0].max()) + Py - Y), max(0, int(pos[:, 1].max()) + Px - X)
    padded = torch.stack([torch.nn.functional.pad(obj[..., c], (0, 0, px0, px1, py0, py1), value=0.) for c in range(2)], -1)
    tiles = torch.stack([padded[y + py0:y + py0 + Py, x + px0:x + px0 + Px] for y, x in pos])
    inten = 0
    for m in range(pr.shape[0]):
        er, ei = multislice_propagate_batch(tiles, pr[m][None], pi[m][None], ENERGY_EV, PSIZE_CM, free_prop_cm=free_prop,
                                            type='delta_beta', sign_convention=sg, pure_projection=True)
        inten = inten + er ** 2 + ei ** 2
    return torch.sqrt(inten)


def ref_loss(pred, meas, loss):
    """ForwardModel.get_mismatch_loss (adorym/forward_model.py:88-103) for magnitude data, poisson_multiplier = 1."""
    if loss == 'lsq':
        return torch.mean((pred - meas) ** 2)
    return torch.mean(pred ** 2 - meas ** 2 * torch.log(pred ** 2))


def gen_kernel_cases(out):
    rel = lambda a, b: float(np.linalg.norm(np.asarray(a, np.complex128) - b) / np.linalg.norm(b))
    for name, (S, free_prop, sg, M, loss_type) in KERNEL_CASES.items():
        inp = kernel_inputs(name)
        res = {}
        for fp64 in (True, False):
            gs.run_fp64 = fp64
            dt = torch.float64 if fp64 else torch.float32
            T = lambda a, g=False: torch.tensor(np.asarray(a, dtype=np.float64), dtype=dt, requires_grad=g)
            if fp64:
                with torch.no_grad():
                    meas = ref_forward(T(inp['truth']), inp['pos'], T(inp['probes'].real), T(inp['probes'].imag), free_prop, sg)
            obj, pr, pi = T(inp['obj'], True), T(inp['probes'].real, True), T(inp['probes'].imag, True)
            pred = ref_forward(obj, inp['pos'], pr, pi, free_prop, sg)
            loss = ref_loss(pred, meas.to(dt), loss_type)
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
        # the model's signature: the gradient is the same for every slice
        assert np.array_equal(r64['grad'], np.broadcast_to(r64['grad'][:, :, :1], r64['grad'].shape))
    out['kernel_cases'] = np.array(sorted(KERNEL_CASES))
    out['kernel_case_params'] = np.array([repr(KERNEL_CASES[k]) for k in sorted(KERNEL_CASES)])


# ----------------------------------------------------------------------------------------------------------------- (b) the driver
DRV = dict(N=16, P=8, n_theta=4, grid=3, step=5, origin=-2, n_epochs=2, minibatch_size=3, learning_rate=1e-6, free_prop_cm='inf',
           energy_ev=cases.ENERGY_EV, psize_cm=cases.PSIZE_CM)


def driver_inputs():
    N, P = DRV['N'], DRV['P']
    truth = np.stack([1e-3 * (0.2 + cases.smooth_field((N, N, N), 2551)), 1e-4 * (0.2 + cases.smooth_field((N, N, N), 2552))], -1)
    guess = [8e-4 * (0.2 + cases.smooth_field((N, N, N), 2553)), 8e-5 * (0.2 + cases.smooth_field((N, N, N), 2554))]
    yy, xx = np.mgrid[:P, :P] - P / 2
    pm, pp = 0.6 + 0.4 * np.exp(-(yy ** 2 + xx ** 2) / 12.), 0.3 * yy / P
    g = DRV['origin'] + DRV['step'] * np.arange(DRV['grid'])
    pos = np.array([(y, x) for y in g for x in g], dtype=float)
    return truth, guess, pm, pp, pos


def gen_driver(out):
    from oracle import adorym_oracle as O
    from tests import projection_ref as PJ
    N, P, n_theta = DRV['N'], DRV['P'], DRV['n_theta']
    truth, guess, pm, pp, pos = driver_inputs()
    theta_ls = np.linspace(0, np.pi, n_theta, dtype='float32')
    phys = O.Physics((P, P), DRV['energy_ev'], DRV['psize_cm'], free_prop_cm=DRV['free_prop_cm'])
    probe = pm * np.exp(1j * pp)
    # the measurement: the restatement's fp64 forward of the truth (no reference data files exist)
    prj = np.zeros((n_theta, len(pos), P, P))
    for it, th in enumerate(theta_ls):
        rot = O.rotate_fwd(truth, O.rotation_coords((N, N, N), th), 'float64')
        tiles, _ = O.extract_tiles(rot, pos.astype(int), (P, P))
        prj[it] = PJ.predict(tiles, probe, phys)
    out['drv/prj'] = prj.astype(np.float32)
    out['drv/probe_mag'], out['drv/probe_phase'] = pm, pp
    out['drv/guess_delta'], out['drv/guess_beta'] = guess
    out['drv/pos'] = pos
    prj = out['drv/prj'].astype(np.float64)
    for fp64 in (True, False):
        gs.run_fp64 = fp64
        rec = {}
        extra = dict(minibatch_size=DRV['minibatch_size'], n_epochs=DRV['n_epochs'], optimizer='adam', learning_rate=DRV['learning_rate'],
                     energy_ev=DRV['energy_ev'], psize_cm=DRV['psize_cm'], free_prop_cm=DRV['free_prop_cm'],
                     initial_guess=[guess[0], guess[1]], probe_type='supplied', probe_initial=[pm, pp], pure_projection=True,
                     run_float64=fp64)
        G.run_driver(prj, (N, N, N), pos, np.pi, n_theta, extra, rec)
        tag = 'drv/%s/' % ('fp64' if fp64 else 'fp32')
        st = np.float64 if fp64 else np.float32
        out[tag + 'losses'] = rec['losses']
        out[tag + 'delta'], out[tag + 'beta'] = rec['delta'].astype(st), rec['beta'].astype(st)
        if fp64:
            out['drv/first_grad'] = rec['first_grad']
            for i, tl in enumerate(rec['task_lists']):
                for j, t in enumerate(tl):
                    out['drv/tasks_%d_%d' % (i, j)] = t
        print(tag, 'losses', rec['losses'])
    # Adam moves a voxel whose gradient is at rounding level by a full step of either sign: how many voxels of the reference's own
    # fp32 run end more than one step away from its fp64 run
    x64 = np.stack([out['drv/fp64/delta'], out['drv/fp64/beta']], -1)
    x32 = np.stack([out['drv/fp32/delta'], out['drv/fp32/beta']], -1).astype(np.float64)
    n_off = int((np.abs(x64 - x32) > DRV['learning_rate']).sum())
    out['drv/voxels_off'] = np.array([n_off, x64.size])
    print('voxels more than one step apart:', n_off, 'of', x64.size)
    out['drv/params'] = np.array(repr(DRV))


if __name__ == '__main__':
    out = {}
    gen_kernel_cases(out)
    gen_driver(out)
    G.save('F25_pure_projection', **out)
