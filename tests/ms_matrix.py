"""One minibatch of the multislice engine against the fp64 oracle, for any point of the kernel matrix (test infrastructure only:
the oracle is the checker, never the product).

``run_case`` builds the inputs and runs the oracle in fp64 and fp32 (``oracle_case``) and the engine (``run_engine``: rotate ->
multislice -> rotate_adjoint, optionally through sub-pixel probe shifts or one probe set per position).  The oracle runs
position by position: every position has its own detector distance (b % n), its own probe set and its own shift, and the batch
loss / gradients are the means of the positions' (all positions have the same number of detector pixels).  ``check`` applies a set of bars to the result.

The tables below name every compiled variant of adm_multislice.hip; tests/test_kernel_matrix_coverage.py parses the kernel
source and fails when a size or a dispatch branch is added there without being added here.
"""
import numpy as np

from oracle import adorym_oracle as O

ENERGY_EV, PSIZE_CM = 5000., 1e-7

# ADM_FOR_EACH_SIZE of adm_multislice.hip: the tuned kernels and the probe-shift kernels exist at these sizes
SIZES = (8, 12, 16, 18, 24, 27, 32, 36, 64, 72)
SHIFT_SIZES = SIZES

# the dispatch branches of launch<> in adm_multislice.hip, keyed like its ADM_LAUNCH(BIN1, MULTI, MODE, PP) calls, and the
# run_case arguments that reach each of them through the engine
BRANCHES = {
    (True, False, 2, False): dict(),                                                   # cached transmissions (the default)
    (True, True, 2, False): dict(n_modes=3),
    (True, False, 0, False): dict(transmission_cache=False),                          # (delta, beta), exp / sincos in the kernel
    (True, True, 0, False): dict(transmission_cache=False, n_modes=3),
    (False, False, 0, False): dict(binning=2, S=5),                                    # the last step bins one slice
    (False, True, 0, False): dict(binning=3, S=7, n_modes=3),                          # the last step bins one slice
    (True, False, 1, False): dict(unknown_type='real_imag'),
    (True, True, 1, False): dict(unknown_type='real_imag', n_modes=3),
    (True, False, 2, True): dict(pp='shifts'),                                         # per-position probes
    (True, True, 2, True): dict(pp='shifts', n_modes=3),
    (True, False, 0, True): dict(pp='shifts', transmission_cache=False),
    (True, True, 0, True): dict(pp='shifts', transmission_cache=False, n_modes=3),
    (True, False, 1, True): dict(pp='shifts', unknown_type='real_imag'),
    (True, True, 1, True): dict(pp='shifts', unknown_type='real_imag', n_modes=3),
}

# detector and loss variants, each run at every size
VARIANTS = {
    'far_sign_m1': dict(sign_convention=-1),
    'far_sign_m1_modes': dict(sign_convention=-1, n_modes=3),
    'far_ortho_modes': dict(normalize_fft=True, n_modes=3),
    'far_ortho_sign_m1': dict(normalize_fft=True, sign_convention=-1, transmission_cache=False),
    'near_field': dict(free_prop=0),
    'fresnel_modes': dict(free_prop=1e-4, n_modes=3),
    'exact_slice_kernel': dict(fresnel_approx=False),
    'poisson_magnitude': dict(loss='poisson', raw_data_type='magnitude', poisson_multiplier=50.),
    'poisson_intensity_modes': dict(loss='poisson', raw_data_type='intensity', poisson_multiplier=50., n_modes=3),
    'beamstop': dict(beamstop=True),
    'beamstop_modes_near': dict(beamstop=True, n_modes=3, free_prop=0),
    'three_distances_pp': dict(free_prop=[1e-4, 2e-4, 3.5e-4], pp='probes', B=12),
}

# fields of the any-size kernel (adm_ms_generic.hip) at its edges: one large-prime pass (127, 113), the loop over the primes
# left after the listed radices (11 * 11), extreme aspect ratios, the largest accepted field (Py*Px <= 16384)
GENERIC_FIELDS = [(127, 127), (113, 120), (121, 121), (8, 2048), (2048, 8), (127, 129)]
GENERIC_REFUSED = [(129, 128), (128, 129), (16, 1040)]

BRANCH_CASES = [(P, br) for P in SIZES for br in BRANCHES]
VARIANT_CASES = [(P, v) for P in SIZES for v in VARIANTS]

# bars: the tuned-size tests' (test_every_compiled_probe_size_vs_oracle, F23) and the generic kernel's
TUNED = dict(pred=2e-6, loss=2e-5, grad=1e-4, grad_abs=1e-5, probe_3x=True, shift=2e-4)
GENERIC = dict(pred=5e-6, loss=3e-5, grad=2e-4, grad_abs=2e-5, probe_3x=False, shift=2e-4)


def dispatch(kw):
    """The ADM_LAUNCH(BIN1, MULTI, MODE, PP) branch that launch<> takes for the run_case arguments ``kw`` (mirrors launch<>
    and the engine's choice of the transmission cache)."""
    binning = kw.get('binning', 1)
    real_imag = kw.get('unknown_type', 'delta_beta') == 'real_imag'
    pre_t = kw.get('transmission_cache', True) and not real_imag and binning == 1
    mode = 1 if real_imag else 2 if pre_t else 0
    return (binning == 1, kw.get('n_modes', 1) > 1, mode, kw.get('pp') is not None)


def rel(a, b):
    a, b = np.asarray(a, np.complex128), np.asarray(b, np.complex128)
    return np.linalg.norm(a - b) / np.linalg.norm(b)


def c2(z):
    return np.ascontiguousarray(np.stack([z.real, z.imag], -1), dtype=np.float32)


def cplx(a):
    return a[..., 0].astype(np.float64) + 1j * a[..., 1].astype(np.float64)


def edge_positions(r, B, Y, X, Py, Px):
    """B positions (top-left corners) hanging over all four edges of a Y x X object, the rest anywhere around it."""
    ylo, yhi, xlo, xhi = -3, Y - Py + 3, -3, X - Px + 3
    corners = [(ylo, xlo + 1), (ylo + 1, xhi), (yhi, xlo), (yhi - 1, xhi - 1)]
    pos = corners[:B] + [(int(r.integers(ylo, yhi + 1)), int(r.integers(xlo, xhi + 1))) for _ in range(B - 4)]
    return np.array(pos)


def run_case(A, ctx, P, **kw):
    """oracle_case + run_engine."""
    return run_engine(A, ctx, oracle_case(P, **kw))


def oracle_case(P, S=5, B=11, n_modes=1, unknown_type='delta_beta', binning=1, transmission_cache=True, free_prop='inf',
                sign_convention=1, normalize_fft=False, fresnel_approx=True, loss='lsq', raw_data_type='magnitude', poisson_multiplier=1.,
                beamstop=False, pp=None, generic=False, margin=(9, 13), seed=0, obj_fn=None, meas_edit=None, shifts_fn=None, probe_edit=None,
                index_fn=None):
    """The inputs of one minibatch and the oracle's results on them.  ``P``: size or (Py, Px); ``free_prop``: 'inf', 0, a distance
    in cm or a list of distances (position b uses distance b % n); ``pp``: None (one shared probe set), 'shifts' (Fourier-shifted per
    position, gradients w.r.t. the probe and the shifts) or 'probes' (a probe set per position handed over as it is).
    ``beamstop``: True (a disc and the first row dropped) or a [Py, Px] mask of its own.  A case may supply its own numbers
    (tests/value_matrix.py): ``obj_fn(r, Y, X, S) -> (obj, truth)`` in place of the weak object drawn here, ``meas_edit(meas,
    beamstop) -> meas`` applied to the measured data, ``shifts_fn(n_entries) -> [n_entries, 2]`` in place of the shifts within
    2.5 px, ``probe_edit(probes) -> probes`` applied to the shared probe set, ``index_fn(B) -> (n_entries, index [B] or None)`` in
    place of the max(2, B - 4) shift entries of which some are used twice (tests/count_matrix.py; an index of None: B entries,
    position b uses entry b and the engine gets no index).  The defaults draw what they always drew, bit for bit.
    Returns a dict of the inputs and the oracle results (``*_o`` fp64, ``*_32`` fp32; ``loss_b_*``: every position's own loss, which
    times ``n_det`` is the engine's loss sum of that position); run_engine adds the engine's (``*``)."""
    Py, Px = (P, P) if np.isscalar(P) else tuple(P)
    r = np.random.default_rng([Py, Px, S, B, n_modes, binning, seed])
    Y, X = Py + margin[0], Px + margin[1]
    # the truth (which makes the data) has ten times the guess's contrast: the residual pred - target is then ~10 % of pred, not
    # ~1 %, and the fp32 rounding of pred does not dominate the gradients (the 3x rule compares kernels, not rounding luck)
    if unknown_type == 'delta_beta':
        mk = lambda c: np.stack([2e-3 * c * r.uniform(size=(Y, X, S)), 2e-4 * c * r.uniform(size=(Y, X, S))], -1)
    else:
        mk = lambda c: np.stack([1 + 1e-2 * c * r.standard_normal((Y, X, S)), 2e-2 * c * r.standard_normal((Y, X, S))], -1)
    obj, truth = (mk(1), mk(10)) if obj_fn is None else obj_fn(r, Y, X, S)
    pos = edge_positions(r, B, Y, X, Py, Px)
    M = n_modes
    rand_probes = lambda *lead: (0.5 + r.uniform(0, 1, lead + (Py, Px))) * np.exp(1j * r.uniform(-np.pi, np.pi, lead + (Py, Px)))
    probes = rand_probes(M)
    if probe_edit is not None:
        probes = probe_edit(probes)
    dists = list(free_prop) if isinstance(free_prop, (list, tuple)) else [free_prop]
    phys = [O.Physics((Py, Px), ENERGY_EV, PSIZE_CM, free_prop_cm=d, binning=binning, fresnel_approx=fresnel_approx,
                      sign_convention=sign_convention, normalize_fft=normalize_fft, unknown_type=unknown_type) for d in dists]
    bs = None
    if isinstance(beamstop, np.ndarray):
        bs = beamstop
    elif beamstop:
        yy, xx = np.meshgrid(np.arange(Py) - Py / 2, np.arange(Px) - Px / 2, indexing='ij')
        bs = np.where(yy ** 2 + xx ** 2 < (min(Py, Px) / 5) ** 2, 0., 1.)
        bs[0, :] = 1e-6                                     # below the 1e-5 threshold: out of the loss
        bs[-1, :] = 3e-5                                    # above it: in, with weight 1
    shifts = idx = None
    if pp == 'shifts':
        n_ent, idx = (max(2, B - 4), None) if index_fn is None else index_fn(B)
        shifts = r.uniform(-2.5, 2.5, (n_ent, 2))
        shifts[0] = (1.75, -2.25)
        shifts[1] = (-1.5, 0.6)
        if shifts_fn is not None:
            shifts = np.asarray(shifts_fn(n_ent), np.float64)
        if index_fn is None:
            idx = np.concatenate([np.arange(n_ent), r.integers(0, n_ent, B - n_ent)]).astype(np.int32)   # some entries twice
        no_index = idx is None
        idx = np.arange(B, dtype=np.int32) if no_index else np.asarray(idx, np.int32)
        pprobes = np.stack([O.fourier_shift(probes, shifts[e], 'float64') for e in idx])              # [B, M, Py, Px]
    elif pp == 'probes':
        pprobes = rand_probes(B, M)
    else:
        pprobes = np.broadcast_to(probes, (B, M, Py, Px))

    # measured data: the truth object's far field / exit wave, fp64, through the same per-position probes and distances
    t_tiles, _ = O.extract_tiles(truth, pos, (Py, Px), unknown_type)
    mag = np.concatenate([O.predict(t_tiles[b:b + 1], pprobes[b], phys[b % len(phys)], 'float64')[0] for b in range(B)])
    meas = mag ** 2 if raw_data_type == 'intensity' else mag
    if meas_edit is not None:
        meas = meas_edit(meas, bs)
    if loss == 'lsq':
        target = O.target_magnitude(meas, raw_data_type)
    else:
        target = np.abs(meas) ** 2 if raw_data_type == 'magnitude' else np.abs(meas)     # the engine takes the intensity

    # oracle, position by position
    lkw = dict(loss_function_type=loss, raw_data_type=raw_data_type, poisson_multiplier=poisson_multiplier, beamstop=bs)
    out = {}
    for dt, sfx in (('float64', '_o'), ('float32', '_32')):
        tiles, _ = O.extract_tiles(obj.astype(dt), pos, (Py, Px), unknown_type)
        lsum, lpos, preds, gts = 0., [], [], []
        gp = np.zeros((M, Py, Px), complex)
        gpb = np.zeros((B, M, Py, Px), complex)
        gs = np.zeros((0 if shifts is None else len(shifts), 2))
        for b in range(B):
            ph, mb = phys[b % len(phys)], meas[b:b + 1]
            if pp == 'shifts':
                l, pr, gt, g, gsh = O.forward_adjoint_tiles(tiles[b:b + 1], probes, mb, ph, dt, shifts=shifts[idx[b]][None], **lkw)
                gp += g
                gs[idx[b]] += gsh[0]
                gpb[b] = O.forward_adjoint_tiles(tiles[b:b + 1], pprobes[b], mb, ph, dt, **lkw)[3]
            else:
                l, pr, gt, g = O.forward_adjoint_tiles(tiles[b:b + 1], pprobes[b], mb, ph, dt, **lkw)
                gp += g
            lsum += l
            lpos.append(l)
            preds.append(pr)
            gts.append(gt)
        out['loss' + sfx] = lsum / B
        out['loss_b' + sfx] = np.array(lpos, np.float64)     # every position's own loss (a mean over its judged detector pixels)
        out['pred' + sfx] = np.concatenate(preds)
        out['grad' + sfx] = O.scatter_tiles_adj(np.concatenate(gts), pos, obj.shape) / B
        out['gprobe' + sfx] = gp / B
        out['gprobe_b' + sfx] = gpb / B
        out['gshift' + sfx] = gs / B

    if pp == 'shifts' and no_index:
        idx = None
    out.update(obj=obj, pos=pos, probes=probes, pprobes=pprobes, target=target, beamstop=bs, shifts=shifts, idx=idx, meas=meas,
               n_det=Py * Px if bs is None else int((np.asarray(bs) >= 1e-5).sum()),
               kw=dict(S=S, B=B, n_modes=M, unknown_type=unknown_type, binning=binning, transmission_cache=transmission_cache,
                       free_prop=free_prop, sign_convention=sign_convention, normalize_fft=normalize_fft, fresnel_approx=fresnel_approx,
                       loss=loss, poisson_multiplier=poisson_multiplier, pp=pp, generic=generic, shape=(Py, Px)))
    return out


def run_engine(A, ctx, case):
    """The engine's results for a case of oracle_case, added to it: rotate -> multislice -> rotate_adjoint."""
    out, k = case, case['kw']
    obj, pos, probes, pprobes, target, bs, shifts, idx = [case[n] for n in ('obj', 'pos', 'probes', 'pprobes', 'target', 'beamstop',
                                                                            'shifts', 'idx')]
    (Py, Px), S, B, M, pp = k['shape'], k['S'], k['B'], k['n_modes'], k['pp']
    Y, X = obj.shape[:2]
    eng = A.MultisliceEngine(ctx, (Y, X, S), (Py, Px), pos, ENERGY_EV, PSIZE_CM, free_prop_cm=k['free_prop'], binning=k['binning'],
                             fresnel_approx=k['fresnel_approx'], sign_convention=k['sign_convention'], normalize_fft=k['normalize_fft'],
                             n_probe_modes=M, max_batch=B, loss_function_type=k['loss'], poisson_multiplier=k['poisson_multiplier'],
                             unknown_type=k['unknown_type'], beamstop=bs, generic=k['generic'], transmission_cache=k['transmission_cache'])
    d_grad = ctx.zeros(obj.shape)
    d_probe = ctx.array(c2(probes))
    d_gp = ctx.zeros((M, Py, Px, 2))
    eng.set_batch(pos, target)
    eng.rotate(ctx.array(obj, np.float32), None)
    if pp == 'shifts':
        d_gs = ctx.zeros(shifts.shape)
        d_shifts, d_idx = ctx.array(shifts, np.float32), ctx.array(idx) if idx is not None else None
        eng.multislice(d_probe, grad_probe=d_gp, want_pred=True, shifts=d_shifts, shift_index=d_idx, grad_shifts=d_gs)
        out['gshift'] = d_gs.get()
        out['gprobe_b'] = cplx(eng._gprobes_b.get()[:B])          # the per-position probe gradients, before the shift adjoint
    elif pp == 'probes':
        d_pprobes = ctx.array(c2(pprobes))
        eng.multislice(None, want_pred=True, probes_b=d_pprobes)
    else:
        eng.multislice(d_probe, grad_probe=d_gp, want_pred=True)
    eng.rotate_adjoint(d_grad, None)
    out['pred'] = eng.pred()
    out['loss'] = eng.loss()
    out['grad'] = d_grad.get()
    out['gprobe'] = cplx(d_gp.get()) if pp != 'probes' else None
    eng.plan.close()
    return out


def _grad_ok(e, e32, bars, what):
    assert e < bars['grad'], (what, e, e32)
    assert e <= 3 * e32 + bars['grad_abs'], (what, e, e32)


def check(res, bars=TUNED):
    """Prediction (whole batch and every position), loss, object gradient, probe gradient (whole and every mode), per-position
    probe gradients and shift gradients where the case has them."""
    e = rel(res['pred'], res['pred_o'])
    assert e < bars['pred'], ('pred', e)
    per = [rel(p, po) for p, po in zip(res['pred'], res['pred_o'])]
    assert max(per) < bars['pred'], ('pred per position', np.argmax(per), max(per))
    assert abs(res['loss'] - res['loss_o']) <= bars['loss'] * abs(res['loss_o']), ('loss', res['loss'], res['loss_o'])
    _grad_ok(rel(res['grad'], res['grad_o']), rel(res['grad_32'], res['grad_o']), bars, 'object gradient')
    if res['gprobe'] is not None:
        if bars['probe_3x']:
            _grad_ok(rel(res['gprobe'], res['gprobe_o']), rel(res['gprobe_32'], res['gprobe_o']), bars, 'probe gradient')
            for m in range(len(res['gprobe'])):
                _grad_ok(rel(res['gprobe'][m], res['gprobe_o'][m]), rel(res['gprobe_32'][m], res['gprobe_o'][m]), bars,
                         'probe gradient of mode %d' % m)
        else:
            e = rel(res['gprobe'], res['gprobe_o'])
            assert e < bars['grad'], ('probe gradient', e)
    if 'gprobe_b' in res:
        _grad_ok(rel(res['gprobe_b'], res['gprobe_b_o']), rel(res['gprobe_b_32'], res['gprobe_b_o']), bars, 'per-position probe gradients')
    if 'gshift' in res:
        e = rel(res['gshift'], res['gshift_o'])
        assert e < bars['shift'], ('shift gradient', e)
