"""The streamed multislice path (adm_ms_streamed.hip, adm_plan_create_streamed): probes larger than 128 x 128 -- which no
one-workgroup kernel takes -- against the fp64 oracle, the streamed kernels against the LDS kernels at sizes both serve, the
engine's dispatch, refusals and memory-bounded rounds, and the driver in 2-D and 3-D (pytest -m gpu).

Cases come from tests/ms_matrix.py (oracle_case: positions hanging over all four edges, truth with ten times the guess's contrast)
and are judged by its GENERIC bars: the 3x rule with the oracle's own fp32 run as the yardstick.
"""
import numpy as np
import pytest

from tests import ms_matrix as MM
from oracle import adorym_oracle as O      # checker only
import cases

pytestmark = pytest.mark.gpu


@pytest.fixture(scope='module')
def A():
    import adorym_amd
    return adorym_amd


@pytest.fixture(scope='module')
def ctx(A):
    c = A.Context(0)
    yield c
    c.close()


def run_streamed(A, ctx, case, streamed=True, want_grad=True, **engine_kw):
    """ms_matrix.run_engine with the engine's ``streamed`` choice (and further engine keywords): rotate -> multislice ->
    rotate_adjoint on one shared probe set.  Returns the case with the engine's results added, and the engine's streamed flag.
    ``want_grad`` False: the forward-only launch; 'gprobe_raw' and 'grad_rot' are then the probe-gradient buffer (handed over
    filled with 3) and the engine's rotated-frame gradient (filled with 5) as the launch left them."""
    out, k = dict(case), case['kw']
    obj, pos, probes, target, bs = [case[n] for n in ('obj', 'pos', 'probes', 'target', 'beamstop')]
    (Py, Px), S, B, M = k['shape'], k['S'], k['B'], k['n_modes']
    Y, X = obj.shape[:2]
    eng = A.MultisliceEngine(ctx, (Y, X, S), (Py, Px), pos, MM.ENERGY_EV, MM.PSIZE_CM, free_prop_cm=k['free_prop'], binning=k['binning'],
                             fresnel_approx=k['fresnel_approx'], sign_convention=k['sign_convention'], normalize_fft=k['normalize_fft'],
                             n_probe_modes=M, max_batch=B, loss_function_type=k['loss'], poisson_multiplier=k['poisson_multiplier'],
                             unknown_type=k['unknown_type'], beamstop=bs, transmission_cache=k['transmission_cache'], streamed=streamed,
                             **engine_kw)
    d_grad = ctx.zeros(obj.shape)
    d_probe = ctx.array(MM.c2(probes))
    d_gp = ctx.zeros((M, Py, Px, 2))
    eng.set_batch(pos, target)
    eng.rotate(ctx.array(obj, np.float32), None)
    if want_grad:
        eng.multislice(d_probe, grad_probe=d_gp, want_pred=True)
        eng.rotate_adjoint(d_grad, None)
        out['grad'] = d_grad.get()
        out['gprobe'] = MM.cplx(d_gp.get())
    else:
        d_gp = ctx.array(np.full((M, Py, Px, 2), 3, np.float32))
        eng.grad_rot.set(np.full(eng.grad_rot.shape, 5, np.float32))
        eng.multislice(d_probe, grad_probe=d_gp, want_grad=False, want_pred=True)
        out['gprobe_raw'], out['grad_rot'] = d_gp.get(), eng.grad_rot.get()
    out['pred'] = eng.pred()
    out['loss'] = eng.loss()
    out['streamed'] = eng.streamed
    out['n_rounds'] = len(eng.rounds(B))
    eng.plan.close()
    return out


# ---------------------------------------------------------------------------------------------------- 1. against the oracle
ORACLE_CASES = {
    'P256_2d_far': dict(P=256, S=1, B=11),
    'P256_S6_modes': dict(P=256, S=6, n_modes=3),
    'P200x240_fresnel_real_imag': dict(P=(200, 240), S=4, free_prop=1e-4, unknown_type='real_imag'),
    'P160_binning2_nocache': dict(P=160, S=5, binning=2, transmission_cache=False),
    'P135_near_poisson_beamstop_modes': dict(P=135, S=3, free_prop=0, loss='poisson', raw_data_type='intensity', poisson_multiplier=50.,
                                             beamstop=True, n_modes=3),
    'P512_S2': dict(P=512, S=2, B=4),
}


@pytest.mark.parametrize('name', list(ORACLE_CASES))
def test_streamed_vs_oracle(A, ctx, name):
    """Probe sizes beyond the LDS kernels, up to 512 (and 135 = 3^3 * 5, 200 x 240) on the streamed plan: prediction, loss, object
    gradient, probe gradient against the fp64 oracle.  Every one of these runs column workgroups of 256 threads over 8 columns
    and several rows per row workgroup; the launch geometries beyond (sides up to 2048, large prime sides) are swept by
    tests/st_matrix.py and tests/test_gpu_streamed_matrix.py."""
    kw = dict(ORACLE_CASES[name])
    res = run_streamed(A, ctx, MM.oracle_case(kw.pop('P'), **kw))
    assert res['streamed']
    MM.check(res, MM.GENERIC)


VARIANTS_256 = [v for v in MM.VARIANTS if v != 'three_distances_pp']


@pytest.mark.parametrize('variant', VARIANTS_256)
def test_streamed_256_detector_and_loss_variants_vs_oracle(A, ctx, variant):
    """Every detector / loss variant of the kernel matrix (one shared probe set) at 256 x 256."""
    res = run_streamed(A, ctx, MM.oracle_case(256, S=3, seed=1, **MM.VARIANTS[variant]))
    MM.check(res, MM.GENERIC)


# ---------------------------------------------------------------------------------------------------- 2. against the LDS kernels
@pytest.mark.regression
@pytest.mark.parametrize('P', [72, 64, 128, (127, 129)])
def test_streamed_matches_lds_kernels(A, ctx, P):
    """The streamed kernels forced where the tuned (72, 64) or the generic (128^2, 127 x 129) kernels run: loss, prediction, object
    gradient and the probe gradient of every mode agree to 1e-5."""
    case = MM.oracle_case(P, S=4, B=11, n_modes=2, seed=3)
    lds, st = run_streamed(A, ctx, case, streamed=False), run_streamed(A, ctx, case, streamed=True)
    assert st['streamed'] and not lds['streamed']
    assert abs(st['loss'] - lds['loss']) <= 1e-5 * abs(lds['loss']), (st['loss'], lds['loss'])
    assert MM.rel(st['pred'], lds['pred']) < 1e-5
    assert MM.rel(st['grad'], lds['grad']) < 1e-5
    for m in range(2):
        assert MM.rel(st['gprobe'][m], lds['gprobe'][m]) < 1e-5, m


# ---------------------------------------------------------------------------------------------------- 3. dispatch, refusals, rounds
def _engine(A, ctx, shape, **kw):
    Py, Px = shape
    return A.MultisliceEngine(ctx, (Py + 6, Px + 6, 2), shape, np.array([(0, 0), (3, 5)]), MM.ENERGY_EV, MM.PSIZE_CM, max_batch=2, **kw)


def test_auto_dispatch(A, ctx):
    """'auto' keeps the LDS kernels up to 128 x 128 and takes the streamed plan beyond; adm_plan_create still refuses beyond."""
    e = _engine(A, ctx, (128, 128), streamed='auto')
    assert e.streamed is False
    e.plan.close()
    e = _engine(A, ctx, (129, 128), streamed='auto')
    assert e.streamed is True
    e.plan.close()
    with pytest.raises(NotImplementedError, match='too large'):
        _engine(A, ctx, (129, 128))
    with pytest.raises(NotImplementedError, match='at most 2048'):
        _engine(A, ctx, (8, 2049), streamed=True)


def test_streamed_refusals(A, ctx):
    """One probe set shared by all positions: shifted and per-position probes are refused, by the engine and by the C ABI."""
    from adorym_amd._lib import check
    P, M = 136, 1
    eng = _engine(A, ctx, (P, P), streamed=True)
    probe = ctx.zeros((M, P, P, 2))
    eng.set_batch(np.array([(0, 0), (3, 5)]), np.ones((2, P, P), np.float32))
    with pytest.raises(NotImplementedError, match='streamed'):
        eng.multislice(probe, shifts=ctx.zeros((2, 2)))
    with pytest.raises(NotImplementedError, match='streamed'):
        eng.multislice(None, probes_b=ctx.zeros((2, M, P, P, 2)))
    lib, h = ctx.lib, eng.plan.handle
    with pytest.raises(NotImplementedError, match='streamed'):
        check(lib.adm_multislice_fwd_adj_pp(h, eng.obj_rot.ptr, probe.ptr, eng._cur_pos.ptr, 2, eng._cur_target.ptr, 1, None, None,
                                            eng._loss.ptr, 1.0, eng._ws.ptr, eng._ws.nbytes))
    with pytest.raises(NotImplementedError, match='streamed'):
        check(lib.adm_probe_shift(h, probe.ptr, ctx.zeros((2, 2)).ptr, None, 2, ctx.zeros((2, M, P, P, 2)).ptr))
    with pytest.raises(NotImplementedError, match='streamed'):
        eng.plan.set_generic(True)
    eng.plan.close()
    e2 = _engine(A, ctx, (P, P), streamed=True, free_prop_cm=1e-4)
    with pytest.raises(NotImplementedError, match='per position'):
        e2.plan.set_detector_kernels([np.ones((P, P), complex)] * 2)
    e2.plan.close()


def test_streamed_rounds_within_workspace_budget(A, ctx):
    """A batch split into rounds by a small workspace budget: each round overlap-added before the next reuses the workspace.
    Against the oracle, and against the one-round launch (object gradient up to the order of the additions)."""
    case = MM.oracle_case(256, S=2, B=11, n_modes=2, seed=4)
    one = run_streamed(A, ctx, case)
    probe_eng = A.MultisliceEngine(ctx, (265, 269, 2), (256, 256), case['pos'], MM.ENERGY_EV, MM.PSIZE_CM, n_probe_modes=2, streamed=True)
    budget = probe_eng.plan.workspace_bytes(4)
    probe_eng.plan.close()
    parts = run_streamed(A, ctx, case, workspace_budget=budget)
    assert one['n_rounds'] == 1 and parts['n_rounds'] == 3
    MM.check(parts, MM.GENERIC)
    assert parts['loss'] == one['loss']
    assert np.array_equal(parts['pred'], one['pred'])
    assert MM.rel(parts['gprobe'], one['gprobe']) < 1e-6
    assert MM.rel(parts['grad'], one['grad']) < 1e-6


# ---------------------------------------------------------------------------------------------------- 4-6. the driver
def _probes(r, M, P):
    yy, xx = np.meshgrid(np.arange(P) - P / 2, np.arange(P) - P / 2, indexing='ij')
    env = np.exp(-(yy ** 2 + xx ** 2) / (2 * (P / 5) ** 2))
    return np.stack([(0.6 ** m) * env * np.exp(1j * (0.3 * m + 0.5 * r.uniform(-1, 1, (P, P)))) for m in range(M)])


def test_driver_2d_256_probe_modes_vs_oracle(A, ctx, tmp_path):
    """reconstruct_ptychography in two_d_mode with a 256 x 256 probe (2 modes) at integer positions, intensity data, Adam on object
    and probe over 2 epochs, against O.reconstruct_2d in fp64 with its fp32 run as the yardstick (the bars of the dense-scan test)."""
    r = cases.rng(2600)
    N, P, M = 300, 256, 2
    pos = np.array([(y, x) for y in (0, 22, 44) for x in (0, 22, 44)], dtype=float)
    truth = np.stack([2e-3 * cases.smooth_field((N, N, 1), 2601), 2e-4 * cases.smooth_field((N, N, 1), 2602)], -1)
    probes = _probes(r, M, P)
    phys = O.Physics((P, P), 8000., 1e-6)
    tiles, _ = O.extract_tiles(truth, pos.astype(int), (P, P))
    prj = (O.predict(tiles, probes, phys, 'float64')[0] ** 2)[None].astype(np.float32)      # intensity data
    guess = [np.full((N, N, 1), 2e-4), np.full((N, N, 1), 2e-5)]
    kw = dict(n_epochs=2, minibatch_size=4, learning_rate=1e-5, raw_data_type='intensity', optimize_probe=True, probe_learning_rate=1e-3)
    st = A.reconstruct_ptychography(
        fname=prj, obj_size=(N, N, 1), probe_pos=pos, theta_st=0, theta_end=0, n_theta=1, two_d_mode=True, energy_ev=8000., psize_cm=1e-6,
        free_prop_cm='inf', n_probe_modes=M, probe_type='supplied', probe_initial=[np.abs(probes), np.angle(probes)], initial_guess=guess,
        gamma=0, alpha_d=0, alpha_b=0, optimizer='adam', save_path=str(tmp_path), output_folder='p256', store_checkpoint=False,
        use_checkpoint=False, return_state=True, **kw)
    runs = {dt: O.reconstruct_2d(prj.astype(np.float64), guess, probes, pos, phys, dtype=dt, **kw) for dt in ('float64', 'float32')}
    o64, o32 = runs['float64'], runs['float32']
    assert len(st['losses']) == len(o64['losses'])
    assert np.allclose(st['losses'], o64['losses'], rtol=max(2e-4, 3 * np.abs(np.array(o32['losses']) / np.array(o64['losses']) - 1).max()))
    x = np.stack([st['delta'], st['beta']], -1)
    upd = np.linalg.norm(o64['obj'] - np.stack(guess, -1))
    e, e_ref = np.linalg.norm(x - o64['obj']) / upd, np.linalg.norm(o32['obj'] - o64['obj']) / upd
    assert upd > 0 and e < max(5e-3, 3 * e_ref), (e, e_ref)
    p = st['probe_real'] + 1j * st['probe_imag']
    pn = np.linalg.norm(o64['probes'])
    assert np.linalg.norm(p - o64['probes']) / pn < max(1e-4, 3 * np.linalg.norm(o32['probes'] - o64['probes']) / pn)


@pytest.mark.parametrize('update_scheme', ['immediate', 'per angle'])
def test_driver_3d_256_probe_vs_oracle(A, ctx, tmp_path, update_scheme):
    """A 264 x 264 x 8 object, 3 angles, a 256 x 256 probe, far field: the driver against O.reconstruct in fp64 (3x rule with the
    oracle's fp32 run as the yardstick)."""
    N, Z, P, n_theta = 264, 8, 256, 3
    truth = np.stack([2e-5 * cases.smooth_field_fast((N, N, Z), 2701), 2e-6 * cases.smooth_field_fast((N, N, Z), 2702)], -1)
    theta_ls = np.linspace(0, np.pi, n_theta, dtype='float32')
    phys = O.Physics((P, P), 5000., 1e-7)
    probe = _probes(cases.rng(2703), 1, P)[0]
    pos = np.array([(0, 0), (0, 8), (8, 0), (8, 8)], dtype=float)
    prj = np.zeros((n_theta, len(pos), P, P))
    for i, th in enumerate(theta_ls):
        rot = O.rotate_fwd(truth, O.rotation_coords((N, N, Z), th), 'float64')
        tiles, _ = O.extract_tiles(rot, pos.astype(int), (P, P))
        prj[i] = O.predict(tiles, probe, phys, 'float64')[0]
    guess = [np.full((N, N, Z), 2e-6), np.full((N, N, Z), 2e-7)]
    kw = dict(n_epochs=1, minibatch_size=2, optimizer='adam', learning_rate=1e-7, update_scheme=update_scheme)
    st = A.reconstruct_ptychography(fname=prj.astype(np.float32), obj_size=(N, N, Z), probe_pos=pos, theta_st=0, theta_end=np.pi,
                                    n_theta=n_theta, energy_ev=5000., psize_cm=1e-7, free_prop_cm='inf', probe_type='supplied',
                                    probe_initial=[np.abs(probe), np.angle(probe)], initial_guess=guess, gamma=0, alpha_d=0,
                                    alpha_b=0, save_path=str(tmp_path), output_folder='p256_3d', store_checkpoint=False, use_checkpoint=False,
                                    return_state=True, **kw)
    runs = {}
    for dt in ('float64', 'float32'):
        runs[dt] = O.reconstruct(prj.astype(np.float32).astype(np.float64), guess, probe, pos, theta_ls, phys, dtype=dt, return_trace=True,
                                 alpha_d=None, alpha_b=None, gamma=None, **kw)
    (o64, l64, _), (o32, l32, _) = runs['float64'], runs['float32']
    assert len(st['losses']) == len(l64)
    assert np.allclose(st['losses'], l64, rtol=max(2e-4, 3 * np.abs(np.array(l32) / np.array(l64) - 1).max()))
    x = np.stack([st['delta'], st['beta']], -1)
    upd = np.linalg.norm(o64 - np.stack(guess, -1))
    e, e_ref = np.linalg.norm(x - o64) / upd, np.linalg.norm(o32 - o64) / upd
    assert upd > 0 and e < max(5e-3, 3 * e_ref), (e, e_ref)


def test_driver_refuses_position_refinement_with_streamed_probe(A, ctx, tmp_path):
    """Sub-pixel probe shifts are not implemented on the streamed path: a 256 x 256 probe with optimize_all_probe_pos is refused
    up front, naming the probe size."""
    N, P = 270, 256
    prj = np.ones((1, 2, P, P), np.float32)
    with pytest.raises(NotImplementedError, match='256 x 256'):
        A.reconstruct_ptychography(fname=prj, obj_size=(N, N, 1), probe_pos=np.array([(0., 0.), (4., 6.)]), theta_st=0, theta_end=0, n_theta=1,
                                   two_d_mode=True, energy_ev=8000., psize_cm=1e-6, free_prop_cm='inf', probe_type='plane',
                                   initial_guess=[np.zeros((N, N, 1)), np.zeros((N, N, 1))], optimize_all_probe_pos=True, n_epochs=1,
                                   minibatch_size=2, gamma=0, alpha_d=0, alpha_b=0, save_path=str(tmp_path), output_folder='ref',
                                   store_checkpoint=False, use_checkpoint=False, return_state=True)
