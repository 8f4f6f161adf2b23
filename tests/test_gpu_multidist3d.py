"""One exit wave to several detector planes on the GPU (pytest -m gpu): the fan-out / fan-in detector step of the streamed multislice
path (adm_ms_multidist.hip), through the engine (MultisliceEngine(detector_fanout=True)) and the C ABI
(adm_plan_set_detector_fanout, adm_multislice_fwd_adj) as the engine calls it.

Checkers: golden F27 (recorded from the reference, tests/golden/gen_f27_multidist_3d.py) and the NumPy restatement
tests/multidist3d_ref.py (tied to the reference by tests/test_multidist3d_ref_vs_golden.py).  Prediction, loss, object and probe
gradients: the bars tests/ms_matrix.py:check applies with GENERIC, the object gradient under the 3x rule with the checker's own
fp32 run as the yardstick; at the launch geometries also the prediction and the probe gradient band by band along the row and
column workgroups (tests/test_gpu_streamed_matrix.py:check_bands).
"""
import ast
import os

import numpy as np
import pytest

from tests import ms_matrix as MM
from tests import st_matrix as SM
from tests import multidist3d_ref as MR
from tests.test_gpu_streamed_matrix import check_bands
from oracle import adorym_oracle as O      # checker only

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENERGY_EV, PSIZE_CM = 8000., 1e-6
BARS = MM.GENERIC
DISTS_CM = [1e-4, 2e-4, 3.5e-4, 5e-4]
rel = MM.rel


@pytest.fixture(scope='module')
def A():
    import adorym_amd
    return adorym_amd


@pytest.fixture(scope='module')
def ctx(A):
    c = A.Context(0)
    yield c
    c.close()


@pytest.fixture(scope='module')
def F():
    return np.load(os.path.join(ROOT, 'tests', 'golden', 'F27_multidist_3d.npz'))


def _engine(A, ctx, case, dists, fanout=True, **engine_kw):
    obj, pos, probes = case['obj'], case['pos'], case['probes']
    M, Py, Px = probes.shape
    Y, X, S = obj.shape[:3]
    return A.MultisliceEngine(ctx, (Y, X, S), (Py, Px), pos, ENERGY_EV, PSIZE_CM, free_prop_cm=dists, sign_convention=case['sign_convention'],
                              n_probe_modes=M, loss_function_type=case.get('loss', 'lsq'), poisson_multiplier=case.get('poisson_multiplier', 1.),
                              beamstop=case.get('beamstop'), streamed=True, detector_fanout=fanout, **engine_kw)


def launch(ctx, eng, case, target, want_grad=True):
    """rotate -> multislice -> rotate_adjoint on the engine.  ``want_grad`` False: 'gprobe_raw' and 'grad_rot' are the probe-gradient
    buffer (handed over filled with 3) and the engine's rotated-frame gradient (filled with 5) as the launch left them."""
    obj, pos, probes = case['obj'], case['pos'], case['probes']
    M, Py, Px = probes.shape
    d_grad = ctx.zeros(obj.shape)
    d_gp = ctx.zeros((M, Py, Px, 2)) if want_grad else ctx.array(np.full((M, Py, Px, 2), 3, np.float32))
    eng.set_batch(pos, np.asarray(target, np.float32))
    eng.rotate(ctx.array(obj, np.float32), None)
    out = {}
    if want_grad:
        eng.multislice(ctx.array(MM.c2(probes)), grad_probe=d_gp, want_pred=True)
        eng.rotate_adjoint(d_grad, None)
        out.update(grad=d_grad.get(), gprobe=MM.cplx(d_gp.get()))
    else:
        eng.grad_rot.set(np.full(eng.grad_rot.shape, 5, np.float32))
        eng.multislice(ctx.array(MM.c2(probes)), grad_probe=d_gp, want_grad=False, want_pred=True)
        out.update(gprobe_raw=d_gp.get(), grad_rot=eng.grad_rot.get())
    out.update(pred=eng.pred(), loss=eng.loss(), n_rounds=len(eng.rounds(len(pos))))
    return out


def run_fanout(A, ctx, case, want_grad=True, **engine_kw):
    """An engine with ``detector_fanout`` on ``case``: obj [Y,X,S,2], pos, probes [M,Py,Px] complex, dists, target [B*D,Py,Px]."""
    eng = _engine(A, ctx, case, case['dists'], **engine_kw)
    assert eng.streamed is True and eng.n_dists == eng.det_per_pos == len(case['dists'])
    out = launch(ctx, eng, case, case['target'], want_grad)
    eng.plan.close()
    return out


def ref_fanout(case, dtype):
    phys = O.Physics(case['probes'].shape[-2:], ENERGY_EV, PSIZE_CM, free_prop_cm=case['dists'][0], sign_convention=case['sign_convention'])
    kw = dict(loss_function_type=case.get('loss', 'lsq'), raw_data_type=case.get('raw_data_type', 'magnitude'),
              poisson_multiplier=case.get('poisson_multiplier', 1.), beamstop=case.get('beamstop'))
    l, p, g, gp = MR.forward_adjoint_object(case['obj'].astype(np.float64), None, case['probes'].astype(np.complex128), case['pos'],
                                            case['meas'], phys, case['dists'], dtype, **kw)
    return dict(loss=l, pred=p, grad=g, gprobe=gp)


def as_res(res, r64, r32, case):
    """The layout ms_matrix.check and check_bands read."""
    out = dict(res)
    for k in ('pred', 'loss', 'grad', 'gprobe'):
        out[k + '_o'], out[k + '_32'] = r64[k], r32[k]
    out['kw'] = dict(shape=tuple(case['probes'].shape[-2:]), free_prop=case['dists'][0])
    return out


def report(res, what):
    print('%s: pred %.2e (fp32 ref %.2e)  loss %.2e  grad %.2e (%.2e)  gprobe %.2e (%.2e)' % (
        what, rel(res['pred'], res['pred_o']), rel(res['pred_32'], res['pred_o']), abs(res['loss'] / res['loss_o'] - 1),
        rel(res['grad'], res['grad_o']), rel(res['grad_32'], res['grad_o']), rel(res['gprobe'], res['gprobe_o']),
        rel(res['gprobe_32'], res['gprobe_o'])))


# ------------------------------------------------------------------------------------------- 1. the fixture's cases (the reference)
FIXTURE_CASES = ['m1_p1_magnitude', 'm1_m1_intensity', 'm2_p1_intensity', 'm2_m1_magnitude']


def fixture_case(F, name):
    names = [str(n) for n in F['kernel_cases']]
    sg, M, rdt = ast.literal_eval(str(F['kernel_case_params'][names.index(name)]))
    c = {k: F['%s/%s' % (name, k)] for k in ('obj', 'pos', 'probes', 'meas')}
    c.update(sign_convention=sg, raw_data_type=rdt, dists=[float(d) for d in F['kernel_dists_cm']])
    c['target'] = O.target_magnitude(c['meas'], rdt)
    return c


@pytest.mark.parametrize('name', FIXTURE_CASES)
def test_kernels_vs_reference(A, ctx, F, name):
    """md_fanout_kernel<false>, md_fanin_kernel<false>: prediction, loss, object gradient and probe gradients against the reference's fp64 run, the
    reference's own fp32 run as the yardstick of the 3x rule (field 12 x 20, S = 5, D = 3; one and two modes, both sign
    conventions, magnitude and intensity data)."""
    case = fixture_case(F, name)
    res = run_fanout(A, ctx, case)
    e32 = F[name + '/err32']
    M = case['probes'].shape[0]
    e = rel(res['pred'], F[name + '/pred'])
    per = max(rel(p, po) for p, po in zip(res['pred'], F[name + '/pred']))
    print(name, 'pred %.2e, worst entry %.2e (fp32 ref %.2e)' % (e, per, e32[0]))
    assert e < BARS['pred'] and per < BARS['pred'], ('pred', e, per)
    e = abs(res['loss'] / float(F[name + '/loss']) - 1)
    print(name, 'loss %.2e (fp32 ref %.2e)' % (e, e32[1]))
    assert e <= BARS['loss'], ('loss', e)
    e = rel(res['grad'], F[name + '/grad'])
    print(name, 'grad %.2e (fp32 ref %.2e)' % (e, e32[2]))
    assert e < BARS['grad'] and e <= 3 * e32[2] + BARS['grad_abs'], ('object gradient', e, e32[2])
    e = rel(res['gprobe'], F[name + '/gprobe'])
    print(name, 'gprobe %.2e (fp32 ref %.2e)' % (e, e32[3]))
    assert e < BARS['grad'] and e <= 3 * e32[3] + BARS['grad_abs'], ('probe gradient', e, e32[3])
    for m in range(M):
        e = rel(res['gprobe'][m], F[name + '/gprobe'][m])
        print(name, 'gprobe of mode %d %.2e (fp32 ref %.2e)' % (m, e, e32[4 + m]))
        assert e < BARS['grad'] and e <= 3 * e32[4 + m] + BARS['grad_abs'], ('probe gradient of mode', m, e, e32[4 + m])


# --------------------------------------------------------------------------------- 2. launch geometries (the restatement)
def make_case(P, S=2, B=3, M=1, D=2, sign_convention=1, seed=0, loss='lsq', poisson_multiplier=1., beamstop=None):
    """Built like ms_matrix.oracle_case: positions hanging over the object's edges, a truth with ten times the guess's contrast
    makes the data."""
    Py, Px = (P, P) if np.isscalar(P) else tuple(P)
    r = np.random.default_rng([Py, Px, S, B, M, D, seed])
    Y, X = Py + 9, Px + 13
    mk = lambda c: np.stack([2e-3 * c * r.uniform(size=(Y, X, S)), 2e-4 * c * r.uniform(size=(Y, X, S))], -1)
    obj, truth = mk(1).astype(np.float32), mk(10).astype(np.float32)
    pos = MM.edge_positions(r, B, Y, X, Py, Px)
    probes = ((0.5 + r.uniform(0, 1, (M, Py, Px))) * np.exp(1j * r.uniform(-np.pi, np.pi, (M, Py, Px)))).astype(np.complex64)
    dists = DISTS_CM[:D]
    phys = O.Physics((Py, Px), ENERGY_EV, PSIZE_CM, free_prop_cm=dists[0], sign_convention=sign_convention)
    tiles, _ = O.extract_tiles(truth.astype(np.float64), pos, (Py, Px))
    meas = MR.predict(tiles, probes.astype(np.complex128), phys, dists).astype(np.float32)
    case = dict(obj=obj, pos=pos, probes=probes, dists=dists, meas=meas, sign_convention=sign_convention, loss=loss,
                poisson_multiplier=poisson_multiplier, beamstop=beamstop, raw_data_type='magnitude')
    case['target'] = meas if loss == 'lsq' else meas ** 2          # (the engine takes the intensity under the Poisson loss)
    return case


_YARD = {}


def yardstick(key, case):
    """The restatement in fp64 and in fp32, built once per module."""
    if key not in _YARD:
        _YARD[key] = (ref_fanout(case, 'float64'), ref_fanout(case, 'float32'))
    return _YARD[key]


def judge(res, r64, r32, case, what):
    res = as_res(res, r64, r32, case)
    report(res, what)
    for k in ('grad', 'gprobe'):       # (a well-conditioned case: the checker's own fp32 run is well inside the cap)
        assert rel(res[k + '_32'], res[k + '_o']) < BARS['grad'] / 3, (what, k, 'ill-conditioned case')
    MM.check(res, BARS)
    check_bands(res, what)
    return res


#            field: (what it reaches, further make_case arguments)
GEOMETRIES = {
    (24, 24): dict(M=2),
    (520, 7): dict(),                     # narrower than cw
    (640, 12): dict(M=2),                 # 320 threads
    (1000, 9): dict(),
    (1024, 16): dict(),                   # the largest cw = 8 column
    (1025, 12): dict(),                   # the smallest cw = 4
    (2048, 5): dict(),                    # the largest column, a last group of 1
    (1031, 10): dict(),                   # one direct-sum pass
}
GEOMETRY_CASES = [(shape, 2) for shape in GEOMETRIES] + [((640, 12), 1), ((1025, 12), 4)]


def test_the_geometries_reach_the_column_classes():
    reached = set().union(*(SM.classes(*shape) for shape in GEOMETRIES))
    for c in ('cw8_nt_gt256', 'cw4', 'nt512', 'colgroup_ragged', 'field_narrower_than_cw'):
        assert c in reached, c
    assert sum(1 for kw in GEOMETRIES.values() if kw.get('M', 1) == 2) >= 2
    assert {D for _, D in GEOMETRY_CASES} == {1, 2, 4} and all((s, 2) in GEOMETRY_CASES for s in GEOMETRIES)


def run_one_distance_fanout(A, ctx, case):
    """D = 1: the engine refuses a single distance by name, so the fan-out is switched on through the C ABI on a plain streamed
    Fresnel engine (before its workspace is sized).  Also returns that engine's results from before the switch."""
    eng = _engine(A, ctx, case, case['dists'][0], fanout=False)
    plain = launch(ctx, eng, case, case['target'])
    eng.plan.close()
    eng = _engine(A, ctx, case, case['dists'][0], fanout=False)
    eng.plan.set_detector_fanout([A.propagate.get_kernel(case['dists'][0] * 1e7, 1240. / ENERGY_EV, np.array([PSIZE_CM] * 3) * 1e7,
                                                         case['probes'].shape[-2:], sign_convention=case['sign_convention'])])
    out = launch(ctx, eng, case, case['target'])
    eng.plan.close()
    return out, plain


@pytest.mark.parametrize('shape,D', GEOMETRY_CASES, ids=lambda v: '%dx%d' % v if isinstance(v, tuple) else 'D%d' % v)
def test_geometries_vs_restatement(A, ctx, shape, D):
    """md_fanout_kernel<false>, md_fanin_kernel<false> at every column-launch geometry (tall, narrow fields: the full LDS layout at small cost);
    S = 2, B = 3 positions over the object's edges, D = 2 at every field and D = 1, D = 4 at one each."""
    case = make_case(shape, D=D, **GEOMETRIES[shape])
    r64, r32 = yardstick((shape, D), case)
    res = run_one_distance_fanout(A, ctx, case)[0] if D == 1 else run_fanout(A, ctx, case)
    judge(res, r64, r32, case, '%dx%d D=%d' % (shape + (D,)))


# ------------------------------------------------------------------------------------------ 3. against the single-distance path
@pytest.mark.regression
def test_fanout_matches_one_streamed_launch_per_distance(A, ctx):
    """The fan-out at D = 3 against three single-distance streamed launches of the same object (the path that existed before):
    the predictions agree within the prediction bar, and the object gradient is the sum of the three gradients times the
    loss-normalisation factor 1 / D (each launch normalises by its own B * pixels) within the gradient bar; so is the probe
    gradient.

    D = 1 (switched on through the C ABI) against the existing Fresnel detector path of the same engine: prediction, loss, object
    gradient and probe gradient are BIT-EQUAL (measured on an MI355X, 640 x 12, two modes); asserted here too, since both do the
    same arithmetic in the same order, but the issue does not make it a condition."""
    case = make_case((135, 21), S=3, B=3, M=2, D=3, seed=5)
    fan = run_fanout(A, ctx, case)
    D = 3
    grads, gprobes = [], []
    for d, dist in enumerate(case['dists']):
        eng = _engine(A, ctx, case, dist, fanout=False)
        one = launch(ctx, eng, case, case['target'][d::D])
        eng.plan.close()
        e = rel(fan['pred'][d::D], one['pred'])
        print('distance %d: pred %.2e' % (d, e))
        assert e < BARS['pred'], (d, e)
        grads.append(one['grad'].astype(np.float64))
        gprobes.append(one['gprobe'])
    e, ep = rel(fan['grad'], sum(grads) / D), rel(fan['gprobe'], sum(gprobes) / D)
    print('grad %.2e  gprobe %.2e' % (e, ep))
    assert e < BARS['grad'] and ep < BARS['grad'], (e, ep)
    one_d = make_case((640, 12), M=2, D=1, seed=6)
    f1, plain = run_one_distance_fanout(A, ctx, one_d)
    equal = {k: bool(np.array_equal(np.asarray(f1[k]), np.asarray(plain[k]))) for k in ('pred', 'loss', 'grad', 'gprobe')}
    print('D = 1 bit-equal to the Fresnel detector path:', equal)
    assert all(equal.values()), equal


# ------------------------------------------------------------------------------------------ 4. semantics
def test_rounds_within_workspace_budget(A, ctx):
    """A workspace budget that forces three rounds at D = 2 (one position each): losses and predictions are the one-round launch's
    bit for bit, the gradients up to the order of the overlap-add."""
    case = make_case((136, 24), S=3, B=3, M=2, D=2, seed=7)
    r64, r32 = ref_fanout(case, 'float64'), ref_fanout(case, 'float32')
    one = run_fanout(A, ctx, case)
    probe_eng = _engine(A, ctx, case, case['dists'])
    budget = probe_eng.plan.workspace_bytes(1)
    assert probe_eng.plan.workspace_bytes(3) - budget == 2 * (probe_eng.plan.workspace_bytes(2) - budget)       # linear in the batch
    probe_eng.plan.close()
    parts = run_fanout(A, ctx, case, workspace_budget=budget)
    assert one['n_rounds'] == 1 and parts['n_rounds'] == 3
    MM.check(as_res(parts, r64, r32, case), BARS)
    assert parts['loss'] == one['loss']
    assert np.array_equal(parts['pred'], one['pred'])
    assert rel(parts['gprobe'], one['gprobe']) < 1e-6
    assert rel(parts['grad'], one['grad']) < 1e-6


def test_workspace_grows_by_the_detector_fields(A, ctx):
    """adm_plan_workspace_bytes with a fan-out of D planes: B * D * M detector fields more, and with M > 1 the detector kernel's
    parked fields grow from B * M to B * D * M."""
    for M in (1, 2):
        case = make_case((40, 24), M=M, D=3, seed=8)
        plain, fan = _engine(A, ctx, case, case['dists'][0], fanout=False), _engine(A, ctx, case, case['dists'])
        fld, B, D = 40 * 24 * 8, 5, 3
        grow = fan.plan.workspace_bytes(B) - plain.plan.workspace_bytes(B)
        want = B * D * M * fld + (B * (D - 1) * M * fld if M > 1 else 0)
        assert want <= grow <= want + B * D * 64 + 64, (M, grow, want)        # (+ loss partials and positions per entry, alignment)
        plain.plan.close(), fan.plan.close()


def test_forward_only(A, ctx):
    """want_grad off: loss and prediction are the full launch's bit for bit and no gradient buffer is written."""
    case = make_case((136, 24), S=2, B=3, M=2, D=2, seed=9)
    full, fwd = run_fanout(A, ctx, case), run_fanout(A, ctx, case, want_grad=False)
    assert fwd['loss'] == full['loss'] and np.array_equal(fwd['pred'], full['pred'])
    assert np.all(fwd['gprobe_raw'] == 3) and np.all(fwd['grad_rot'] == 5)


def test_two_launches_give_identical_bits(A, ctx):
    case = make_case((135, 21), M=2, D=3, seed=10)
    a, b = run_fanout(A, ctx, case), run_fanout(A, ctx, case)
    for k in ('pred', 'loss', 'grad', 'gprobe'):
        assert np.array_equal(np.asarray(a[k]), np.asarray(b[k])), k


def test_detector_mask_shared_by_all_distances(A, ctx):
    """``beamstop=``: one mask for every distance; a NaN target under a dropped pixel changes nothing, bit for bit."""
    Py, Px = 40, 24
    yy, xx = np.meshgrid(np.arange(Py) - Py / 2, np.arange(Px) - Px / 2, indexing='ij')
    bs = np.where(yy ** 2 + xx ** 2 < 25, 0., 1.)
    bs[0, :] = 1e-6                                     # below the 1e-5 threshold: out of the loss
    case = make_case((Py, Px), S=2, B=3, M=2, D=2, seed=11, beamstop=bs)
    r64, r32 = ref_fanout(case, 'float64'), ref_fanout(case, 'float32')
    res = run_fanout(A, ctx, case)
    MM.check(as_res(res, r64, r32, case), BARS)
    poisoned = dict(case, target=case['target'].copy())
    poisoned['target'][:, bs < 1e-5] = np.nan
    res_nan = run_fanout(A, ctx, poisoned)
    for k in ('loss', 'grad', 'gprobe'):
        assert np.array_equal(np.asarray(res[k]), np.asarray(res_nan[k])), k
    assert np.array_equal(res['pred'], res_nan['pred']) and np.isfinite(res_nan['loss'])


def test_poisson_loss(A, ctx):
    case = make_case((40, 24), S=2, B=3, M=1, D=2, seed=12, loss='poisson', poisson_multiplier=50.)
    r64, r32 = ref_fanout(case, 'float64'), ref_fanout(case, 'float32')
    res = as_res(run_fanout(A, ctx, case), r64, r32, case)
    report(res, 'poisson')
    MM.check(res, BARS)


# ------------------------------------------------------------------------------------------ 5. refusals
def test_engine_refusals(A, ctx):
    case = make_case((24, 20), D=2)
    for kw, name in ((dict(exit_shift=True), 'exit_shift'), (dict(probe_shift=True), 'probe_shift'),
                     (dict(slice_pos_cm=[0., 1e-4]), 'slice_pos_cm')):
        with pytest.raises(NotImplementedError, match='detector_fanout together with %s' % name):
            _engine(A, ctx, case, case['dists'], **kw)
    for fp in ('inf', 0, None, 2e-4, [2e-4]):
        with pytest.raises(ValueError, match='detector_fanout needs a sequence of at least two detector distances'):
            _engine(A, ctx, case, fp)
    with pytest.raises(NotImplementedError, match='detector_fanout needs the streamed plan'):
        A.MultisliceEngine(ctx, (33, 33, 2), (24, 20), case['pos'], ENERGY_EV, PSIZE_CM, free_prop_cm=case['dists'], streamed=False,
                           detector_fanout=True)
    eng = _engine(A, ctx, case, case['dists'])
    eng.set_batch(case['pos'], case['target'])
    probe = ctx.array(MM.c2(case['probes']))
    with pytest.raises(NotImplementedError, match='detector_fanout together with shifts'):
        eng.multislice(probe, shifts=ctx.zeros((3, 2)))
    with pytest.raises(NotImplementedError, match='detector_fanout together with probes_b'):
        eng.multislice(None, probes_b=ctx.zeros((3, 1, 24, 20, 2)))
    with pytest.raises(ValueError, match='set_batch: targets must hold 6 x 24 x 20'):
        eng.set_batch(case['pos'], case['target'][:3])
    eng.plan.close()
    # without detector_fanout a sequence of distances on a streamed engine is refused as it always was
    with pytest.raises(NotImplementedError, match='per position'):
        _engine(A, ctx, case, case['dists'], fanout=False)


def test_abi_refusals(A, ctx):
    from adorym_amd._lib import check
    case = make_case((24, 20), D=2)
    k = [np.ones((24, 20), complex)] * 2
    re, im = np.ones((2, 24, 20), np.float32), np.zeros((2, 24, 20), np.float32)
    lds = A.MultisliceEngine(ctx, (33, 33, 2), (24, 20), case['pos'], ENERGY_EV, PSIZE_CM, free_prop_cm=2e-4)
    with pytest.raises(NotImplementedError, match='adm_plan_set_detector_fanout: a detector fan-out needs a streamed plan'):
        lds.plan.set_detector_fanout(k)
    lds.plan.close()
    far = A.MultisliceEngine(ctx, (33, 33, 2), (24, 20), case['pos'], ENERGY_EV, PSIZE_CM, streamed=True)
    with pytest.raises(ValueError, match='adm_plan_set_detector_fanout: the plan.s det_mode is not ADM_DET_FRESNEL'):
        far.plan.set_detector_fanout(k)
    far.plan.close()
    for kw, what in ((dict(exit_shift=True), 'exit-wave shifts'), (dict(probe_shift=True), 'probe shifts'),
                     (dict(slice_pos_cm=[0., 1e-4]), 'slice positions')):
        eng = A.MultisliceEngine(ctx, (33, 33, 2), (24, 20), case['pos'], ENERGY_EV, PSIZE_CM, free_prop_cm=2e-4, streamed=True, **kw)
        with pytest.raises(NotImplementedError, match='adm_plan_set_detector_fanout: a detector fan-out on a plan with %s' % what):
            eng.plan.set_detector_fanout(k)
        eng.plan.close()
    eng = _engine(A, ctx, case, case['dists'])
    lib, h = ctx.lib, eng.plan.handle
    for n in (-1, 65):
        with pytest.raises(ValueError, match='adm_plan_set_detector_fanout: n must be in'):
            check(lib.adm_plan_set_detector_fanout(h, n, re.ctypes.data, im.ctypes.data))
    with pytest.raises(ValueError, match='adm_plan_set_detector_fanout: null kernels'):
        check(lib.adm_plan_set_detector_fanout(h, 2, None, None))
    # ... and the other setters refuse a plan with a fan-out
    with pytest.raises(NotImplementedError, match='adm_plan_set_exit_shift: exit-wave shifts on a plan with a detector fan-out'):
        check(lib.adm_plan_set_exit_shift(h, 1))
    with pytest.raises(NotImplementedError, match='adm_plan_set_probe_shift: probe shifts on a plan with a detector fan-out'):
        check(lib.adm_plan_set_probe_shift(h, 1))
    z = ctx.zeros((2,))
    with pytest.raises(NotImplementedError, match='adm_plan_set_slice_positions: slice positions together with a detector fan-out'):
        check(lib.adm_plan_set_slice_positions(h, z.ptr, 2, 0.155, 10., 10.))
    check(lib.adm_plan_set_detector_fanout(h, 0, None, None))          # off again: the plain Fresnel plan
    check(lib.adm_plan_set_exit_shift(h, 1))
    eng.plan.close()
