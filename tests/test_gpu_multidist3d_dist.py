"""The distances of the detector fan-out as parameters on the GPU (pytest -m gpu): the gradient instantiations of adm_ms_multidist.hip through the engine
(MultisliceEngine(detector_fanout=True, refine_distances=True), multislice(grad_dists=...)) and the C ABI
(adm_plan_set_fanout_distances, adm_multislice_fwd_adj_fanout_dist) as the engine calls it.

Checkers: golden F28 (recorded from the reference with optimize_free_prop, tests/golden/gen_f28_multidist3d_dist.py) and the NumPy
restatement tests/multidist3d_dist_ref.py (tied to the reference by tests/test_multidist3d_dist_ref_vs_golden.py), which takes the
distances rounded to float32 as the engine holds them.  Prediction, loss, object and probe gradients: ms_matrix.GENERIC.  dL/dd
against the reference: e <= 3 * (the reference's own fp32 distance from its fp64 run) + floor, floor = the fp32 restatement's own
distance from fp64 (test_gpu_sparse_multislice.py:check_3x's rule); against the restatement: e <= 3 * (the fp32 restatement's
distance) + GENERIC['grad_abs'] under the cap GENERIC['grad'], the rule the object gradient has in this matrix.
"""
import ast
import os

import numpy as np
import pytest

from tests import ms_matrix as MM
from tests import fan_matrix as FM
from tests import multidist3d_dist_ref as DR
from tests import test_gpu_multidist3d as MD
from oracle import adorym_oracle as O      # checker only

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENERGY_EV, PSIZE_CM = MD.ENERGY_EV, MD.PSIZE_CM
BARS = MM.GENERIC
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
    return np.load(os.path.join(ROOT, 'tests', 'golden', 'F28_multidist3d_dist.npz'))


def round32(dists):
    return [float(np.float32(d)) for d in dists]


def refine_engine(A, ctx, case, **engine_kw):
    eng = MD._engine(A, ctx, case, case['dists'], refine_distances=True, **engine_kw)
    assert eng.streamed is True and eng.refine_distances and eng.dists.shape == (len(case['dists']),) and eng.dists.dtype == np.float32
    assert np.array_equal(eng.dists.get(), np.asarray(case['dists'], np.float32))
    return eng


def launch(ctx, eng, case, want_dists=True, gd=None):
    """MD.launch with the distance gradient: 'gdists' is the buffer ``gd`` (default: a zeroed one) as the launch left it."""
    obj, pos, probes = case['obj'], case['pos'], case['probes']
    M, Py, Px = probes.shape
    d_grad, d_gp = ctx.zeros(obj.shape), ctx.zeros((M, Py, Px, 2))
    if gd is None:
        gd = ctx.zeros((len(case['dists']),))
    eng.set_batch(pos, np.asarray(case['target'], np.float32))
    eng.rotate(ctx.array(obj, np.float32), None)
    eng.multislice(ctx.array(MM.c2(probes)), grad_probe=d_gp, want_pred=True, grad_dists=gd if want_dists else None)
    eng.rotate_adjoint(d_grad, None)
    return dict(grad=d_grad.get(), gprobe=MM.cplx(d_gp.get()), pred=eng.pred(), loss=eng.loss(), gdists=gd.get().astype(np.float64),
                n_rounds=len(eng.rounds(len(pos))))


def run_refine(A, ctx, case, **engine_kw):
    eng = refine_engine(A, ctx, case, **engine_kw)
    out = launch(ctx, eng, case)
    eng.plan.close()
    return out


def ref_dists(case, dtype):
    """loss, pred, dL/dd, per-field terms of the restatement"""
    phys = O.Physics(case['probes'].shape[-2:], ENERGY_EV, PSIZE_CM, free_prop_cm=case['dists'][0], sign_convention=case['sign_convention'])
    return DR.forward_dist_grad_object(case['obj'].astype(np.float64), None, case['probes'].astype(np.complex128), case['pos'], case['meas'],
                                       phys, case['dists'], dtype, raw_data_type=case.get('raw_data_type', 'magnitude'))


# ------------------------------------------------------------------------------------------- 1. the fixture's cases (the reference)
def fixture_case(F, name):
    names = [str(n) for n in F['kernel_cases']]
    sg, M, rdt = ast.literal_eval(str(F['kernel_case_params'][names.index(name)]))
    c = {k: F['%s/%s' % (name, k)] for k in ('obj', 'pos', 'probes', 'meas')}
    c.update(sign_convention=sg, raw_data_type=rdt, dists=[float(d) for d in F['kernel_dists_cm']])
    c['target'] = O.target_magnitude(c['meas'], rdt)
    return c


@pytest.mark.parametrize('name', MD.FIXTURE_CASES)
def test_kernels_vs_reference(A, ctx, F, name):
    """st_fresnel_table_kernel, md_fanout_kernel<true>, md_fanin_kernel<true>, st_dd_reduce_kernel: prediction, loss, object gradient, probe gradient and
    dL/d free_prop_cm against the reference's fp64 run with optimize_free_prop (field 12 x 20, S = 5, D = 3, the model's distances
    off the data's by 10 %, -8 %, 5 %; one and two modes, both sign conventions, magnitude and intensity data)."""
    case = fixture_case(F, name)
    res = run_refine(A, ctx, case)
    e32 = F[name + '/err32']
    e = rel(res['pred'], F[name + '/pred'])
    print(name, 'pred %.2e (fp32 ref %.2e)' % (e, e32[0]))
    assert e < BARS['pred'], ('pred', e)
    e = abs(res['loss'] / float(F[name + '/loss']) - 1)
    print(name, 'loss %.2e (fp32 ref %.2e)' % (e, e32[1]))
    assert e <= BARS['loss'], ('loss', e)
    for k, i in (('grad', 2), ('gprobe', 3)):
        e = rel(res[k], F['%s/%s' % (name, k)])
        print(name, '%s %.2e (fp32 ref %.2e)' % (k, e, e32[i]))
        assert e < BARS['grad'] and e <= 3 * e32[i] + BARS['grad_abs'], (k, e, e32[i])
    gd64, gd32 = ref_dists(case, 'float64')[2], ref_dists(case, 'float32')[2]
    floor = rel(gd32, gd64)
    e = rel(res['gdists'], F[name + '/gdists'])
    print(name, 'dL/dd %.2e (fp32 ref %.2e, fp32 restatement %.2e)' % (e, e32[4], floor), res['gdists'], F[name + '/gdists'])
    assert e <= 3 * e32[4] + floor, ('dL/dd', e, e32[4], floor)


# --------------------------------------------------------------------------------- 2. launch geometries (the restatement)
#   name: fan_matrix.make_case arguments (the field 24 x 20 = fan_matrix.FIELD unless P says otherwise)
GEOMETRIES = {
    '12x20_groups_8_8_4': dict(P=(12, 20), B=3, D=3, M=1),                    # column groups 8, 8, 4: the last one clipped
    '24x20_D64': dict(B=3, D=64, M=1),
    '1025x12_cw4': dict(P=FM.TALL, B=2, D=3, M=1),                            # column width 4, the 1024 / 1025 boundary
    'M2': dict(B=3, D=2, M=2),
    'M4_D3': dict(B=3, D=3, M=4),
    'B85_255_partials': dict(B=85, D=2, M=1),                                 # B * M * ncg = 255: below st_dd_reduce_kernel's stride
    'B86_258_partials': dict(B=86, D=2, M=1),                                 # ... and 258: above it
    'sigma_m1': dict(B=3, D=3, M=2, sign_convention=-1),
    'repeated': dict(B=3, D=3, M=2, dists=FM.DISTANCE_SETS['repeated']),
    'aliased': dict(B=3, D=3, M=2, dists=FM.DISTANCE_SETS['aliased']),
}
_BUILT = {}


def built(name, **kw):
    """The case and the restatement's results on it (fp64 and fp32; the fan-out's own quantities through MD.ref_fanout), computed
    once per process and left unchanged."""
    if name not in _BUILT:
        kw = dict(kw)
        D = kw['D']
        kw['dists'] = round32(kw.get('dists') or FM.default_dists(D))        # float32-representable: every path sees the same values
        case = FM.make_case(**kw)
        r64, r32 = MD.ref_fanout(case, 'float64'), MD.ref_fanout(case, 'float32')
        d64, d32 = ref_dists(case, 'float64'), ref_dists(case, 'float32')
        assert rel(d64[1], r64['pred']) < 1e-12 and abs(d64[0] / r64['loss'] - 1) < 1e-12       # one model, stated twice
        _BUILT[name] = (case, r64, r32, d64[2], d32[2])
    return _BUILT[name]


def check_dists(res, gd64, gd32, what):
    e, e32 = rel(res['gdists'], gd64), rel(gd32, gd64)
    print(what, 'dL/dd %.2e (fp32 restatement %.2e)' % (e, e32), res['gdists'][:4], gd64[:4])
    assert np.all(np.isfinite(res['gdists'])) and e < BARS['grad'] and e <= 3 * e32 + BARS['grad_abs'], (what, 'dL/dd', e, e32)


def test_the_geometries_sit_on_both_sides_of_the_reduce_stride():
    ncg = -(-FM.FIELD[1] // 8)
    assert 85 * ncg == 255 and 86 * ncg == 258 and (12, 20) == GEOMETRIES['12x20_groups_8_8_4']['P'] and FM.TALL == (1025, 12)
    assert FM.DISTANCE_SETS['repeated'][0] == FM.DISTANCE_SETS['repeated'][1]
    assert any(FM.phase_step_at_nyquist(z, FM.FIELD) > 1 for z in FM.DISTANCE_SETS['aliased'])


@pytest.mark.parametrize('name', list(GEOMETRIES))
def test_geometries_vs_restatement(A, ctx, name):
    """md_fanout_kernel<true>, md_fanin_kernel<true>, st_dd_reduce_kernel over the column geometries (clipped last group, cw = 4 at 1025 rows), the
    fan-out limit D = 64, one to four modes, both sides of the reduce kernel's stride of 256 partials, sigma = -1, a repeated
    distance and an aliased set: dL/dd against the fp64 restatement, and prediction, loss, object and probe gradients as the
    fan-out tests judge them."""
    case, r64, r32, gd64, gd32 = built(name, **GEOMETRIES[name])
    res = run_refine(A, ctx, case)
    MM.check(MD.as_res(res, r64, r32, case), BARS)
    check_dists(res, gd64, gd32, name)


def test_rounds_add_up(A, ctx):
    """B = 7, D = 3, M = 2 forced into three rounds (3, 2, 2 positions) by the workspace budget: every round adds its share."""
    name = 'rounds_B7_D3_M2'
    B, D, M, cap, split = FM.ROUNDS[name]
    case, r64, r32, gd64, gd32 = built(name, B=B, D=D, M=M)
    probe_eng = refine_engine(A, ctx, case)
    one, budget = probe_eng.plan.workspace_bytes(1), probe_eng.plan.workspace_bytes(cap)
    assert probe_eng.plan.workspace_bytes(3) - one == 2 * (probe_eng.plan.workspace_bytes(2) - one)       # linear in the batch
    whole = launch(ctx, probe_eng, case)
    probe_eng.plan.close()
    eng = refine_engine(A, ctx, case, workspace_budget=budget)
    assert [n for _, n in eng.rounds(B)] == split
    parts = launch(ctx, eng, case)
    eng.plan.close()
    assert whole['n_rounds'] == 1 and parts['n_rounds'] == 3
    MM.check(MD.as_res(parts, r64, r32, case), BARS)
    check_dists(parts, gd64, gd32, name)
    assert parts['loss'] == whole['loss'] and np.array_equal(parts['pred'], whole['pred'])
    assert rel(parts['gdists'], whole['gdists']) < 1e-6          # (float32 accumulation of three shares against one)


def test_workspace_grows_by_the_kept_spectra_and_the_partials(A, ctx):
    case = built('M2', **GEOMETRIES['M2'])[0]
    plain, ref = MD._engine(A, ctx, case, case['dists']), refine_engine(A, ctx, case)
    Py, Px = FM.FIELD
    B, D, M, ncg = 5, 2, 2, -(-Px // 8)
    assert ref.plan.workspace_bytes(B) - plain.plan.workspace_bytes(B) == B * M * Py * Px * 8 + D * B * M * ncg * 8
    plain.plan.close(), ref.plan.close()


# ------------------------------------------------------------------------------------------ 3. bit for bit
def test_the_request_changes_no_other_bit(A, ctx):
    """On one refine_distances engine: a launch with grad_dists and one without give identical prediction, loss, object and probe
    gradients (and the buffer stays zero when not requested); the same launch twice gives identical bits, dL/dd included; a second
    launch into the same buffer gives exactly twice the first (+=)."""
    case = built('M2', **GEOMETRIES['M2'])[0]
    eng = refine_engine(A, ctx, case)
    a = launch(ctx, eng, case)
    off = launch(ctx, eng, case, want_dists=False)
    b = launch(ctx, eng, case)
    for k in ('pred', 'loss', 'grad', 'gprobe'):
        assert np.array_equal(np.asarray(a[k]), np.asarray(off[k])), k
        assert np.array_equal(np.asarray(a[k]), np.asarray(b[k])), k
    assert np.all(off['gdists'] == 0) and np.all(a['gdists'] != 0)
    assert np.array_equal(a['gdists'], b['gdists'])
    gd = ctx.zeros((len(case['dists']),))
    launch(ctx, eng, case, gd=gd)
    twice = launch(ctx, eng, case, gd=gd)
    assert np.array_equal(twice['gdists'], 2 * a['gdists'])
    eng.plan.close()


# ------------------------------------------------------------------------------------------ 4. the table on the device
def test_device_table_agrees_with_host_table(A, ctx):
    """The predictions of a refine_distances engine against those of a host-table engine at the same float32-representable
    distances, under the prediction bar; the aliased set too (phases of hundreds of radians)."""
    for name in ('M2', 'aliased'):
        case = built(name, **GEOMETRIES[name])[0]
        host = MD.run_fanout(A, ctx, case)
        dev = run_refine(A, ctx, case)
        e = rel(dev['pred'], host['pred'])
        print(name, 'device table vs host table: pred %.2e' % e)
        assert e < BARS['pred'], (name, e)


def test_changed_distances_rebuild_the_table(A, ctx):
    """st_fresnel_table_kernel: after dists.set(new) + dists_changed() the predictions are those of a fresh engine built at ``new``, bit
    for bit; the distances the engine was built with are gone."""
    case = built('M2', **GEOMETRIES['M2'])[0]
    new = round32([1.3 * d for d in case['dists']])
    eng = refine_engine(A, ctx, case)
    before = launch(ctx, eng, case)
    eng.dists.set(np.asarray(new, np.float32))
    eng.dists_changed()
    after = launch(ctx, eng, case)
    eng.plan.close()
    fresh = run_refine(A, ctx, dict(case, dists=new))
    for k in ('pred', 'loss', 'grad', 'gprobe', 'gdists'):
        assert np.array_equal(np.asarray(after[k]), np.asarray(fresh[k])), k
    assert rel(after['pred'], before['pred']) > 1e-3


# ------------------------------------------------------------------------------------------ 5. refusals
def test_engine_refusals(A, ctx):
    case = built('M2', **GEOMETRIES['M2'])[0]
    with pytest.raises(ValueError, match='refine_distances needs detector_fanout=True'):
        A.MultisliceEngine(ctx, (33, 33, 2), FM.FIELD, case['pos'], ENERGY_EV, PSIZE_CM, free_prop_cm=2e-4, streamed=True, refine_distances=True)
    eng = MD._engine(A, ctx, case, case['dists'])
    assert eng.dists is None
    eng.set_batch(case['pos'], case['target'])
    with pytest.raises(ValueError, match='grad_dists: the engine was built without refine_distances'):
        eng.multislice(ctx.array(MM.c2(case['probes'])), grad_dists=ctx.zeros((2,)))
    with pytest.raises(ValueError, match='dists_changed: the engine was built without refine_distances'):
        eng.dists_changed()
    eng.plan.close()
    eng = refine_engine(A, ctx, case)
    eng.set_batch(case['pos'], case['target'])
    with pytest.raises(ValueError, match=r'grad_dists must be float32 \[2\]'):
        eng.multislice(ctx.array(MM.c2(case['probes'])), grad_dists=ctx.zeros((3,)))
    eng.plan.close()


def test_abi_refusals(A, ctx):
    from adorym_amd._lib import check
    case = built('M2', **GEOMETRIES['M2'])[0]
    lib = ctx.lib
    d = ctx.array(np.asarray(case['dists'], np.float32))
    geo = (0.155, 10., 10.)
    lds = A.MultisliceEngine(ctx, (33, 33, 2), FM.FIELD, case['pos'], ENERGY_EV, PSIZE_CM, free_prop_cm=2e-4)
    with pytest.raises(NotImplementedError, match='adm_plan_set_fanout_distances: a detector fan-out needs a streamed plan'):
        check(lib.adm_plan_set_fanout_distances(lds.plan.handle, d.ptr, 2, *geo))
    lds.plan.close()
    far = A.MultisliceEngine(ctx, (33, 33, 2), FM.FIELD, case['pos'], ENERGY_EV, PSIZE_CM, streamed=True)
    with pytest.raises(ValueError, match='adm_plan_set_fanout_distances: the plan.s det_mode is not ADM_DET_FRESNEL'):
        check(lib.adm_plan_set_fanout_distances(far.plan.handle, d.ptr, 2, *geo))
    far.plan.close()
    for kw, what in ((dict(exit_shift=True), 'exit-wave shifts'), (dict(probe_shift=True), 'probe shifts'),
                     (dict(slice_pos_cm=[0., 1e-4]), 'slice positions')):
        eng = A.MultisliceEngine(ctx, (33, 33, 2), FM.FIELD, case['pos'], ENERGY_EV, PSIZE_CM, free_prop_cm=2e-4, streamed=True, **kw)
        with pytest.raises(NotImplementedError, match='adm_plan_set_fanout_distances: a detector fan-out on a plan with %s' % what):
            check(lib.adm_plan_set_fanout_distances(eng.plan.handle, d.ptr, 2, *geo))
        eng.plan.close()
    # a host-table fan-out has no distances to differentiate
    host = MD._engine(A, ctx, case, case['dists'])
    host.set_batch(case['pos'], case['target'])
    host.rotate(ctx.array(case['obj'], np.float32), None)
    args = host._ms_args(ctx.array(MM.c2(case['probes'])), None, True, False, 1., 0, len(case['pos']), host._ws)
    with pytest.raises(ValueError, match='adm_multislice_fwd_adj_fanout_dist: the plan has no fan-out distances'):
        check(lib.adm_multislice_fwd_adj_fanout_dist(*(args + (ctx.zeros((2,)).ptr,))))
    host.plan.close()
    eng = refine_engine(A, ctx, case)
    h = eng.plan.handle
    for n in (0, -1, 65):
        with pytest.raises(ValueError, match='adm_plan_set_fanout_distances: n must be in'):
            check(lib.adm_plan_set_fanout_distances(h, d.ptr, n, *geo))
    with pytest.raises(ValueError, match='adm_plan_set_fanout_distances: null distances'):
        check(lib.adm_plan_set_fanout_distances(h, None, 2, *geo))
    with pytest.raises(ValueError, match='adm_plan_set_fanout_distances: wavelength and voxel sizes must be positive'):
        check(lib.adm_plan_set_fanout_distances(h, d.ptr, 2, 0., 10., 10.))
    # ... and the other setters refuse a plan that has them
    with pytest.raises(NotImplementedError, match='adm_plan_set_exit_shift: exit-wave shifts on a plan with a detector fan-out'):
        check(lib.adm_plan_set_exit_shift(h, 1))
    with pytest.raises(NotImplementedError, match='adm_plan_set_probe_shift: probe shifts on a plan with a detector fan-out'):
        check(lib.adm_plan_set_probe_shift(h, 1))
    z = ctx.zeros((2,))
    with pytest.raises(NotImplementedError, match='adm_plan_set_slice_positions: slice positions together with a detector fan-out'):
        check(lib.adm_plan_set_slice_positions(h, z.ptr, 2, *geo))
    eng.plan.close()
