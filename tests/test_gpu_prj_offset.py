"""Per-angle projection alignment on the GPU (pytest -m gpu): the detector-step kernels that Fourier-shift the exit wave by one
offset per position and form dL/d offset (adm_ms_exitshift.hip), through the C ABI (adm_plan_set_exit_shift,
adm_multislice_fwd_adj_exit_shift) as the engine calls it.

Checkers: golden F24 (recorded from the reference, tests/golden/gen_f24_prj_offset.py) and the NumPy restatement
tests/prj_offset_ref.py (tied to the reference by tests/test_prj_offset_ref_vs_golden.py).  Prediction, loss, object and probe
gradients: the bars tests/ms_matrix.py:check applies with GENERIC.  Shift gradient: at most three times the distance of the
checker's own fp32 run from fp64, plus 2^-24 (the buffer is fp32).
"""
import ast
import os

import numpy as np
import pytest

from tests import ms_matrix as MM
from tests import prj_offset_ref as PR
from oracle import adorym_oracle as O      # checker only

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENERGY_EV, PSIZE_CM = 8000., 1e-6
BARS = MM.GENERIC
FREE_PROP_CM = 2e-4
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
    return np.load(os.path.join(ROOT, 'tests', 'golden', 'F24_prj_offset.npz'))


def run_shifted(A, ctx, case, want_gs=True, gs_init=None, keep_engine=False, canaries=False, **engine_kw):
    """rotate -> multislice(exit_shifts=...) -> rotate_adjoint of an engine built with exit_shift=True.  ``case``: obj [Y,X,S,2],
    pos, probes [M,Py,Px] complex, shifts [n,2], index [B] or None, meas [B,Py,Px], unknown_type, free_prop, sign_convention.
    ``canaries``: shifts and the gradient buffer are views into larger arrays whose surroundings must come back untouched."""
    obj, pos, probes, meas = [case[k] for k in ('obj', 'pos', 'probes', 'meas')]
    shifts = np.ascontiguousarray(case['shifts'], np.float32)
    M, Py, Px = probes.shape
    Y, X, S = obj.shape[:3]
    B, n = len(pos), len(shifts)
    eng = A.MultisliceEngine(ctx, (Y, X, S), (Py, Px), pos, ENERGY_EV, PSIZE_CM, free_prop_cm=case['free_prop'],
                             sign_convention=case['sign_convention'], n_probe_modes=M, max_batch=B, unknown_type=case['unknown_type'],
                             exit_shift=True, **engine_kw)
    assert eng.streamed is True
    d_grad, d_gp = ctx.zeros(obj.shape), ctx.zeros((M, Py, Px, 2))
    pad = 3 if canaries else 0
    host_s = np.full((n + 2 * pad, 2), 1e30, np.float32)             # (an offset read from the surroundings would wreck everything)
    host_s[pad:pad + n] = shifts
    host_g = np.full((n + 2 * pad, 2), -7.25, np.float32)
    host_g[pad:pad + n] = 0 if gs_init is None else gs_init
    all_s, all_g = ctx.array(host_s), ctx.array(host_g)
    d_s, d_gs = all_s.view(2 * pad, (n, 2)), all_g.view(2 * pad, (n, 2))
    d_idx = ctx.array(np.ascontiguousarray(case['index'], np.int32)) if case.get('index') is not None else None
    eng.set_batch(pos, np.asarray(meas, np.float32))
    eng.rotate(ctx.array(obj, np.float32), None)
    eng.multislice(ctx.array(MM.c2(probes)), grad_probe=d_gp, want_pred=True, exit_shifts=d_s, exit_shift_index=d_idx,
                   grad_exit_shifts=d_gs if want_gs else None)
    eng.rotate_adjoint(d_grad, None)
    g_all = all_g.get()
    out = dict(pred=eng.pred(), loss=eng.loss(), grad=d_grad.get(), gprobe=MM.cplx(d_gp.get()), gs_raw=g_all[pad:pad + n].copy(),
               gs=g_all[pad:pad + n].astype(np.float64), n_rounds=len(eng.rounds(B)))
    if canaries:
        assert np.array_equal(all_s.get(), host_s)
        assert np.all(g_all[:pad] == -7.25) and np.all(g_all[pad + n:] == -7.25)
    if keep_engine:
        out['engine'] = eng
    else:
        eng.plan.close()
    return out


def ref_shifted(case, dtype):
    phys = O.Physics(case['probes'].shape[-2:], ENERGY_EV, PSIZE_CM, free_prop_cm=case['free_prop'], sign_convention=case['sign_convention'],
                     unknown_type=case['unknown_type'])
    l, p, g, gp, gs = PR.forward_adjoint_object(case['obj'].astype(np.float64), None, case['probes'].astype(np.complex128), case['pos'],
                                                case['meas'], phys, np.asarray(case['shifts'], np.float64), case.get('index'), dtype)
    return dict(loss=l, pred=p, grad=g, gprobe=gp, gs=gs)


def gs_bar(e32):
    return 3 * e32 + 2. ** -24


def check_3x(res, r64, e32, what=''):
    """``e32``: the fp32 yardstick's distances from fp64 (pred, loss, grad, gprobe, gs, gprobe per mode ...).  Every figure is
    printed before it is held to its bar."""
    e = rel(res['pred'], r64['pred'])
    per = max(rel(p, po) for p, po in zip(res['pred'], r64['pred']))
    print(what, 'pred %.2e, worst position %.2e (fp32 ref %.2e)' % (e, per, e32[0]))
    assert e < BARS['pred'] and per < BARS['pred'], ('pred', e, per)
    e = abs(res['loss'] / r64['loss'] - 1)
    print(what, 'loss %.2e (fp32 ref %.2e)' % (e, e32[1]))
    assert e <= BARS['loss'], ('loss', e)
    e = rel(res['grad'], r64['grad'])
    print(what, 'grad %.2e (fp32 ref %.2e)' % (e, e32[2]))
    assert e < BARS['grad'] and e <= 3 * e32[2] + BARS['grad_abs'], ('object gradient', e, e32[2])
    e = rel(res['gprobe'], r64['gprobe'])
    print(what, 'gprobe %.2e (fp32 ref %.2e)' % (e, e32[3]))
    assert e < BARS['grad'], ('probe gradient', e)
    e = rel(res['gs'], r64['gs'])
    print(what, 'dL/ds %.2e (fp32 ref %.2e, bar %.2e)' % (e, e32[4], gs_bar(e32[4])), res['gs'].ravel(), np.asarray(r64['gs']).ravel())
    assert e <= gs_bar(e32[4]), ('dL/ds', e, e32[4], res['gs'], r64['gs'])


# ------------------------------------------------------------------------------------------- 1. the fixture's cases (the reference)
FIXTURE_CASES = ['s3_fresnel_p1', 's3_fresnel_m1_modes2', 's1_fresnel', 's3_exit_wave', 's3_fresnel_real_imag']


def fixture_case(F, name):
    names = [str(n) for n in F['kernel_cases']]
    S, unknown, free_prop, sg, M = ast.literal_eval(str(F['kernel_case_params'][names.index(name)]))
    c = {k: F['%s/%s' % (name, k)] for k in ('obj', 'pos', 'probes', 'shifts', 'index', 'meas')}
    c.update(unknown_type=unknown, free_prop=free_prop if free_prop is not None else 0, sign_convention=sg)
    return c


@pytest.mark.parametrize('name', FIXTURE_CASES)
def test_kernels_vs_reference(A, ctx, F, name):
    """es_col_conv_kernel<false>, es_col_conv_kernel<true>, st_shift_reduce_kernel: prediction, loss, object gradient, probe gradient and
    dL/ds against the reference's fp64 run, the reference's own fp32 run as the yardstick."""
    case = fixture_case(F, name)
    res = run_shifted(A, ctx, case, canaries=True)
    r64 = {k: F['%s/%s' % (name, k)] for k in ('pred', 'grad', 'gprobe', 'gs')}
    r64['loss'] = float(F[name + '/loss'])
    check_3x(res, r64, F[name + '/err32'], name)


def test_far_field_leaves_the_gradient_buffer_alone(A, ctx, F):
    """A far-field magnitude does not see the offsets: the launch is the plain one, the prediction is the reference's, and the
    gradient buffer comes back bit-unchanged."""
    name = 's3_far_field'
    case = fixture_case(F, name)
    init = np.arange(8, dtype=np.float32).reshape(4, 2) * 0.3 - 1
    res = run_shifted(A, ctx, case, gs_init=init, canaries=True)
    assert np.array_equal(res['gs_raw'], init)
    assert rel(res['pred'], F[name + '/pred']) < BARS['pred'] and abs(res['loss'] / float(F[name + '/loss']) - 1) <= BARS['loss']
    e = rel(res['grad'], F[name + '/grad'])
    assert e < BARS['grad'] and e <= 3 * F[name + '/err32'][2] + BARS['grad_abs']
    assert rel(res['gprobe'], F[name + '/gprobe']) < BARS['grad']


# --------------------------------------------------------------------------------- 2. launch geometries (the restatement)
def make_case(P, S=2, B=5, M=1, shared=False, unknown_type='delta_beta', free_prop=FREE_PROP_CM, sign_convention=1, seed=0, shifts_fn=None):
    """Built like ms_matrix.oracle_case: positions hanging over all four edges, a truth with ten times the guess's contrast and
    other offsets makes the data.  ``shifts_fn(n) -> [n, 2]``: offsets in place of the ones drawn within 2 px."""
    Py, Px = (P, P) if np.isscalar(P) else tuple(P)
    r = np.random.default_rng([Py, Px, S, B, M, seed])
    Y, X = Py + 9, Px + 13
    if unknown_type == 'delta_beta':
        mk = lambda c: np.stack([2e-3 * c * r.uniform(size=(Y, X, S)), 2e-4 * c * r.uniform(size=(Y, X, S))], -1)
    else:           # (a transmission near 1, as make_case of test_gpu_sparse_multislice.py)
        mk = lambda c: np.stack([1 + 1e-2 * c * r.standard_normal((Y, X, S)), 2e-2 * c * r.standard_normal((Y, X, S))], -1)
    obj, truth = mk(1).astype(np.float32), mk(10).astype(np.float32)
    pos = MM.edge_positions(r, B, Y, X, Py, Px)
    probes = ((0.5 + r.uniform(0, 1, (M, Py, Px))) * np.exp(1j * r.uniform(-np.pi, np.pi, (M, Py, Px)))).astype(np.complex64)
    index = np.array([0, 1, 2, 1, 0][:B], np.int32) if shared else None
    n = 3 if shared else B
    shifts = r.uniform(-2, 2, (n, 2)).astype(np.float32)
    if shifts_fn is not None:
        shifts = np.asarray(shifts_fn(n), np.float32)
    phys = O.Physics((Py, Px), ENERGY_EV, PSIZE_CM, free_prop_cm=free_prop, sign_convention=sign_convention, unknown_type=unknown_type)
    tiles, _ = O.extract_tiles(truth.astype(np.float64), pos, (Py, Px), unknown_type)
    meas = PR.predict(tiles, probes.astype(np.complex128), phys, shifts.astype(np.float64) + r.uniform(-0.3, 0.3, (n, 2)), index)
    return dict(obj=obj, pos=pos, probes=probes, shifts=shifts, index=index, meas=meas.astype(np.float32), unknown_type=unknown_type,
                free_prop=free_prop, sign_convention=sign_convention)


def yardstick(case):
    """The restatement in fp64 and the distances of its fp32 run, in the layout of the fixture's err32."""
    r64, r32 = ref_shifted(case, 'float64'), ref_shifted(case, 'float32')
    e32 = [rel(r32['pred'], r64['pred']), abs(r32['loss'] / r64['loss'] - 1), rel(r32['grad'], r64['grad']), rel(r32['gprobe'], r64['gprobe']),
           rel(r32['gs'], r64['gs'])]
    return r64, e32


GEOMETRIES = {
    '24x20': dict(P=(24, 20)),                       # 256 threads, last column group of 4
    '17x13_exit_wave': dict(P=(17, 13), free_prop=0),     # odd, prime sides; H = 1
    '135x21_modes2': dict(P=(135, 21), M=2),         # odd sides, several modes
    '640x12': dict(P=(640, 12)),                     # 320 threads, ragged last group
    '1025x6': dict(P=(1025, 6)),                     # cw = 4, last group of 2
}


@pytest.mark.parametrize('shared', [False, True], ids=['index_null', 'shared_entries'])
@pytest.mark.parametrize('name', list(GEOMETRIES))
def test_geometries_vs_restatement(A, ctx, name, shared):
    """es_col_conv_kernel<false>, es_col_conv_kernel<true>, st_shift_reduce_kernel at every column-launch geometry; S = 2, B = 5."""
    kw = dict(GEOMETRIES[name])
    case = make_case(kw.pop('P'), shared=shared, **kw)
    r64, e32 = yardstick(case)
    check_3x(run_shifted(A, ctx, case, canaries=True), r64, e32, name)


# ------------------------------------------------------------------------------------------ 3. semantics
def test_gradient_is_added_to_the_buffer(A, ctx):
    case = make_case((24, 20), shared=True, seed=1)
    init = np.array([[1.5, -2.], [0.25, 4.], [-8., 0.5]], np.float32)
    zero, added = run_shifted(A, ctx, case), run_shifted(A, ctx, case, gs_init=init, canaries=True)
    assert np.linalg.norm(zero['gs']) > 0
    assert np.array_equal(added['gs_raw'], init + zero['gs_raw'])            # (one fp32 addition per element either way)
    for k in ('pred', 'loss', 'grad', 'gprobe'):
        assert np.array_equal(np.asarray(zero[k]), np.asarray(added[k])), k


def test_two_launches_give_identical_bits(A, ctx):
    case = make_case((135, 21), M=2, shared=True, seed=2)
    a, b = run_shifted(A, ctx, case), run_shifted(A, ctx, case)
    for k in ('pred', 'loss', 'grad', 'gprobe', 'gs_raw'):
        assert np.array_equal(np.asarray(a[k]), np.asarray(b[k])), k


def test_no_shift_gradient_leaves_the_rest_unchanged(A, ctx):
    case = make_case((24, 20), M=2, seed=3)
    with_gs, without = run_shifted(A, ctx, case), run_shifted(A, ctx, case, want_gs=False)
    for k in ('pred', 'loss', 'grad', 'gprobe'):
        assert np.array_equal(np.asarray(with_gs[k]), np.asarray(without[k])), k
    assert np.all(without['gs'] == 0) and np.linalg.norm(with_gs['gs']) > 0


@pytest.mark.parametrize('free_prop', [FREE_PROP_CM, 0], ids=['fresnel', 'exit_wave'])
def test_zero_offsets_reproduce_the_plain_streamed_launch(A, ctx, free_prop):
    case = make_case((40, 24), M=2, free_prop=free_prop, seed=4)
    case['shifts'] = np.zeros_like(case['shifts'])
    res = run_shifted(A, ctx, case)
    obj, pos, probes, meas = [case[k] for k in ('obj', 'pos', 'probes', 'meas')]
    eng = A.MultisliceEngine(ctx, obj.shape[:3], probes.shape[1:], pos, ENERGY_EV, PSIZE_CM, free_prop_cm=free_prop, n_probe_modes=2,
                             max_batch=len(pos), streamed=True)
    eng.set_batch(pos, meas)
    eng.rotate(ctx.array(obj, np.float32), None)
    eng.multislice(ctx.array(MM.c2(probes)), want_pred=True)
    e = rel(res['pred'], eng.pred())
    print('zero offsets vs plain streamed launch: pred', e)
    assert e < 2e-6
    eng.plan.close()


def test_rounds_within_workspace_budget(A, ctx):
    """A batch split into rounds by the workspace budget: loss and prediction bit-identical, every round adds its share of dL/ds
    (inside the same 3x bar) -- with an index (entries shared across rounds) and without (every round its own entries)."""
    for shared in (True, False):
        case = make_case((135, 21), M=2, shared=shared, seed=5)
        one = run_shifted(A, ctx, case, keep_engine=True)
        budget = one['engine'].plan.workspace_bytes(2)
        one['engine'].plan.close()
        parts = run_shifted(A, ctx, case, workspace_budget=budget, canaries=True)
        assert one['n_rounds'] == 1 and parts['n_rounds'] == 3
        assert parts['loss'] == one['loss'] and np.array_equal(parts['pred'], one['pred'])
        r64, e32 = yardstick(case)
        check_3x(parts, r64, e32, 'rounds')
        assert rel(parts['gs'], one['gs']) <= gs_bar(e32[4])


def test_round_offsets_into_the_entries_and_into_the_index(A, ctx):
    """What a round starting at position o is handed: without an index the entries from o on (8 * o bytes into both tables), with
    one the index from o on (4 * o bytes) and the tables whole.  5 positions at 24 x 20 in 3 rounds against one launch, without
    an index and with a permutation: loss sums and predictions bit for bit, dL/ds inside the bar of the test above."""
    base = make_case((24, 20), seed=6)
    for index in (None, np.array([3, 0, 4, 1, 2], np.int32)):
        case = dict(base, index=index)
        one = run_shifted(A, ctx, case, keep_engine=True)
        eng = one['engine']
        budget, sums = eng.plan.workspace_bytes(2), eng._loss.view(0, (5,)).get()
        eng.plan.close()
        parts = run_shifted(A, ctx, case, workspace_budget=budget, canaries=True, keep_engine=True)
        assert one['n_rounds'] == 1 and parts['n_rounds'] == 3
        assert np.array_equal(parts['engine']._loss.view(0, (5,)).get(), sums) and np.all(sums > 0)
        parts['engine'].plan.close()
        assert parts['loss'] == one['loss'] and np.array_equal(parts['pred'], one['pred'])
        e32 = yardstick(case)[1]
        e = rel(parts['gs'], one['gs'])
        print('index' if index is not None else 'no index', 'rounds vs one launch: dL/ds %.2e (bar %.2e)' % (e, gs_bar(e32[4])))
        assert np.linalg.norm(one['gs']) > 0 and e <= gs_bar(e32[4])


def test_workspace_grows_by_the_kept_spectrum_and_stays_linear(A, ctx):
    from adorym_amd._lib import check
    for probe, M in (((256, 256), 1), ((1025, 132), 3), ((40, 24), 2)):
        obj = (probe[0] + 37, probe[1] + 20, 3)         # (odd and even frames)
        plain = A.Plan(ctx, obj, probe, ((0, 0), (0, 0)), 1.0, np.ones(probe, complex), n_modes=M, streamed=True)
        w0 = {b: plain.workspace_bytes(b) for b in (1, 2, 3, 7, 64, 300)}
        check(ctx.lib.adm_plan_set_exit_shift(plain.handle, 1))
        w1 = {b: plain.workspace_bytes(b) for b in (1, 2, 3, 7, 64, 300)}
        check(ctx.lib.adm_plan_set_exit_shift(plain.handle, 0))
        assert {b: plain.workspace_bytes(b) for b in w0} == w0                 # switched off: the sizes it always reported
        plain.close()
        for b in (3, 7, 64, 300):
            assert w1[b] == w1[1] + (b - 1) * (w1[2] - w1[1]), (probe, b)
        keep = M * probe[0] * probe[1] * 8
        for b in w0:
            assert w1[b] >= w0[b] + b * keep and w1[b] % 8 == 0, (probe, b)


# ------------------------------------------------------------------------------------------------------------ 4. refusals
def test_refusals(A, ctx):
    from adorym_amd._lib import check
    pos = np.array([(0, 0), (3, 5)])
    mk = lambda **kw: A.MultisliceEngine(ctx, (30, 30, 3), (24, 24), pos, ENERGY_EV, PSIZE_CM, max_batch=2, **kw)
    lds = mk()                                                   # a plan of adm_plan_create
    assert lds.streamed is False
    with pytest.raises(NotImplementedError, match='streamed plan'):
        check(ctx.lib.adm_plan_set_exit_shift(lds.plan.handle, 1))
    lds.set_batch(pos, np.ones((2, 24, 24), np.float32))
    s, probe = ctx.zeros((2, 2)), ctx.zeros((1, 24, 24, 2))
    with pytest.raises(NotImplementedError, match='streamed plan'):
        check(ctx.lib.adm_multislice_fwd_adj_exit_shift(lds.plan.handle, lds.obj_rot.ptr, probe.ptr, lds._cur_pos.ptr, 2, lds._cur_target.ptr,
                                                        1, None, None, lds._loss.ptr, 1.0, lds._ws.ptr, lds._ws.nbytes, s.ptr, None, None))
    with pytest.raises(ValueError, match='exit_shift=True'):
        lds.multislice(probe, exit_shifts=s)
    lds.plan.close()
    st = mk(streamed=True)                                       # streamed, not switched
    st.set_batch(pos, np.ones((2, 24, 24), np.float32))
    with pytest.raises(ValueError, match='adm_plan_set_exit_shift'):
        check(ctx.lib.adm_multislice_fwd_adj_exit_shift(st.plan.handle, st.obj_rot.ptr, probe.ptr, st._cur_pos.ptr, 2, st._cur_target.ptr,
                                                        1, None, None, st._loss.ptr, 1.0, st._ws.ptr, st._ws.nbytes, s.ptr, None, None))
    st.plan.close()
    sp = mk(slice_pos_cm=[0., 1e-3, 2e-3])                       # slice positions and exit shifts exclude each other, either order
    with pytest.raises(NotImplementedError, match='slice positions'):
        check(ctx.lib.adm_plan_set_exit_shift(sp.plan.handle, 1))
    sp.plan.close()
    xs = mk(exit_shift=True)
    assert xs.streamed is True
    z = ctx.array(np.array([0., 1e-3, 2e-3], np.float32))
    with pytest.raises(NotImplementedError, match='exit-wave shifts'):
        check(ctx.lib.adm_plan_set_slice_positions(xs.plan.handle, z.ptr, 3, 0.155, 10., 10.))
    xs.set_batch(pos, np.ones((2, 24, 24), np.float32))
    with pytest.raises(NotImplementedError, match='exit_shifts together with shifts'):
        xs.multislice(probe, exit_shifts=s, shifts=s)
    with pytest.raises(NotImplementedError, match='exit_shifts together with probes_b'):
        xs.multislice(probe, exit_shifts=s, probes_b=ctx.zeros((2, 1, 24, 24, 2)))
    with pytest.raises(ValueError, match='exit_shift_index'):
        xs.multislice(probe, exit_shifts=ctx.zeros((1, 2)))
    with pytest.raises(ValueError, match='need exit_shifts'):
        xs.multislice(probe, grad_exit_shifts=s)
    with pytest.raises(ValueError, match='null shifts'):
        check(ctx.lib.adm_multislice_fwd_adj_exit_shift(xs.plan.handle, xs.obj_rot.ptr, probe.ptr, xs._cur_pos.ptr, 2, xs._cur_target.ptr,
                                                        1, None, None, xs._loss.ptr, 1.0, xs._ws.ptr, xs._ws.nbytes, None, None, None))
    xs.plan.close()
    with pytest.raises(NotImplementedError, match='exit_shift together with slice_pos_cm'):
        mk(exit_shift=True, slice_pos_cm=[0., 1e-3, 2e-3])
    with pytest.raises(NotImplementedError, match='detector distances'):
        A.MultisliceEngine(ctx, (30, 30, 1), (24, 24), np.repeat(pos, 2, axis=0), ENERGY_EV, PSIZE_CM, free_prop_cm=[1e-3, 2e-3], max_batch=4,
                           exit_shift=True)
