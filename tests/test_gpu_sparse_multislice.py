"""Sparse multislice ptychography (slices at arbitrary depths, optionally refined) on the GPU (pytest -m gpu): the streamed kernels
with one transfer function per gap and the slice-position gradient (adm_ms_streamed.hip), the engine, SparseMultisliceModel and
the driver.

Checkers: golden F21 (recorded from the reference, tests/golden/gen_f21_sparse.py) and the NumPy restatement tests/sparse_ref.py
(tied to the reference and to the pinned oracle by tests/test_sparse_ref_vs_golden.py).  The rule throughout is the 3x rule: the
product's distance from the fp64 result is at most three times the distance of the fp32 run of the checker itself, plus a floor
-- tests/ms_matrix.py's GENERIC floors for prediction, loss, object and probe gradients; for dL/dz, which has no sibling, the
restatement's own fp32 error on the same case, computed here.
"""
import ast
import os
import pickle
import socket
import sys

import numpy as np
import pytest

from tests import ms_matrix as MM
from tests import sparse_ref as SR
from oracle import adorym_oracle as O      # checker only
import cases

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENERGY_EV, PSIZE_CM = 8000., 1e-6
BARS = MM.GENERIC


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
    return np.load(os.path.join(ROOT, 'tests', 'golden', 'F21_sparse_multislice.npz'))


rel = MM.rel


def run_sparse(A, ctx, case, want_gz=True, want_grad=True, keep_engine=False, **engine_kw):
    """rotate -> multislice -> rotate_adjoint of an engine built with the case's slice positions.  ``case``: obj [Y,X,S,2], pos,
    probes [M,Py,Px] complex, z [S] cm, meas [B,Py,Px], unknown_type, free_prop, sign_convention."""
    obj, pos, probes, z, meas = [case[k] for k in ('obj', 'pos', 'probes', 'z', 'meas')]
    M, Py, Px = probes.shape
    Y, X, S = obj.shape[:3]
    B = len(pos)
    eng = A.MultisliceEngine(ctx, (Y, X, S), (Py, Px), pos, ENERGY_EV, PSIZE_CM, free_prop_cm=case['free_prop'],
                             sign_convention=case['sign_convention'], n_probe_modes=M, max_batch=B, unknown_type=case['unknown_type'],
                             slice_pos_cm=z, **engine_kw)
    assert eng.streamed is True
    d_grad, d_gp, d_gz = ctx.zeros(obj.shape), ctx.zeros((M, Py, Px, 2)), ctx.zeros((S,))
    eng.set_batch(pos, np.asarray(meas, np.float32))
    eng.rotate(ctx.array(obj, np.float32), None)
    eng.multislice(ctx.array(MM.c2(probes)), grad_probe=d_gp, want_pred=True, grad_slice_pos=d_gz if want_gz else None)
    eng.rotate_adjoint(d_grad, None)
    out = dict(pred=eng.pred(), loss=eng.loss(), grad=d_grad.get(), gprobe=MM.cplx(d_gp.get()), gz=d_gz.get().astype(np.float64),
               n_rounds=len(eng.rounds(B)), z_after=eng.slice_pos.get())
    if keep_engine:
        out['engine'] = eng
    else:
        eng.plan.close()
    return out


def ref_sparse(case, dtype):
    phys = O.Physics(case['probes'].shape[-2:], ENERGY_EV, PSIZE_CM, free_prop_cm=case['free_prop'], sign_convention=case['sign_convention'],
                     unknown_type=case['unknown_type'])
    l, p, g, gp, gz = SR.forward_adjoint_object(case['obj'].astype(np.float64), None, case['probes'].astype(np.complex128), case['pos'],
                                                case['meas'], phys, np.asarray(case['z'], np.float64), dtype)
    return dict(loss=l, pred=p, grad=g, gprobe=gp, gz=gz)


def check_3x(res, r64, e32, gz_floor, what=''):
    """``e32``: the fp32 yardstick's distances from fp64 (pred, loss, grad, gprobe, gz, gprobe per mode ...)."""
    e = rel(res['pred'], r64['pred'])
    print(what, 'pred %.2e (fp32 ref %.2e)' % (e, e32[0]))
    assert e <= 3 * e32[0] + BARS['pred'], ('pred', e, e32[0])
    e = abs(res['loss'] / r64['loss'] - 1)
    print(what, 'loss %.2e (fp32 ref %.2e)' % (e, e32[1]))
    assert e <= 3 * e32[1] + BARS['loss'], ('loss', e, e32[1])
    e = rel(res['grad'], r64['grad'])
    print(what, 'grad %.2e (fp32 ref %.2e)' % (e, e32[2]))
    assert e < BARS['grad'] and e <= 3 * e32[2] + BARS['grad_abs'], ('object gradient', e, e32[2])
    for m in range(len(res['gprobe'])):
        e = rel(res['gprobe'][m], r64['gprobe'][m])
        print(what, 'gprobe[%d] %.2e (fp32 ref %.2e)' % (m, e, e32[5 + m]))
        assert e < BARS['grad'] and e <= 3 * e32[5 + m] + BARS['grad_abs'], ('probe gradient of mode %d' % m, e, e32[5 + m])
    e = rel(res['gz'], r64['gz'])
    print(what, 'dL/dz %.2e (fp32 ref %.2e, floor %.2e)' % (e, e32[4], gz_floor), res['gz'], r64['gz'])
    assert e <= 3 * e32[4] + gz_floor, ('dL/dz', e, e32[4], gz_floor, res['gz'], r64['gz'])


# ------------------------------------------------------------------------------------------- 1. the fixture's cases (the reference)
FIXTURE_CASES = ['s2_db_far_p1_m1', 's2_ri_none_m1_m2', 's3_db_fresnel_m1_m2', 's3_ri_far_m1_m1', 's3_db_none_p1_m1', 's3_ri_far_p1_m2',
                 's5_ri_fresnel_p1_m1', 's5_db_far_m1_m2']


def fixture_case(F, name):
    names = [str(n) for n in F['kernel_cases']]
    S, unknown, free_prop, sg, M = ast.literal_eval(str(F['kernel_case_params'][names.index(name)]))
    c = {k: F['%s/%s' % (name, k)] for k in ('obj', 'pos', 'probes', 'z', 'meas')}
    c.update(unknown_type=unknown, free_prop=free_prop if free_prop is not None else 0, sign_convention=sg)
    return c


@pytest.mark.parametrize('name', FIXTURE_CASES)
def test_engine_vs_reference(A, ctx, F, name):
    """Prediction, loss, object gradient, probe gradient per mode and dL/dz against the reference's fp64 run, the reference's own
    fp32 run as the yardstick."""
    case = fixture_case(F, name)
    res = run_sparse(A, ctx, case)
    r64 = {k: F['%s/%s' % (name, k)] for k in ('pred', 'grad', 'gprobe', 'gz')}
    r64['loss'] = float(F[name + '/loss'])
    floor = rel(ref_sparse(case, 'float32')['gz'], r64['gz'])
    check_3x(res, r64, F[name + '/err32'], floor, name)
    assert np.array_equal(res['z_after'], case['z'].astype(np.float32))       # a launch does not touch the positions


# --------------------------------------------------------------------------------- 2. sizes the fixture does not hold (restatement)
def make_case(P, S=3, B=11, M=1, unknown_type='delta_beta', free_prop='inf', sign_convention=1, seed=0, z=None):
    """Built like ms_matrix.oracle_case: positions hanging over all four edges, a truth with ten times the guess's contrast (and
    slice positions 3 % away) makes the data.  ``z`` [S] (cm): slice positions in place of the ones drawn."""
    Py, Px = (P, P) if np.isscalar(P) else tuple(P)
    r = np.random.default_rng([Py, Px, S, B, M, seed])
    Y, X = Py + 9, Px + 13
    if unknown_type == 'delta_beta':
        mk = lambda c: np.stack([2e-3 * c * r.uniform(size=(Y, X, S)), 2e-4 * c * r.uniform(size=(Y, X, S))], -1)
    else:
        mk = lambda c: np.stack([1 + 1e-2 * c * r.standard_normal((Y, X, S)), 2e-2 * c * r.standard_normal((Y, X, S))], -1)
    obj, truth = mk(1).astype(np.float32), mk(10).astype(np.float32)
    pos = MM.edge_positions(r, B, Y, X, Py, Px)
    probes = ((0.5 + r.uniform(0, 1, (M, Py, Px))) * np.exp(1j * r.uniform(-np.pi, np.pi, (M, Py, Px)))).astype(np.complex64)
    drawn = np.concatenate([[0.], np.cumsum(r.uniform(3e-4, 3e-3, S - 1))]).astype(np.float32)      # unequal gaps, 3 - 30 um
    z = drawn if z is None else np.asarray(z, np.float32)
    phys = O.Physics((Py, Px), ENERGY_EV, PSIZE_CM, free_prop_cm=free_prop, sign_convention=sign_convention, unknown_type=unknown_type)
    tiles, _ = O.extract_tiles(truth.astype(np.float64), pos, (Py, Px), unknown_type)
    meas = SR.predict(tiles, probes.astype(np.complex128), phys, (z * np.float32(1.03)).astype(np.float64))
    return dict(obj=obj, pos=pos, probes=probes, z=z, meas=meas.astype(np.float32), unknown_type=unknown_type, free_prop=free_prop,
                sign_convention=sign_convention)


def yardstick(case):
    """The restatement in fp64 and the distances of its fp32 run, in the layout of the fixture's err32."""
    r64, r32 = ref_sparse(case, 'float64'), ref_sparse(case, 'float32')
    e32 = [rel(r32['pred'], r64['pred']), abs(r32['loss'] / r64['loss'] - 1), rel(r32['grad'], r64['grad']), rel(r32['gprobe'], r64['gprobe']),
           rel(r32['gz'], r64['gz'])] + [rel(r32['gprobe'][m], r64['gprobe'][m]) for m in range(len(r64['gprobe']))]
    return r64, e32


SIZE_CASES = {
    'P72_S8': dict(P=72, S=8),
    'P136_S4_modes_real_imag': dict(P=136, S=4, M=2, unknown_type='real_imag'),
    'P136_S4_modes_fresnel': dict(P=136, S=4, M=2, free_prop=2e-3),
    'P200x240_S3_sign_m1': dict(P=(200, 240), S=3, sign_convention=-1),
    'P256_S8': dict(P=256, S=8),
    'P256_S3_modes_near': dict(P=256, S=3, M=2, free_prop=0),
}


@pytest.mark.parametrize('name', list(SIZE_CASES))
def test_engine_sizes_vs_restatement(A, ctx, name):
    """72 (a tuned size, forced onto the streamed plan by the slice positions), 136, 200 x 240, 256; S up to 8; B = 11."""
    kw = dict(SIZE_CASES[name])
    case = make_case(kw.pop('P'), **kw)
    r64, e32 = yardstick(case)
    # dL/dz comes back as float32, whose own resolution is 6e-8..1.2e-7: a case whose fp32 yardstick is not well above that (it
    # happens -- a real_imag object in front of a Fresnel detector: 1e-7; two slices and an exit-wave detector: 4e-9, the
    # rounding errors of 1e6 terms average out) would measure the output rounding, not the kernel.  The cases are chosen, from
    # the restatement alone, to have yardsticks of at least 1e-6.
    assert e32[4] >= 1e-6, e32[4]
    check_3x(run_sparse(A, ctx, case), r64, e32, e32[4], name)


# ------------------------------------------------------------------------------------------ 3. determinism, rounds, no leaks
def _same_bits(a, b, keys=('pred', 'loss', 'grad', 'gprobe', 'gz')):
    for k in keys:
        assert np.array_equal(np.asarray(a[k]), np.asarray(b[k])), k


def test_two_launches_give_identical_bits(A, ctx):
    case = make_case(136, S=4, M=2, seed=2)
    _same_bits(run_sparse(A, ctx, case), run_sparse(A, ctx, case))


def test_rounds_within_workspace_budget(A, ctx):
    """A batch split into rounds by the workspace budget: loss and prediction bit-identical, every round adds its share of dL/dz
    (inside the same 3x bar)."""
    case = make_case(136, S=3, M=2, seed=3)
    one = run_sparse(A, ctx, case, keep_engine=True)
    budget = one['engine'].plan.workspace_bytes(4)
    one['engine'].plan.close()
    parts = run_sparse(A, ctx, case, workspace_budget=budget)
    assert one['n_rounds'] == 1 and parts['n_rounds'] == 3
    assert parts['loss'] == one['loss'] and np.array_equal(parts['pred'], one['pred'])
    r64, e32 = yardstick(case)
    check_3x(parts, r64, e32, e32[4], 'rounds')
    assert rel(parts['gprobe'], one['gprobe']) < 1e-6 and rel(parts['grad'], one['grad']) < 1e-6


def test_no_slice_position_gradient_leaves_the_rest_unchanged(A, ctx):
    case = make_case(72, S=3, M=2, seed=4)
    with_gz, without = run_sparse(A, ctx, case), run_sparse(A, ctx, case, want_gz=False)
    _same_bits(with_gz, without, keys=('pred', 'loss', 'grad', 'gprobe'))
    assert np.all(without['gz'] == 0) and np.linalg.norm(with_gz['gz']) > 0


def test_streamed_engine_without_positions_is_untouched_by_a_sparse_one(A, ctx):
    """No shared state: an equidistant streamed engine gives the same bits before and after a sparse engine ran in the process,
    and with z_s = s * voxel the sparse engine agrees with it to rounding."""
    dense = MM.oracle_case(136, S=3, B=11, n_modes=2, seed=5)

    def run_dense():
        from tests.test_gpu_streamed_multislice import run_streamed
        return run_streamed(A, ctx, dense, streamed=True)
    before = run_dense()
    run_sparse(A, ctx, make_case(136, S=3, M=2, seed=5))
    after = run_dense()
    _same_bits(before, after, keys=('pred', 'loss', 'grad', 'gprobe'))


def test_equal_gaps_agree_with_the_equidistant_streamed_engine(A, ctx):
    """z_s = s * voxel: every gap's table is the dense path's H / (Py*Px) up to the rounding of the phase (a host fp64 exp rounded
    to fp32 there, an fp32 sincos of the fp64-reduced phase here)."""
    from tests.test_gpu_streamed_multislice import run_streamed
    dense = MM.oracle_case(136, S=3, B=11, n_modes=2, seed=6)
    st = run_streamed(A, ctx, dense, streamed=True)
    case = dict(obj=dense['obj'], pos=dense['pos'], probes=dense['probes'], z=np.arange(3) * MM.PSIZE_CM, meas=dense['target'],
                unknown_type='delta_beta', free_prop='inf', sign_convention=1)
    Y, X, S = dense['obj'].shape[:3]
    eng = A.MultisliceEngine(ctx, (Y, X, S), (136, 136), dense['pos'], MM.ENERGY_EV, MM.PSIZE_CM, n_probe_modes=2, max_batch=11,
                             slice_pos_cm=case['z'])
    d_grad, d_gp = ctx.zeros(dense['obj'].shape), ctx.zeros((2, 136, 136, 2))
    eng.set_batch(dense['pos'], dense['target'])
    eng.rotate(ctx.array(dense['obj'], np.float32), None)
    eng.multislice(ctx.array(MM.c2(dense['probes'])), grad_probe=d_gp, want_pred=True)
    eng.rotate_adjoint(d_grad, None)
    assert rel(eng.pred(), st['pred']) < 1e-5 and abs(eng.loss() / st['loss'] - 1) < 1e-5       # (the bars of test_streamed_matches_lds_kernels)
    assert rel(d_grad.get(), st['grad']) < 1e-5 and rel(MM.cplx(d_gp.get()), st['gprobe']) < 1e-5
    eng.plan.close()


# ------------------------------------------------------------------------------------------------------------ 4. refusals
def test_refusals(A, ctx):
    from adorym_amd._lib import check
    pos = np.array([(0, 0), (3, 5)])
    mk = lambda **kw: A.MultisliceEngine(ctx, (30, 30, 3), (24, 24), pos, ENERGY_EV, PSIZE_CM, max_batch=2, **kw)
    with pytest.raises(ValueError, match='slice positions'):
        mk(slice_pos_cm=[0., 1e-3])
    with pytest.raises(ValueError, match='binning'):
        mk(slice_pos_cm=[0., 1e-3, 2e-3], binning=2)
    lds = mk()                                                   # a plan of adm_plan_create
    assert lds.streamed is False
    z = ctx.array(np.array([0., 1e-3, 2e-3], np.float32))
    with pytest.raises(NotImplementedError, match='streamed plan'):
        check(ctx.lib.adm_plan_set_slice_positions(lds.plan.handle, z.ptr, 3, 0.155, 10., 10.))
    lds.plan.close()
    st = mk(streamed=True)
    with pytest.raises(ValueError, match='2 positions for a plan of 3 slices'):
        check(ctx.lib.adm_plan_set_slice_positions(st.plan.handle, z.ptr, 2, 0.155, 10., 10.))
    st.set_batch(pos, np.ones((2, 24, 24), np.float32))
    with pytest.raises(ValueError, match='no slice positions'):
        check(ctx.lib.adm_multislice_fwd_adj_sparse(st.plan.handle, st.obj_rot.ptr, ctx.zeros((1, 24, 24, 2)).ptr, st._cur_pos.ptr, 2,
                                                    st._cur_target.ptr, 1, None, None, st._loss.ptr, 1.0, st._ws.ptr, st._ws.nbytes, z.ptr))
    with pytest.raises(ValueError, match='slice_pos_cm'):
        st.multislice(ctx.zeros((1, 24, 24, 2)), grad_slice_pos=z)
    st.plan.close()
    b2 = mk(streamed=True, binning=2)
    with pytest.raises(ValueError, match='binning'):
        check(ctx.lib.adm_plan_set_slice_positions(b2.plan.handle, z.ptr, 3, 0.155, 10., 10.))
    b2.plan.close()
    sp = mk(slice_pos_cm=[0., 1e-3, 2e-3])
    sp.set_batch(pos, np.ones((2, 24, 24), np.float32))
    with pytest.raises(NotImplementedError, match='streamed'):
        sp.multislice(ctx.zeros((1, 24, 24, 2)), shifts=ctx.zeros((2, 2)))
    sp.plan.close()


def _drv_kw(tmp_path, **kw):
    base = dict(theta_st=0, theta_end=0, n_theta=1, two_d_mode=True, energy_ev=ENERGY_EV, psize_cm=PSIZE_CM, free_prop_cm='inf',
                gamma=0, alpha_d=0, alpha_b=0, optimizer='adam', save_path=str(tmp_path), output_folder='out', store_checkpoint=False,
                use_checkpoint=False, return_state=True)
    base.update(kw)
    return base


def test_driver_refusals(A, tmp_path):
    N, P = 30, 16
    prj = np.ones((1, 2, P, P), np.float32)
    guess = [np.zeros((N, N, 2)), np.zeros((N, N, 2))]
    kw = _drv_kw(tmp_path, fname=prj, obj_size=(N, N, 2), probe_pos=np.array([(0., 0.), (4., 6.)]), probe_type='plane', initial_guess=guess,
                 n_epochs=1, minibatch_size=2, slice_pos_cm_ls=[0, 10e-4])
    with pytest.raises(NotImplementedError, match='sub-pixel'):
        A.reconstruct_ptychography(**dict(kw, optimize_all_probe_pos=True))
    with pytest.raises(NotImplementedError, match='sub-pixel'):
        A.reconstruct_ptychography(**dict(kw, probe_pos=np.array([(0., 0.), (4.5, 6.)])))
    with pytest.raises(NotImplementedError, match='binning'):
        A.reconstruct_ptychography(**dict(kw, binning=2))
    with pytest.raises(ValueError, match='3 slice positions'):
        A.reconstruct_ptychography(**dict(kw, slice_pos_cm_ls=[0, 10e-4, 20e-4]))
    with pytest.raises(NotImplementedError, match='multi-distance'):
        A.reconstruct_ptychography(**dict(kw, fname=np.ones((1, 4, P, P), np.float32), free_prop_cm=[1e-3, 2e-3]))


# ------------------------------------------------------------------------------------------------------------ 5. the driver
def _drv_inputs(F):
    par = ast.literal_eval(str(F['drv/params']))
    probe = F['drv/probe_mag'] * np.exp(1j * F['drv/probe_phase'])
    kw = dict(fname=F['drv/prj'], obj_size=(par['N'], par['N'], par['S']), probe_pos=F['drv/pos'], unknown_type='real_imag',
              initial_guess=[F['drv/guess_mag'].astype(np.float64), F['drv/guess_phase'].astype(np.float64)], probe_type='supplied',
              probe_initial=[F['drv/probe_mag'], F['drv/probe_phase']], slice_pos_cm_ls=np.array(par['z0']), n_epochs=par['n_epochs'],
              minibatch_size=par['minibatch_size'], learning_rate=par['learning_rate'], optimize_probe=True,
              probe_learning_rate=par['probe_learning_rate'], slice_pos_learning_rate=par['slice_pos_learning_rate'])
    return par, probe, kw


def _check_driver(st, F, run, n_z):
    """Losses, z after every update, final object and probe against the reference's fp64 driver run, its fp32 run as the yardstick;
    floors: those of test_driver_2d_256_probe_modes_vs_oracle (losses 2e-4, object 5e-3 of the update, probe 1e-4) and, for z,
    1e-4 of the distance z has moved: z lives in fp32, whose spacing at 5e-3 cm is 4.7e-10 cm, and an update (the Adam step, the
    anchor subtraction) rounds it a few times -- ~1e-9 cm against the 2.8e-5 cm of the first update, 4e-5, rounded up."""
    t64, t32 = 'drv/%s_fp64/' % run, 'drv/%s_fp32/' % run
    l64, l32 = F[t64 + 'losses'], F[t32 + 'losses']
    assert len(st['losses']) == len(l64)
    print('losses', st['losses'], l64)
    assert np.allclose(st['losses'], l64, rtol=max(2e-4, 3 * np.abs(l32 / l64 - 1).max()))
    cp = lambda t, a, b: F[t + a].astype(np.float64) * np.exp(1j * F[t + b].astype(np.float64))
    x64, x32 = cp(t64, 'mag', 'phase'), cp(t32, 'mag', 'phase')
    x0 = F['drv/guess_mag'].astype(np.float64) * np.exp(1j * F['drv/guess_phase'].astype(np.float64))
    x = st['delta'].astype(np.float64) + 1j * st['beta'].astype(np.float64)
    upd = np.linalg.norm(x64 - x0)
    e, e_ref = np.linalg.norm(x - x64) / upd, np.linalg.norm(x32 - x64) / upd
    print('object', e, e_ref)
    assert upd > 0 and e < max(5e-3, 3 * e_ref), (e, e_ref)
    p64, p32 = cp(t64, 'probe_mag_ds_1', 'probe_phase_ds_1'), cp(t32, 'probe_mag_ds_1', 'probe_phase_ds_1')
    p = st['probe_real'] + 1j * st['probe_imag']
    pn = np.linalg.norm(p64)
    assert np.linalg.norm(p - p64) / pn < max(1e-4, 3 * np.linalg.norm(p32 - p64) / pn)
    z64, z32 = F[t64 + 'z_trace'], F[t32 + 'z_trace']
    if run == 'zfix':
        assert st['slice_pos_history'] is None and np.array_equal(st['slice_pos_cm_ls'], z64[-1].astype(np.float32))
        return
    zh = st['slice_pos_history'].astype(np.float64)
    assert zh.shape == z64.shape == (n_z, z64.shape[1]) and np.all(zh[:, 0] == 0)
    z0 = np.array(ast.literal_eval(str(F['drv/params']))['z0'])
    for k in range(n_z):
        moved = np.linalg.norm(z64[k] - z0)
        e, e_ref = np.linalg.norm(zh[k] - z64[k]) / moved, np.linalg.norm(z32[k] - z64[k]) / moved
        print('z after update %d' % k, zh[k], z64[k], e, e_ref)
        assert moved > 0 and e <= 3 * e_ref + 1e-4, (k, zh[k], z64[k], e, e_ref)
    assert np.array_equal(st['slice_pos_cm_ls'], st['slice_pos_history'][-1])


@pytest.mark.parametrize('model', ['auto', 'class'])
def test_driver_refines_slice_positions_vs_reference(A, F, tmp_path, model):
    par, _, kw = _drv_inputs(F)
    fm = 'auto' if model == 'auto' else A.SparseMultisliceModel
    st = A.reconstruct_ptychography(**_drv_kw(tmp_path, forward_model=fm, optimize_slice_pos=True, **kw))
    _check_driver(st, F, 'zopt', par['n_epochs'] * 2)


def test_driver_fixed_slice_positions_vs_reference(A, F, tmp_path):
    par, _, kw = _drv_inputs(F)
    st = A.reconstruct_ptychography(**_drv_kw(tmp_path, optimize_slice_pos=False, **kw))
    _check_driver(st, F, 'zfix', 0)


def test_driver_3d_object_vs_restatement(A, tmp_path):
    """A 28 x 28 x 4 object seen from three angles, 16 x 16 probe, slices at unequal depths, object + probe + slice positions
    refined, against tests/sparse_ref.py in fp64 with its fp32 run as the yardstick."""
    N, S, P, n_theta = 28, 4, 16, 3
    truth = np.stack([2e-3 * cases.smooth_field((N, N, S), 2171), 2e-4 * cases.smooth_field((N, N, S), 2172)], -1)
    guess = [6e-4 * cases.smooth_field((N, N, S), 2173), 6e-5 * cases.smooth_field((N, N, S), 2174)]
    theta_ls = np.linspace(0, np.pi, n_theta, dtype='float32')
    yy, xx = np.mgrid[:P, :P] - P / 2
    probe = np.exp(-(yy ** 2 + xx ** 2) / 30.) * np.exp(1j * 0.1 * yy / P)
    pos = np.array([(0, 0), (0, 12), (12, 0), (12, 12)], dtype=float)
    z0, z_true = np.array([0., 1e-3, 2.5e-3, 3e-3]), np.array([0., 1.05e-3, 2.4e-3, 3.1e-3])
    phys = O.Physics((P, P), ENERGY_EV, PSIZE_CM)
    prj = np.zeros((n_theta, len(pos), P, P))
    for i, th in enumerate(theta_ls):
        rot = O.rotate_fwd(truth, O.rotation_coords((N, N, S), th), 'float64')
        tiles, _ = O.extract_tiles(rot, pos.astype(int), (P, P))
        prj[i] = SR.predict(tiles, probe, phys, z_true)
    prj = prj.astype(np.float32)
    kw = dict(n_epochs=2, minibatch_size=2, learning_rate=1e-5, optimize_probe=True, probe_learning_rate=1e-3, optimize_slice_pos=True,
              slice_pos_learning_rate=1e-5)
    st = A.reconstruct_ptychography(fname=prj, obj_size=(N, N, S), probe_pos=pos, theta_st=0, theta_end=np.pi, n_theta=n_theta,
                                    energy_ev=ENERGY_EV, psize_cm=PSIZE_CM, free_prop_cm='inf', probe_type='supplied',
                                    probe_initial=[np.abs(probe), np.angle(probe)], initial_guess=guess, slice_pos_cm_ls=z0, gamma=0, alpha_d=0,
                                    alpha_b=0, optimizer='adam', save_path=str(tmp_path), output_folder='s3d', store_checkpoint=False,
                                    use_checkpoint=False, return_state=True, **kw)
    runs = {dt: SR.reconstruct(prj.astype(np.float64), guess, probe, pos, phys, z0, theta_ls=theta_ls, dtype=dt, **kw) for dt in ('float64', 'float32')}
    o64, o32 = runs['float64'], runs['float32']
    assert len(st['losses']) == len(o64['losses'])
    assert np.allclose(st['losses'], o64['losses'], rtol=max(2e-4, 3 * np.abs(np.array(o32['losses']) / np.array(o64['losses']) - 1).max()))
    x = np.stack([st['delta'], st['beta']], -1)
    upd = np.linalg.norm(o64['obj'] - np.stack(guess, -1))
    e, e_ref = np.linalg.norm(x - o64['obj']) / upd, np.linalg.norm(o32['obj'] - o64['obj']) / upd
    print('object', e, e_ref)
    assert upd > 0 and e < max(5e-3, 3 * e_ref), (e, e_ref)
    zh = st['slice_pos_history'].astype(np.float64)
    assert zh.shape == o64['z_history'].shape
    for k in range(len(zh)):
        moved = np.linalg.norm(o64['z_history'][k] - z0)
        e, e_ref = np.linalg.norm(zh[k] - o64['z_history'][k]) / moved, np.linalg.norm(o32['z_history'][k] - o64['z_history'][k]) / moved
        print('z after update %d' % k, zh[k], o64['z_history'][k], e, e_ref)
        assert e <= 3 * e_ref + 1e-4, (k, zh[k], o64['z_history'][k], e, e_ref)


def test_checkpoint_carries_the_slice_positions(A, F, tmp_path):
    """params_0 holds slice_pos_cm_ls under the reference's key, and a resumed run starts from the refined positions: resumed
    with the refinement delayed beyond the end, its final z IS the checkpointed one -- the first run's z after its first update (the last
    checkpoint is written in front of the epoch's second and last minibatch)."""
    par, _, kw = _drv_inputs(F)
    common = dict(optimize_slice_pos=True, store_checkpoint=True, n_batch_per_checkpoint=1)
    part = A.reconstruct_ptychography(**_drv_kw(tmp_path, output_folder='part', **dict(kw, n_epochs=1, **common)))
    with open(os.path.join(part['output_folder'], 'checkpoint', 'params_0'), 'rb') as f:
        saved = pickle.load(f)
    assert 'slice_pos_cm_ls' in saved
    z_saved = np.asarray(saved['slice_pos_cm_ls'], np.float32)
    assert np.array_equal(z_saved, part['slice_pos_history'][0]) and not np.array_equal(z_saved, np.array(par['z0'], np.float32))
    res = A.reconstruct_ptychography(**_drv_kw(tmp_path, output_folder='part', **dict(kw, n_epochs=1, use_checkpoint=True,
                                                                                     other_params_update_delay=10 ** 6, **common)))
    assert np.array_equal(res['slice_pos_cm_ls'], z_saved)


def test_manual_script_keyword_set(A, F, tmp_path):
    """tests/manual_scripts/test_sparse_multislice_ptycho.py of the reference at reduced size (two slices 10 um apart, probe from
    the data with an extra defocus and rescaled intensity, probe updates delayed): runs, and the loss falls."""
    par, _, _ = _drv_inputs(F)
    N = par['N']
    st = A.reconstruct_ptychography(
        fname=F['drv/prj'], probe_pos=F['drv/pos'], energy_ev=ENERGY_EV, psize_cm=PSIZE_CM, theta_st=0, theta_end=0, theta_downsample=None,
        n_epochs=6, obj_size=(N, N, 2), alpha_d=0, alpha_b=0, gamma=0, two_d_mode=True, learning_rate=1e-3, probe_learning_rate=1e-3,
        minibatch_size=8, randomize_probe_pos=False, n_batch_per_update=1, output_folder='test', cpu_only=False, save_path=str(tmp_path),
        multiscale_level=1, use_checkpoint=False, store_checkpoint=False, n_epoch_final_pass=None, save_intermediate=True,
        full_intermediate=True, initial_guess=None, random_guess_means_sigmas=(1., 0., 0.001, 0.002), n_dp_batch=350, optimize_probe=True,
        probe_update_delay=4, slice_pos_cm_ls=[0, 10e-4], probe_type='ifft', probe_extra_defocus_cm=20e-4, probe_initial=None,
        rescale_probe_intensity=True, forward_algorithm='fresnel', finite_support_mask_path=None, shared_file_object=False,
        reweighted_l1=False, optimizer='adam', free_prop_cm='inf', backend='pytorch', raw_data_type='magnitude', beamstop=None, debug=False,
        optimize_all_probe_pos=False, all_probe_pos_learning_rate=1e-2, optimize_slice_pos=False, slice_pos_learning_rate=1e-5,
        save_history=True, update_scheme='immediate', unknown_type='real_imag', save_stdout=True, loss_function_type='lsq',
        normalize_fft=False, sign_convention=1, return_state=True)
    l = np.array(st['losses'])
    assert len(l) == 12 and np.all(np.isfinite(l)) and l[-2:].mean() < l[:2].mean(), l
    assert np.array_equal(st['slice_pos_cm_ls'], np.array([0, 10e-4], np.float32))


# ------------------------------------------------------------------------------------------------------------ 6. two ranks
def _free_port():
    s = socket.socket(); s.bind(('127.0.0.1', 0)); p = s.getsockname()[1]; s.close()
    return p


def _worker(rank, world, port, tmp, q):
    """One rank: a fresh process that has not touched the GPU before (the pattern of tests/test_gpu_world2.py)."""
    sys.path.insert(0, ROOT)
    sys.path.insert(0, os.path.join(ROOT, 'tests', 'golden'))
    os.environ.update(RANK=str(rank), WORLD_SIZE=str(world), LOCAL_RANK='0', MASTER_ADDR='127.0.0.1', MASTER_PORT=str(port), ADM_COMM='host')
    try:
        import adorym_amd as A
        from adorym_amd import comm as C
        F = np.load(os.path.join(ROOT, 'tests', 'golden', 'F21_sparse_multislice.npz'))
        par, _, kw = _drv_inputs(F)
        comm = C.from_env()
        assert type(comm) is C.HostStagedComm and comm.size == world
        st = A.reconstruct_ptychography(comm=comm, **_drv_kw(tmp, optimize_slice_pos=True, **dict(kw, minibatch_size=par['minibatch_size'] // world)))
        comm.close()
        q.put(dict(rank=rank, z=st['slice_pos_cm_ls'], zh=st['slice_pos_history'], losses=np.array(st['losses'])))
    except Exception as e:       # report instead of leaving the parent waiting for the queue
        import traceback
        q.put(dict(rank=rank, error='%r\n%s' % (e, traceback.format_exc())))


def test_world2_slice_positions(F, tmp_path):
    """Two ranks on one GPU (host-staged transport), each with half of every global batch: the slice-position gradients are summed
    over the ranks, so both end with the same z -- the z of the two-rank restatement (fp64, its fp32 run as the yardstick), which
    runs over the same global batches as the one-rank fixture run."""
    import multiprocessing as mp
    world, port = 2, _free_port()
    os.environ['ADM_RDV_TOKEN'] = __import__('secrets').token_hex(16)
    mpc = mp.get_context('spawn')
    q = mpc.Queue()
    procs = [mpc.Process(target=_worker, args=(r, world, port, str(tmp_path), q)) for r in range(world)]
    [p.start() for p in procs]
    res = [q.get(timeout=600) for _ in procs]
    [p.join(120) for p in procs]
    for r in res:
        assert 'error' not in r, r['error']
    res = sorted(res, key=lambda r: r['rank'])
    assert np.array_equal(res[0]['z'], res[1]['z']) and np.array_equal(res[0]['zh'], res[1]['zh'])
    par, probe, kw = _drv_inputs(F)
    gm, gp = kw['initial_guess']
    guess = [gm * np.cos(gp), gm * np.sin(gp)]
    phys = O.Physics(probe.shape, ENERGY_EV, PSIZE_CM, unknown_type='real_imag')
    runs = {dt: SR.reconstruct(F['drv/prj'].astype(np.float64), guess, probe, F['drv/pos'], phys, par['z0'], n_epochs=par['n_epochs'],
                               minibatch_size=par['minibatch_size'] // world, learning_rate=par['learning_rate'], optimize_probe=True,
                               probe_learning_rate=par['probe_learning_rate'], optimize_slice_pos=True,
                               slice_pos_learning_rate=par['slice_pos_learning_rate'], n_ranks=world, dtype=dt) for dt in ('float64', 'float32')}
    z64, z32, zh = runs['float64']['z_history'], runs['float32']['z_history'], res[0]['zh'].astype(np.float64)
    assert zh.shape == z64.shape
    for k in range(len(zh)):
        moved = np.linalg.norm(z64[k] - np.array(par['z0']))
        e, e_ref = np.linalg.norm(zh[k] - z64[k]) / moved, np.linalg.norm(z32[k] - z64[k]) / moved
        print('z after update %d' % k, zh[k], z64[k], e, e_ref)
        assert e <= 3 * e_ref + 1e-4, (k, zh[k], z64[k], e, e_ref)
    # the same global batches as the one-rank run: the summed gradient is twice the one-rank mean, which Adam's normalisation
    # removes up to eps -- the two runs' z agree far inside one step
    one = F['drv/zopt_fp64/z_trace']
    assert np.abs(zh - one).max() < 0.05 * par['slice_pos_learning_rate']
