"""adorym_amd.ProjectionEngine (pure_projection=True) against the NumPy restatement tests/projection_ref.py (pytest -m gpu).

Checkers: golden F25 (a) (the reference in fp64, its own fp32 run as the yardstick; tests/golden/gen_f25_pure_projection.py) on the
fixture's inputs, and the restatement in fp64 with its fp32 run as the yardstick (tests/test_projection_ref_vs_golden.py: a fair
one) at the sizes the fixture does not hold.  Bars: the 3x rule with the floors of tests/test_gpu_sparse_multislice.py (BARS).
"""
import ast
import os

import numpy as np
import pytest

from oracle import adorym_oracle as O
from tests import ms_matrix as MM
from tests import projection_ref as PJ

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENERGY_EV, PSIZE_CM = 8000., 1e-6
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
    return np.load(os.path.join(ROOT, 'tests', 'golden', 'F25_pure_projection.npz'))


def run_engine(A, ctx, case, theta=None, shifts=None, cls=None, **engine_kw):
    """rotate -> launch -> rotate_adjoint of a ProjectionEngine (or ``cls``).  ``case``: obj [Y,X,S,2], pos, probes [M,Py,Px] complex,
    meas [B,Py,Px], free_prop, sign_convention, loss."""
    obj, pos, probes, meas = [case[k] for k in ('obj', 'pos', 'probes', 'meas')]
    M, Py, Px = probes.shape
    B = len(pos)
    eng = (cls or A.ProjectionEngine)(ctx, obj.shape[:3], (Py, Px), pos, ENERGY_EV, PSIZE_CM, free_prop_cm=case['free_prop'],
                                      sign_convention=case['sign_convention'], n_probe_modes=M, max_batch=B,
                                      loss_function_type=case.get('loss', 'lsq'), beamstop=case.get('beamstop'), **engine_kw)
    table = A.RotationTable(ctx, obj.shape[:3], np.float32(theta)) if theta is not None else None
    d_grad, d_gp = ctx.zeros(obj.shape), ctx.zeros((M, Py, Px, 2))
    kw = {}
    if shifts is not None:
        d_gs = ctx.zeros((B, 2))
        kw = dict(shifts=ctx.array(np.asarray(shifts, np.float32)), grad_shifts=d_gs)
    # (the engine takes the data as the loss wants them: magnitudes for LSQ, intensities for Poisson -- ForwardModel.get_data)
    target = np.asarray(meas, np.float64) ** 2 if case.get('loss') == 'poisson' else meas
    eng.set_batch(pos, np.asarray(target, np.float32))
    eng.rotate(ctx.array(obj, np.float32), table)
    eng.multislice(ctx.array(MM.c2(probes)), grad_probe=d_gp, want_pred=True, **kw)
    eng.rotate_adjoint(d_grad, table)
    out = dict(pred=eng.pred(), loss=eng.loss(), grad=d_grad.get(), gprobe=MM.cplx(d_gp.get()), streamed=eng.streamed)
    if shifts is not None:
        out['gs'] = d_gs.get().astype(np.float64)
    if hasattr(eng, 'close'):
        eng.close()
    else:
        eng.plan.close()
    return out


def run_ref(case, dtype, theta=None, shifts=None):
    obj = case['obj']
    phys = O.Physics(case['probes'].shape[-2:], ENERGY_EV, PSIZE_CM, free_prop_cm=case['free_prop'], sign_convention=case['sign_convention'])
    coords = O.rotation_coords(obj.shape[:3], np.float32(theta), dtype) if theta is not None else None
    kw = dict(loss_function_type=case.get('loss', 'lsq'), beamstop=case.get('beamstop'))
    if shifts is not None:
        kw['shifts'] = np.asarray(shifts, np.float64)
    out = PJ.forward_adjoint_object(obj.astype(np.float64), coords, case['probes'].astype(np.complex128), case['pos'], case['meas'], phys,
                                    dtype, **kw)
    return dict(zip(('loss', 'pred', 'grad', 'gprobe', 'gs'), out))


def yardstick(r32, r64):
    """The fp32 run's distances from the fp64 run: pred, loss, grad, gprobe (whole), then gprobe per mode."""
    return [rel(r32['pred'], r64['pred']), abs(r32['loss'] / r64['loss'] - 1), rel(r32['grad'], r64['grad']),
            rel(r32['gprobe'], r64['gprobe'])] + [rel(a, b) for a, b in zip(r32['gprobe'], r64['gprobe'])]


def check_3x(res, r64, e32, what=''):
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
        print(what, 'gprobe[%d] %.2e (fp32 ref %.2e)' % (m, e, e32[4 + m]))
        assert e < BARS['grad'] and e <= 3 * e32[4 + m] + BARS['grad_abs'], ('probe gradient of mode %d' % m, e, e32[4 + m])


# ------------------------------------------------------------------------------------------- 1. the fixture's cases (the reference)
FIXTURE_CASES = ['s%d_%s' % (S, k) for S in (7, 1) for k in ('far_field', 'fresnel_m1_modes2', 'exit_wave', 'far_field_poisson')]


def fixture_case(F, name):
    names = [str(n) for n in F['kernel_cases']]
    S, free_prop, sg, M, loss = ast.literal_eval(str(F['kernel_case_params'][names.index(name)]))
    case = {k: F['%s/%s' % (name, k)] for k in ('obj', 'pos', 'probes', 'meas')}
    case.update(free_prop=free_prop, sign_convention=sg, loss=loss)
    return case


@pytest.mark.parametrize('name', FIXTURE_CASES)
def test_fixture_case_vs_reference(A, ctx, F, name):
    case = fixture_case(F, name)
    res = run_engine(A, ctx, case)
    r64 = {k: F['%s/%s' % (name, k)] for k in ('pred', 'grad', 'gprobe')}
    r64['loss'] = float(F[name + '/loss'])
    check_3x(res, r64, F[name + '/err32'], name)
    g = res['grad']
    assert np.array_equal(g, np.broadcast_to(g[:, :, :1], g.shape))          # one gradient for all slices, bit for bit


# ------------------------------------------------------------------------------------------- 2. beyond the fixture (the restatement)
def make_case(seed, size, probe, B, M=1, free_prop='inf', sg=1, beamstop=False):
    r = np.random.default_rng(seed)
    Y, X, S = size
    Py, Px = probe
    mk = lambda c: np.stack([14e-3 / S * c * r.uniform(size=(Y, X, S)), 14e-4 / S * c * r.uniform(size=(Y, X, S))], -1).astype(np.float32)
    obj, truth = mk(1), mk(1.5)
    pos = MM.edge_positions(r, B, Y, X, Py, Px)
    probes = ((0.5 + r.uniform(0, 1, (M, Py, Px))) * np.exp(1j * r.uniform(-np.pi, np.pi, (M, Py, Px)))).astype(np.complex64)
    case = dict(obj=obj, pos=pos, probes=probes, free_prop=free_prop, sign_convention=sg)
    if beamstop:
        yy, xx = np.mgrid[:Py, :Px]
        case['beamstop'] = (np.hypot(yy - Py / 2, xx - Px / 2) > 2.5).astype(np.float32)
    phys = O.Physics(probe, ENERGY_EV, PSIZE_CM, free_prop_cm=free_prop, sign_convention=sg)
    tiles, _ = O.extract_tiles(truth.astype(np.float64), pos, probe)
    case['meas'] = PJ.predict(tiles, probes.astype(np.complex128), phys)
    return case


def test_rotated_object_gradient(A, ctx):
    """37 x 53 x 7 at a non-zero angle, two modes, a Fresnel detector and a beamstop: the object gradient after the back-rotation."""
    case = make_case(2561, (37, 53, 7), (12, 20), 5, M=2, free_prop=2e-4, sg=-1, beamstop=True)
    theta = 0.6
    res = run_engine(A, ctx, case, theta=theta)
    r64, r32 = run_ref(case, 'float64', theta), run_ref(case, 'float32', theta)
    check_3x(res, r64, yardstick(r32, r64), 'rotated')
    assert np.abs(res['grad']).max() > 0


def test_sub_pixel_shifts(A, ctx):
    """One Fourier-shifted probe set per position (the one-slice engine's adm_probe_shift path, a tuned probe size)."""
    case = make_case(2562, (23, 29, 5), (16, 16), 5, free_prop='inf')
    shifts = np.array([[0.3, -0.45], [-0.2, 0.1], [0.49, 0.25], [-0.35, -0.4], [0.05, 0.3]])
    res = run_engine(A, ctx, case, theta=-0.4, shifts=shifts)
    r64, r32 = run_ref(case, 'float64', -0.4, shifts), run_ref(case, 'float32', -0.4, shifts)
    check_3x(res, r64, yardstick(r32, r64), 'shifts')
    e, e32 = rel(res['gs'], r64['gs']), rel(r32['gs'], r64['gs'])
    print('dL/dshifts %.2e (fp32 ref %.2e)' % (e, e32))
    assert e <= 3 * e32 + BARS['shift']


def test_streamed_probe_136(A, ctx):
    """A 136 x 136 probe does not fit one workgroup's LDS: streamed='auto' gives the one-slice engine the streamed kernels."""
    case = make_case(2563, (140, 150, 3), (136, 136), 2, free_prop=2e-4)
    res = run_engine(A, ctx, case, streamed='auto')
    assert res['streamed'] is True
    r64, r32 = run_ref(case, 'float64'), run_ref(case, 'float32')
    check_3x(res, r64, yardstick(r32, r64), 'streamed 136')


@pytest.mark.regression
@pytest.mark.parametrize('name', ['s1_fresnel_m1_modes2', 's1_far_field_poisson'])
def test_one_slice_equals_the_multislice_engine_bit_for_bit(A, ctx, F, name):
    """S = 1: the sum of one slice is the slice, the broadcast to one slice is a copy -- the ordinary engine's bits."""
    case = fixture_case(F, name)
    a = run_engine(A, ctx, case)
    b = run_engine(A, ctx, case, cls=A.MultisliceEngine)
    for k in ('pred', 'grad', 'gprobe'):
        assert np.array_equal(np.ascontiguousarray(a[k]).view(np.uint8), np.ascontiguousarray(b[k]).view(np.uint8)), k
    assert a['loss'] == b['loss']


def test_refusals(A, ctx):
    args = (ctx, (20, 20, 4), (16, 16), np.zeros((1, 2)), ENERGY_EV, PSIZE_CM)
    with pytest.raises(NotImplementedError, match="unknown_type='real_imag'"):
        A.ProjectionEngine(*args, unknown_type='real_imag')
    with pytest.raises(NotImplementedError, match='slice_pos_cm'):
        A.ProjectionEngine(*args, slice_pos_cm=[0., 1e-4, 2e-4, 3e-4])
    with pytest.raises(NotImplementedError, match='exit_shift'):
        A.ProjectionEngine(*args, exit_shift=True)
    with pytest.raises(NotImplementedError, match='detector distances'):
        A.ProjectionEngine(*args, free_prop_cm=[1e-3, 2e-3])
    with pytest.raises(NotImplementedError, match='pure_projection'):
        A.AngleBatch(ctx, (20, 20, 4), (16, 16), 2, ENERGY_EV, PSIZE_CM, pure_projection=True)
