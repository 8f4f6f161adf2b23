"""Every launch geometry of the any-size multislice kernel (ms_generic_kernel, adm_ms_generic.hip) against the fp64 oracle
(pytest -m gpu).  tests/gen_matrix.py holds the fields, the classes of geometry they reach and the launch sequences;
tests/test_generic_matrix_coverage.py ties those tables to the kernel source and checks the cases on the oracle alone.

Judged twice: by ms_matrix.check with the GENERIC bars (whole arrays, by norm), and slot by slot -- element i = tid + j * nt of
the field lives in register slot j of every thread, so the natural-order intervals [j * nt, (j + 1) * nt) of every position's
prediction (through the far-field fftshift, as the kernel's my / mx) and of every mode's probe gradient are judged on their own
by the 3x rule, with the oracle's fp32 run on the same band as the yardstick (check_bands of the streamed matrix, handed the
slot bands).  An error confined to the last, ragged slot of 127 x 129 (1023 of 16383 elements) is diluted fourfold in a norm
over the whole array; in its own band it is not.  No band may be without signal.

Every oracle case is built once per module (_CASES) and left as it is; the engine's results go into a copy.
"""
import time

import numpy as np
import pytest

from tests import gen_matrix as GM
from tests import ms_matrix as MM
from tests.test_gpu_streamed_matrix import check_bands, transposed

pytestmark = pytest.mark.gpu
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


_CASES = {}


def case_key(P, **kw):
    return (tuple(P), tuple(sorted((k, str(v)) for k, v in kw.items())))


def oracle_case(P, **kw):
    """MM.oracle_case, built once per module."""
    key = case_key(P, **kw)
    if key not in _CASES:
        _CASES[key] = MM.oracle_case(P, **kw)
    return _CASES[key]


def run(A, ctx, case):
    """MM.run_engine (what MM.run_case runs behind the oracle) on a copy of the shared case."""
    return MM.run_engine(A, ctx, dict(case))


def slot_sets(shape):
    return (('slot', None, GM.slot_bands(*shape)),)


def judge(res, what):
    shape = res['kw']['shape']
    gp = res['gprobe'] is not None
    print('%s: pred %.2e (fp32 oracle %.2e)  loss %.2e  grad %.2e (%.2e)  gprobe %.2e (%.2e)' % (
        what, MM.rel(res['pred'], res['pred_o']), MM.rel(res['pred_32'], res['pred_o']), abs(res['loss'] / res['loss_o'] - 1),
        MM.rel(res['grad'], res['grad_o']), MM.rel(res['grad_32'], res['grad_o']),
        MM.rel(res['gprobe'], res['gprobe_o']) if gp else 0, MM.rel(res['gprobe_32'], res['gprobe_o']) if gp else 0))
    MM.check(res, BARS)
    return check_bands(res, what, slot_sets(shape), BARS, without_signal=0, each=True)


# ---------------------------------------------------------------------------------------------------- a. shapes
@pytest.mark.parametrize('shape', sorted(GM.SHAPES, key=lambda s: (s[0] * s[1], s)), ids=lambda s: '%dx%d' % s)
def test_shapes_vs_oracle(A, ctx, shape):
    """Every field of gen_matrix.SHAPES, in ascending size: prediction, loss, object gradient and probe gradient against the
    fp64 oracle by the GENERIC bars, then the prediction and the probe gradient slot by slot."""
    assert GM.supported(*shape)
    judge(run(A, ctx, oracle_case(shape, **GM.SHAPES[shape])), '%dx%d' % shape)


# ---------------------------------------------------------------------------------------------------- b. launch sequences
def run_flagged(A, ctx, case, want_grad=True, want_pred=True, with_gprobe=True):
    """The launch of MM.run_engine on one shared probe set with an output left out: ``want_grad`` False -- the forward-only
    launch, 'gprobe_raw' and 'grad_rot' are then the probe-gradient buffer (handed over filled with 3) and the engine's
    rotated-frame gradient (filled with 5) as the launch left them; ``want_pred`` False -- pred = NULL; ``with_gprobe`` False --
    grad_probe = NULL."""
    out, k = {}, case['kw']
    obj, pos, probes, target, bs = [case[n] for n in ('obj', 'pos', 'probes', 'target', 'beamstop')]
    (Py, Px), S, B, M = k['shape'], k['S'], k['B'], k['n_modes']
    Y, X = obj.shape[:2]
    eng = A.MultisliceEngine(ctx, (Y, X, S), (Py, Px), pos, MM.ENERGY_EV, MM.PSIZE_CM, free_prop_cm=k['free_prop'], binning=k['binning'],
                             fresnel_approx=k['fresnel_approx'], sign_convention=k['sign_convention'], normalize_fft=k['normalize_fft'],
                             n_probe_modes=M, max_batch=B, loss_function_type=k['loss'], poisson_multiplier=k['poisson_multiplier'],
                             unknown_type=k['unknown_type'], beamstop=bs, generic=k['generic'], transmission_cache=k['transmission_cache'])
    d_grad = ctx.zeros(obj.shape)
    d_probe = ctx.array(MM.c2(probes))
    eng.set_batch(pos, target)
    eng.rotate(ctx.array(obj, np.float32), None)
    if want_grad:
        d_gp = ctx.zeros((M, Py, Px, 2)) if with_gprobe else None
        eng.multislice(d_probe, grad_probe=d_gp, want_pred=want_pred)
        eng.rotate_adjoint(d_grad, None)
        out['grad'] = d_grad.get()
        if with_gprobe:
            out['gprobe'] = MM.cplx(d_gp.get())
    else:
        d_gp = ctx.array(np.full((M, Py, Px, 2), 3, np.float32))
        eng.grad_rot.set(np.full(eng.grad_rot.shape, 5, np.float32))
        eng.multislice(d_probe, grad_probe=d_gp, want_grad=False, want_pred=want_pred)
        out['gprobe_raw'], out['grad_rot'] = d_gp.get(), eng.grad_rot.get()
    if want_pred:
        out['pred'] = eng.pred()
    out['loss'] = eng.loss()
    eng.plan.close()
    return out


def same_bits(a, b, keys, what):
    for k in keys:
        assert np.array_equal(np.asarray(a[k]), np.asarray(b[k])), (what, k)


@pytest.mark.parametrize('name,cls', GM.SEQUENCE_CASES)
def test_sequences_vs_oracle(A, ctx, name, cls):
    """Every run-time branch of the kernel at a field of 256 threads and at one of 640, both with a ragged last slot.  Flagged
    sequences launch a second time with an output left out: every other output keeps its bits, and a forward-only launch
    writes no gradient buffer."""
    kw, flags = GM.sequence_kw(name)
    case = oracle_case(GM.SEQUENCE_SHAPES[cls], **kw)
    full = run(A, ctx, case)
    judge(full, '%s %s' % (name, cls))
    if 'forward_only' in flags:
        fwd = run_flagged(A, ctx, case, want_grad=False)
        same_bits(fwd, full, ('loss', 'pred'), name)
        assert np.all(fwd['gprobe_raw'] == 3) and np.all(fwd['grad_rot'] == 5)
    if 'pred_null' in flags:
        same_bits(run_flagged(A, ctx, case, want_pred=False), full, ('loss', 'grad', 'gprobe'), name)
    if 'gprobe_null' in flags:
        same_bits(run_flagged(A, ctx, case, with_gprobe=False), full, ('loss', 'pred', 'grad'), name)


@pytest.mark.regression
@pytest.mark.parametrize('name', [n for n in GM.SEQUENCES if GM.sequence_kw(n)[1]])
def test_flagged_launches_keep_the_other_outputs_bits(A, ctx, name):
    """The relations of the flagged sequences at the largest ragged field (127 x 129, 1024 threads): forward-only, pred = NULL
    and grad_probe = NULL launches against the full launch, bit for bit."""
    kw, flags = GM.sequence_kw(name)
    case = oracle_case((127, 129), **kw)
    full = run_flagged(A, ctx, case)
    if 'forward_only' in flags:
        fwd = run_flagged(A, ctx, case, want_grad=False)
        same_bits(fwd, full, ('loss', 'pred'), name)
        assert np.all(fwd['gprobe_raw'] == 3) and np.all(fwd['grad_rot'] == 5)
    if 'pred_null' in flags:
        same_bits(run_flagged(A, ctx, case, want_pred=False), full, ('loss', 'grad', 'gprobe'), name)
    if 'gprobe_null' in flags:
        same_bits(run_flagged(A, ctx, case, with_gprobe=False), full, ('loss', 'pred', 'grad'), name)


# ---------------------------------------------------------------------------------------------------- c. consistency
@pytest.mark.regression
def test_two_launches_give_identical_bits_at_the_largest_ragged_field(A, ctx):
    case = oracle_case((127, 129), S=3, B=5, n_modes=3)
    a, b = run(A, ctx, case), run(A, ctx, case)
    assert a['loss'] == b['loss']
    same_bits(a, b, ('pred', 'grad', 'gprobe'), '127x129')
    judge(a, '127x129 three modes')


@pytest.mark.regression
@pytest.mark.parametrize('shape', GM.TRANSPOSED_PAIRS, ids=lambda s: '%dx%d' % s)
def test_transposed_problem_agrees(A, ctx, shape):
    """Exchanging the axes of the whole problem moves the five passes of 1890 (the two leftover primes of 143) from the x passes
    to the y passes and every element into another slot: loss, prediction and gradients agree to the 1e-5 of the streamed
    matrix's test_transposed_problem_agrees."""
    case = oracle_case(shape, S=3, B=5, n_modes=2, seed=7)
    a, b = run(A, ctx, case), run(A, ctx, transposed(case))
    assert abs(b['loss'] - a['loss']) <= 1e-5 * abs(a['loss']), (a['loss'], b['loss'])
    assert MM.rel(np.swapaxes(b['pred'], -1, -2), a['pred']) < 1e-5
    assert MM.rel(b['grad'].transpose(1, 0, 2, 3), a['grad']) < 1e-5
    for m in range(2):
        assert MM.rel(b['gprobe'][m].T, a['gprobe'][m]) < 1e-5, m
    judge(b, '%dx%d transposed' % shape)


# ---------------------------------------------------------------------------------------------------- d. the LDS bound
def test_fields_at_the_lds_bound(A, ctx):
    """4 x 4096, 2 x 8192 and 1 x 16384 hold 16384 elements like 128 x 128 and are refused all the same: the field, a row of
    x twiddles and a column of y twiddles do not fit 160 KB - 256.  3 x 4096 (four passes of 8, no 2048 side limit on this path)
    is on the accepted side and is swept with the other fields."""
    for Py, Px in GM.LDS_REFUSED:
        assert Py * Px == GM.NT_CAP * GM.GEN_E and GM.threads(Py, Px) == GM.NT_CAP and not GM.supported(Py, Px)
        with pytest.raises(NotImplementedError):
            A.MultisliceEngine(ctx, (Py + 2, Px + 2, 3), (Py, Px), np.array([(0, 0)]), MM.ENERGY_EV, MM.PSIZE_CM)
        assert b'too large' in ctx.lib.adm_last_error()
    assert GM.supported(*GM.LDS_ACCEPTED) and GM.LDS_ACCEPTED in GM.SHAPES
    eng = A.MultisliceEngine(ctx, (5, 4098, 3), GM.LDS_ACCEPTED, np.array([(0, 0)]), MM.ENERGY_EV, MM.PSIZE_CM)
    assert not eng.streamed
    eng.plan.close()


if __name__ == '__main__':      # the CPU time of the module's oracle runs
    t0 = time.time()
    for shape in GM.SHAPES:
        oracle_case(shape, **GM.SHAPES[shape])
    t1 = time.time()
    for name, cls in GM.SEQUENCE_CASES:
        oracle_case(GM.SEQUENCE_SHAPES[cls], **GM.sequence_kw(name)[0])
    print('oracle: %d shapes %.1f s, %d sequence cases %.1f s' % (len(GM.SHAPES), t1 - t0, len(GM.SEQUENCE_CASES), time.time() - t1))
