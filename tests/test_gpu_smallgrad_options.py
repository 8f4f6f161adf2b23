"""dL/dz, dL/ds and dL/dd under every loss, data, mask and mode-count option on the GPU (pytest -m gpu): the rows of
tests/smallgrad_matrix.py through the runners of the three sibling modules (run_sparse, run_shifted, run_refine), each one small
engine and one launch at 24 x 20.

Reference: the extended restatements (tests/sparse_ref.py, tests/prj_offset_ref.py, tests/multidist3d_dist_ref.py) in fp64, tied to
the pinned oracle and to finite differences by tests/test_smallgrad_conditions.py; yardstick: their float32 run.  Judgement: each
module's own rule -- check_3x of test_gpu_sparse_multislice.py with the fp32 restatement's dL/dz error as the floor, check_3x /
gs_bar of test_gpu_prj_offset.py, ms_matrix.check with GENERIC and check_dists of test_gpu_multidist3d_dist.py.  Every figure is
printed before it is held to its bar.
"""
import numpy as np
import pytest

from tests import ms_matrix as MM
from tests import smallgrad_matrix as T
from tests import test_gpu_sparse_multislice as SP
from tests import test_gpu_prj_offset as PO
from tests import test_gpu_multidist3d as MD
from tests import test_gpu_multidist3d_dist as DD

pytestmark = pytest.mark.gpu
BARS = MM.GENERIC
rel = MM.rel

OPTION_ROWS = [n for n, r in T.ROWS.items() if r['kind'] == 'reference']
IDENTITY_ROWS = [n for n, r in T.ROWS.items() if r['kind'] == 'identity']
FAR_ROWS = list(T.FAR_ROWS)
MASKED_ROWS = [n for n in OPTION_ROWS if T.settings(T.ROWS[n]['option'])['beamstop']]
TWICE_ROWS = ['sparse-poisson_intensity-M2', 'exit_shift-beamstop_poisson-M2', 'fanout-poisson_magnitude-M2']
MOVED_PAIRS = [('sparse-z-base-%s' % o, 'sparse-z-moved_1cm-%s' % o) for o in T.Z_LOSSES]
Z_ROWS = [n for n, r in T.Z_ROWS.items() if r['kw']['z'] != 'moved_1cm']
ZERO_ROWS = list(T.ZERO_ROWS)
OUTPUTS = ('pred', 'loss', 'grad', 'gprobe', 'small')


@pytest.fixture(scope='module')
def A():
    import adorym_amd
    return adorym_amd


@pytest.fixture(scope='module')
def ctx(A):
    c = A.Context(0)
    yield c
    c.close()


def run_row(A, ctx, case, gs_init=None, **over):
    """The path's own runner on a row's case; 'small' is the small gradient as the launch left it (float32 values in fp64)."""
    path = case['row']['path']
    kw = T.engine_kw(case)
    kw.update(over)
    if path == 'sparse':
        res = SP.run_sparse(A, ctx, T.engine_case(case), **kw)
        res['small'] = res['gz']
    elif path == 'exit_shift':
        res = PO.run_shifted(A, ctx, T.engine_case(case), gs_init=gs_init, canaries=True, **kw)
        res['small'] = res['gs']
    else:
        res = DD.run_refine(A, ctx, case, **kw)
        res['small'] = res['gdists']
    return res


def judge(case, res, r64, r32, e32, what):
    """Each module's own rule, the extended restatement in fp64 as the reference and its float32 run as the yardstick."""
    path = case['row']['path']
    for k in OUTPUTS:
        assert np.all(np.isfinite(np.asarray(res[k]))), (what, k, 'not finite')
    if path == 'sparse':
        SP.check_3x(res, dict(r64, gz=r64['small']), e32, e32[4], what)
    elif path == 'exit_shift':
        PO.check_3x(res, dict(r64, gs=r64['small']), e32, what)
    else:
        full = MD.as_res(res, r64, r32, case)
        MD.report(full, what)
        MM.check(full, BARS)
        DD.check_dists(res, r64['small'], r32['small'], what)


def same_bits(a, b, what, keep=None):
    """Every output bit-identical (``keep`` [Py, Px] bool: the prediction at these detector pixels only) and finite."""
    for k in OUTPUTS:
        x, y = np.asarray(a[k]), np.asarray(b[k])
        if k == 'pred' and keep is not None:
            x, y = x[:, keep], y[:, keep]
        assert np.all(np.isfinite(x)), (what, k, 'not finite')
        assert np.array_equal(x, y), (what, k)


# ------------------------------------------------------------------------------------------------------------------ 1. the options
@pytest.mark.parametrize('name', OPTION_ROWS)
def test_options_vs_restatement(A, ctx, name):
    """Prediction, loss, object gradient, probe gradient and the small gradient of every option x path x mode count."""
    case = T.build(name)
    r64, r32, e32 = T.yardstick(name)
    judge(case, run_row(A, ctx, case), r64, r32, e32, name)


@pytest.mark.parametrize('name', IDENTITY_ROWS)
def test_normalize_fft_changes_no_bit_behind_a_fresnel_or_exit_wave_detector(A, ctx, name):
    case = T.build(name)
    assert case['normalize_fft'] is True
    same_bits(run_row(A, ctx, case), run_row(A, ctx, case, normalize_fft=False), name)


@pytest.mark.parametrize('name', FAR_ROWS)
def test_far_field_leaves_the_offset_gradient_alone(A, ctx, name):
    """A far-field magnitude does not see the offsets, under either loss: the gradient buffer comes back bit-unchanged and the
    rest is the restatement's."""
    case = T.build(name)
    init = np.arange(6, dtype=np.float32).reshape(3, 2) * 0.3 - 1
    res = run_row(A, ctx, case, gs_init=init)
    assert np.array_equal(res['gs_raw'], init)
    r64, r32 = T.ref(case), T.ref(case, 'float32')
    full = MD.as_res(res, r64, r32, dict(case, dists=['inf']))
    MD.report(full, name)
    MM.check(full, BARS)


# ------------------------------------------------------------------------------------------------------------------ 2. under the mask
@pytest.mark.parametrize('roll', [0, 2])
@pytest.mark.parametrize('name', MASKED_ROWS)
def test_dirt_under_the_mask_changes_no_bit(A, ctx, name, roll):
    """NaN, +inf, -1, 0 and 3e38 in the target under the mask: loss, prediction at the kept pixels, object gradient, probe gradient
    and the small gradient are finite and bit-identical to the clean run."""
    case = T.build(name)
    dirty = T.dirtied(case, roll)
    drop = case['beamstop'] < 1e-5
    assert not np.all(np.isfinite(dirty['target'][:, drop])) and np.array_equal(dirty['target'][:, ~drop], case['target'][:, ~drop])
    same_bits(run_row(A, ctx, dirty), run_row(A, ctx, case), '%s roll %d' % (name, roll), keep=~drop)


@pytest.mark.parametrize('name', ZERO_ROWS)
def test_zero_predictions_under_two_modes(A, ctx, name):
    """M = 2, an exit-wave detector, both probes exactly 0 outside a disc: loss_term_nz divides by a prediction that is zero up to
    the rounding of a transform pair (and exactly zero where that cancels).  With those pixels under the mask every output, the
    small gradient included, is finite and the restatement's.  Without the mask the outcome is only recorded: the reference has
    no guard there either, and its fp64 run divides rounding noise by rounding noise."""
    bare = T.build(name)
    case = T.with_mask(bare, T.zero_mask())
    r64, r32 = T.ref(case), T.ref(case, 'float32')
    e32 = [rel(r32[k], r64[k]) for k in ('pred', 'pred', 'grad', 'gprobe', 'small')] + [rel(a, b) for a, b in zip(r32['gprobe'], r64['gprobe'])]
    e32[1] = abs(r32['loss'] / r64['loss'] - 1)
    res = run_row(A, ctx, case)
    out = ~T.disc()
    print(name, 'masked: predictions of exactly zero: %d of %d, largest %.1e' % ((res['pred'][:, out] == 0).sum(), res['pred'][:, out].size,
                                                                                 res['pred'][:, out].max()))
    judge(case, res, r64, r32, e32, name)
    res = run_row(A, ctx, bare)
    print(name, 'unmasked:', {k: bool(np.all(np.isfinite(np.asarray(res[k])))) for k in OUTPUTS})
    assert np.all(np.isfinite(res['pred']))


# ------------------------------------------------------------------------------------------------------------------ 3. bit for bit
@pytest.mark.parametrize('name', TWICE_ROWS)
def test_two_launches_give_identical_bits(A, ctx, name):
    case = T.build(name)
    same_bits(run_row(A, ctx, case), run_row(A, ctx, case), name)


# ------------------------------------------------------------------------------------------------------------------ 4. slice positions
@pytest.mark.parametrize('name', Z_ROWS)
def test_slice_position_values_vs_restatement(A, ctx, name):
    """A zero gap, a negative gap and the ladder of gaps up to its top rung, by the sparse module's rule."""
    case = T.build(name)
    r64, r32, e32 = T.yardstick(name)
    assert e32[4] >= T.MIN_YARDSTICK, e32[4]
    judge(case, run_row(A, ctx, case), r64, r32, e32, name)


@pytest.mark.parametrize('base,moved', MOVED_PAIRS)
def test_moving_every_slice_by_1_cm_changes_no_bit(A, ctx, base, moved):
    """z + 1 cm is exact in float32 for these positions, so the device sees the same gaps."""
    a, b = T.build(base), T.build(moved)
    assert np.array_equal(np.diff(b['z'].astype(np.float64)), np.diff(a['z'].astype(np.float64))) and np.all(b['z'] >= 1)
    same_bits(run_row(A, ctx, b), run_row(A, ctx, a), moved)
