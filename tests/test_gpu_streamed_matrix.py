"""Every launch geometry of the streamed multislice path (adm_ms_streamed.hip) up to 2048 x 2048 against the fp64 oracle
(pytest -m gpu).  tests/st_matrix.py holds the fields, the classes of geometry they reach and the launch-sequence variants;
tests/test_streamed_matrix_coverage.py ties those tables to the kernel source.

Judged twice: by ms_matrix.check with the GENERIC bars (whole arrays, by norm), and band by band along the launch geometry --
every row workgroup's rows and every column workgroup's columns of the prediction and of the probe gradient on their own, by
the 3x rule with the oracle's fp32 run on the same band as the yardstick.  An error confined to the last, ragged group of a
2048-wide field is diluted by sqrt(4 / 2048) in a norm over the whole array; in its own band it is not.

CPU time of the oracle runs (fp64 and fp32; every case is built once per module, _CASES), measured on 8 cores with
`python -m tests.test_gpu_streamed_matrix` and the like: 2048 x 2048 (S = 2, B = 4) 26 s, 1536 x 1280 (S = 2, B = 4, 2 modes)
18 s, 1024 x 1024 5 s, every other field under 2.5 s -- 64 s for the 22 fields; the 40 sequence cases 59 s; the sparse cases'
restatement 23 s (1536 x 1280: 19 s): 2.5 minutes.  On 16 cores the whole module, GPU work included, takes 53 s.
"""
import time

import numpy as np
import pytest

from tests import ms_matrix as MM
from tests import st_matrix as SM
from tests.test_gpu_streamed_multislice import run_streamed
from tests import test_gpu_sparse_multislice as SP

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


def oracle_case(P, **kw):
    """MM.oracle_case, built once per module."""
    key = (P, tuple(sorted((k, str(v)) for k, v in kw.items())))
    if key not in _CASES:
        _CASES[key] = MM.oracle_case(P, **kw)
    return _CASES[key]


def sparse_case(name):
    """make_case and its yardstick (fp64 restatement, distances of its fp32 run), built once per module."""
    key = ('sparse', name)
    if key not in _CASES:
        kw = dict(SM.SPARSE_CASES[name])
        case = SP.make_case(kw.pop('P'), **kw)
        _CASES[key] = (case,) + SP.yardstick(case)
    return _CASES[key]


# ------------------------------------------------------------------------------------------------------------ band-wise bars
def _band_sums(a, axis, bands, shift):
    """Sums of the non-negative [Py, Px] array ``a`` over every band of ``axis`` (None: the bands are intervals of the flattened
    index ky * Px + kx).  ``shift``: the bands are intervals of the natural-order spectrum index k, which the far-field detector
    shows at pixel (k + N/2) % N."""
    if axis is None:
        if shift:
            a = np.roll(a, (-(a.shape[0] // 2), -(a.shape[1] // 2)), (0, 1))      # a[ky, kx] <- detector pixel ((ky + Py/2) % Py, ...)
        line = a.reshape(-1)
    else:
        line = a.sum(1 - axis)
        if shift:
            line = np.roll(line, -(len(line) // 2))           # line[k] <- detector pixel (k + N/2) % N
    return np.add.reduceat(line, [lo for lo, _ in bands])


def geometry_bands(shape):
    """The band sets of the streamed path: (name, axis, bands) of the row workgroups' rows and the column workgroups' columns."""
    return (('row', 0, SM.row_bands(*shape)), ('col', 1, SM.col_bands(*shape)))


def band_errors(x, x64, x32, shape, shifted, band_sets=None):
    """Per band set (default: row groups, then column groups): the relative distance of ``x`` and of the oracle's fp32 run from
    the fp64 oracle on every band, and which bands carry enough signal to be judged.  Arrays are [..., Py, Px]; ``band_sets``
    holds (name, axis, bands), the bands tiling the axis (axis None: the flattened field) from 0 to its end."""
    Py, Px = shape
    sq = lambda d: (np.abs(d) ** 2).reshape(-1, Py, Px).sum(0)
    d, d32, n64 = sq(np.asarray(x) - x64), sq(np.asarray(x32) - x64), sq(x64)
    out = []
    for _, axis, bands in (geometry_bands(shape) if band_sets is None else band_sets):
        n = _band_sums(n64, axis, bands, shifted)
        judged = n >= 1e-6 * n.max()                              # norm >= 1e-3 of the largest band's
        with np.errstate(divide='ignore', invalid='ignore'):
            e = np.sqrt(_band_sums(d, axis, bands, shifted) / n)
            e32 = np.sqrt(_band_sums(d32, axis, bands, shifted) / n)
        out.append((e, e32, judged))
    return out


def check_bands(res, what, band_sets=None, bars=BARS, without_signal=0.05, each=False):
    """The 3x rule on every band: prediction (floor bars['pred']) and probe gradient (floor bars['grad_abs'], and below
    bars['grad']).  ``band_sets``: as for band_errors; ``without_signal``: the share of a set's bands that may be without signal;
    ``each``: every position's prediction and every mode's probe gradient on its own instead of their sums."""
    shape, far = res['kw']['shape'], res['kw']['free_prop'] == 'inf'
    sets = geometry_bands(shape) if band_sets is None else band_sets
    worst = {}
    for name, floor, cap, shifted in (('pred', bars['pred'], None, far), ('gprobe', bars['grad_abs'], bars['grad'], False)):
        if res.get(name) is None:
            continue                                              # (per-position probes: no probe gradient is formed)
        arrays = [res[name], res[name + '_o'], res[name + '_32']]
        items = [(name, arrays)] if not each else [('%s[%d]' % (name, k), [a[k] for a in arrays]) for k in range(len(arrays[0]))]
        for item, (x, x64, x32) in items:
            for (axis, _, _), (e, e32, judged) in zip(sets, band_errors(x, x64, x32, shape, shifted, sets)):
                assert (~judged).sum() <= without_signal * len(judged), (what, item, axis, 'bands without signal', int((~judged).sum()), len(judged))
                margin = np.where(judged, e - (3 * e32 + floor), -np.inf)
                k = int(np.argmax(margin))
                if (name, axis) not in worst or e[k] - 3 * e32[k] > worst[name, axis][2] - 3 * worst[name, axis][3]:
                    worst[name, axis] = (k, len(e), float(e[k]), float(e32[k]))
                if not each:
                    print('%s %s %s bands: worst %d of %d: %.2e (fp32 oracle %.2e)' % ((what, name, axis) + worst[name, axis]))
                assert margin[k] <= 0, (what, item, axis, 'band %d of %d' % (k, len(e)), e[k], e32[k])
                if cap is not None:
                    assert e[judged].max() < cap, (what, item, axis, e[judged].max())
    if each:
        for (name, axis), w in worst.items():
            print('%s %s %s bands: worst %d of %d: %.2e (fp32 oracle %.2e)' % ((what, name, axis) + w))
    return worst


def judge(res, what):
    assert res['streamed']
    print('%s: pred %.2e (fp32 oracle %.2e)  loss %.2e  grad %.2e (%.2e)  gprobe %.2e (%.2e)' % (
        what, MM.rel(res['pred'], res['pred_o']), MM.rel(res['pred_32'], res['pred_o']), abs(res['loss'] / res['loss_o'] - 1),
        MM.rel(res['grad'], res['grad_o']), MM.rel(res['grad_32'], res['grad_o']),
        MM.rel(res['gprobe'], res['gprobe_o']), MM.rel(res['gprobe_32'], res['gprobe_o'])))
    # the case itself must be well-conditioned: where the oracle's own fp32 run misses a third of the cap on the gradients, the
    # 3x rule and the cap contradict each other and the test would measure the data, not the kernels
    for k in ('grad', 'gprobe'):
        assert MM.rel(res[k + '_32'], res[k + '_o']) < BARS['grad'] / 3, (what, k, 'ill-conditioned case')
    MM.check(res, BARS)
    check_bands(res, what)


# ---------------------------------------------------------------------------------------------------- a, b. shapes
@pytest.mark.parametrize('shape', sorted(SM.SHAPES, key=lambda s: (s[0] * s[1], s)), ids=lambda s: '%dx%d' % s)
def test_shapes_vs_oracle(A, ctx, shape):
    """Every field of st_matrix.SHAPES, in ascending size: prediction, loss, object gradient and probe gradient against the fp64
    oracle by the GENERIC bars, then the prediction and the probe gradient band by band."""
    res = run_streamed(A, ctx, oracle_case(shape, **SM.SHAPES[shape]))
    judge(res, '%dx%d' % shape)


# ---------------------------------------------------------------------------------------------------- c. launch sequences
@pytest.mark.parametrize('name,cls', SM.SEQUENCE_CASES)
def test_sequences_vs_oracle(A, ctx, name, cls):
    """Every launch-sequence variant of ms_streamed_launch at a field of 320 threads x 8 columns and at one of 4 columns.
    Forward-only launches: prediction and loss are the full launch's bit for bit and no gradient buffer is written."""
    kw, forward_only = SM.sequence_kw(name)
    case = oracle_case(SM.SEQUENCE_SHAPES[cls], **kw)
    full = run_streamed(A, ctx, case)
    judge(full, '%s %s' % (name, cls))
    if forward_only:
        fwd = run_streamed(A, ctx, case, want_grad=False)
        assert fwd['streamed']
        assert fwd['loss'] == full['loss'] and np.array_equal(fwd['pred'], full['pred'])
        assert np.all(fwd['gprobe_raw'] == 3) and np.all(fwd['grad_rot'] == 5)


# ---------------------------------------------------------------------------------------------------- d. sparse, dL/dz
@pytest.mark.parametrize('name', list(SM.SPARSE_CASES))
def test_sparse_vs_restatement(A, ctx, name):
    """Sparse multislice with the slice-position gradient at the new geometries (odd sides, 39 gaps, thousands of partials per
    gap), by the 3x rule of tests/test_gpu_sparse_multislice.py.  As there, the restatement's own fp32 dL/dz error must be at
    least 1e-6, so that the test measures the kernels and not the rounding of the fp32 output."""
    case, r64, e32 = sparse_case(name)
    assert e32[4] >= 1e-6, e32[4]
    SP.check_3x(SP.run_sparse(A, ctx, case), r64, e32, e32[4], name)


# ---------------------------------------------------------------------------------------------------- e. consistency
def transposed(case):
    """The same problem with its two axes exchanged: object, positions, probes, data (and the oracle's results)."""
    t = dict(case)
    t['obj'] = np.ascontiguousarray(case['obj'].transpose(1, 0, 2, 3))
    t['pos'] = np.ascontiguousarray(case['pos'][:, ::-1])
    for k in ('probes', 'target', 'pred_o', 'pred_32', 'gprobe_o', 'gprobe_32'):
        t[k] = np.ascontiguousarray(np.swapaxes(case[k], -1, -2))
    for k in ('grad_o', 'grad_32'):
        t[k] = np.ascontiguousarray(case[k].transpose(1, 0, 2, 3))
    assert case['beamstop'] is None
    t['kw'] = dict(case['kw'], shape=case['kw']['shape'][::-1])
    return t


@pytest.mark.regression
@pytest.mark.parametrize('shape', [(1152, 12), (2048, 5)], ids=lambda s: '%dx%d' % s)
def test_transposed_problem_agrees(A, ctx, shape):
    """Exchanging the axes of the whole problem turns a field of 4 columns per workgroup into one of 8, and ragged row groups
    into ragged column groups: loss, prediction and gradients agree to the 1e-5 of test_streamed_matches_lds_kernels."""
    case = oracle_case(shape, S=3, B=5, n_modes=2, seed=7)
    a, b = run_streamed(A, ctx, case), run_streamed(A, ctx, transposed(case))
    assert SM.geometry(*shape)['cw'] == 4 and SM.geometry(*shape[::-1])['cw'] == 8
    assert abs(b['loss'] - a['loss']) <= 1e-5 * abs(a['loss']), (a['loss'], b['loss'])
    assert MM.rel(np.swapaxes(b['pred'], -1, -2), a['pred']) < 1e-5
    assert MM.rel(b['grad'].transpose(1, 0, 2, 3), a['grad']) < 1e-5
    for m in range(2):
        assert MM.rel(b['gprobe'][m].T, a['gprobe'][m]) < 1e-5, m
    judge(b, '%dx%d transposed' % shape)


@pytest.mark.regression
def test_two_launches_give_identical_bits_at_four_columns(A, ctx):
    case = oracle_case((1025, 132), S=3, B=5, n_modes=3)
    a, b = run_streamed(A, ctx, case), run_streamed(A, ctx, case)
    assert a['loss'] == b['loss']
    for k in ('pred', 'grad', 'gprobe'):
        assert np.array_equal(a[k], b[k]), k


@pytest.mark.regression
def test_rounds_within_workspace_budget_at_four_columns(A, ctx):
    """A batch of 5 in three rounds at 1025 x 132 (test_streamed_rounds_within_workspace_budget at 256)."""
    shape = (1025, 132)
    case = oracle_case(shape, S=3, B=5, n_modes=3)
    one = run_streamed(A, ctx, case)
    Y, X, S = case['obj'].shape[:3]
    probe_eng = A.MultisliceEngine(ctx, (Y, X, S), shape, case['pos'], MM.ENERGY_EV, MM.PSIZE_CM, n_probe_modes=3, streamed=True)
    budget = probe_eng.plan.workspace_bytes(2)
    probe_eng.plan.close()
    parts = run_streamed(A, ctx, case, workspace_budget=budget)
    assert one['n_rounds'] == 1 and parts['n_rounds'] == 3
    judge(parts, 'rounds')
    assert parts['loss'] == one['loss']
    assert np.array_equal(parts['pred'], one['pred'])
    assert MM.rel(parts['gprobe'], one['gprobe']) < 1e-6
    assert MM.rel(parts['grad'], one['grad']) < 1e-6


# ---------------------------------------------------------------------------------------------------- f. refusals at the edge
def _engine(A, ctx, shape, **kw):
    Py, Px = shape
    return A.MultisliceEngine(ctx, (Py + 6, Px + 6, 2), shape, np.array([(0, 0), (3, 5)]), MM.ENERGY_EV, MM.PSIZE_CM, max_batch=2,
                              streamed=True, **kw)


def test_sides_at_the_edge(A, ctx):
    """2049 in either axis is refused with a message; 2048 x 1 and 1 x 2048 are accepted and run (against the oracle)."""
    for shape in ((2049, 8), (8, 2049), (2049, 2049)):
        with pytest.raises(NotImplementedError, match='at most 2048'):
            _engine(A, ctx, shape)
    for shape in ((2048, 1), (1, 2048)):      # (B = 8: the four corner positions of a one-pixel-wide tile miss the object altogether)
        judge(run_streamed(A, ctx, oracle_case(shape, S=2, B=8)), '%dx%d' % shape)


def test_most_slice_positions(A, ctx):
    """A sparse plan of ST_MAX_SLICES + 1 slice positions is refused with a message; one of exactly ST_MAX_SLICES is accepted
    and runs at an 8 x 8 field (1023 gaps in st_dd_reduce_kernel's LDS) against the restatement, whose two runs take a few
    seconds; st_sparse_anchor_kernel moves all 1024 positions."""
    n = SM.ST_MAX_SLICES
    pos = np.array([(0, 0), (3, 5)])
    with pytest.raises(NotImplementedError, match='more than %d slice positions' % n):
        A.MultisliceEngine(ctx, (14, 14, n + 1), (8, 8), pos, SP.ENERGY_EV, SP.PSIZE_CM, max_batch=2,
                           slice_pos_cm=np.arange(n + 1) * 1e-4)
    key = ('sparse', 'most')
    if key not in _CASES:
        case = SP.make_case(8, S=n, B=4, seed=9)
        # (gaps of 3 - 30 um add up to 1.7 cm over 1023 gaps: shortened to 0.03 - 0.3 um, the total depth of the other cases)
        case['z'] = (case['z'] * 1e-2).astype(np.float32)
        _CASES[key] = (case,) + SP.yardstick(case)
    case, r64, e32 = _CASES[key]
    res = SP.run_sparse(A, ctx, case, keep_engine=True)
    eng = res.pop('engine')
    assert e32[4] >= 1e-6, e32[4]                          # (2.4e-5: the rule of test_engine_sizes_vs_restatement)
    SP.check_3x(res, r64, e32, e32[4], 'S=%d' % n)
    eng.slice_pos.set((case['z'] + np.float32(0.25)).astype(np.float32))
    eng.anchor_slice_pos()
    z = eng.slice_pos.get()
    eng.plan.close()
    assert np.array_equal(z, (case['z'] + np.float32(0.25)) - (case['z'][0] + np.float32(0.25)))


if __name__ == '__main__':      # the CPU time of the module's oracle runs, and the band condition from the oracle alone
    total = 0.
    for shape in sorted(SM.SHAPES, key=lambda s: (s[0] * s[1], s)):
        t = time.time()
        c = oracle_case(shape, **SM.SHAPES[shape])
        dt = time.time() - t
        total += dt
        far = c['kw']['free_prop'] == 'inf'
        low = [int((~j).sum()) for n, s in (('pred', far), ('gprobe', False)) for _, _, j in band_errors(c[n + '_32'], c[n + '_o'], c[n + '_32'], shape, s)]
        print('%-12s %6.1f s   pred fp32 %.2e   bands without signal %s' % ('%dx%d' % shape, dt, MM.rel(c['pred_32'], c['pred_o']), low), flush=True)
    print('shapes: %.0f s' % total)
