"""The table of tests/smallgrad_matrix.py held to the pinned oracle, to finite differences and to its own rules (no GPU).

* neutral parameters (gaps equal to the voxel spacing, offsets of exactly zero, one distance at a time): under every option the
  extended restatements return what O.forward_adjoint_tiles returns with the same options -- which ties their new loss arguments
  to the oracle the goldens hold;
* finite differences: dL/dz, dL/ds and dL/dd of every row against central differences of the restatement's own loss in fp64, and
  the mistakes each row guards against (the mask ignored, the LSQ cotangent under the Poisson loss, ...) at least ten bars away;
* yardsticks: every row's float32 restatement well inside ms_matrix.GENERIC and, on the small gradient, above the rounding of a
  float32 output;
* count: every option x path x mode count exactly once, and the GPU module names only rows of the table.
"""
import numpy as np
import pytest

from oracle import adorym_oracle as O
from tests import ms_matrix as MM
from tests import smallgrad_matrix as T
from tests import sparse_ref as SR
from tests import prj_offset_ref as PR
from tests import multidist3d_ref as MR
from tests import multidist3d_dist_ref as DR

rel = MM.rel
REFERENCE_ROWS = [n for n, r in T.ROWS.items() if r['kind'] == 'reference']
IDENTITY_ROWS = [n for n, r in T.ROWS.items() if r['kind'] == 'identity']


# ------------------------------------------------------------------------------------------------------------------ count
def test_every_option_path_and_mode_count_once():
    want = sorted((p, o, M) for p in T.PATHS for o in T.PATH_OPTIONS[p] for M in T.MODE_COUNTS)
    have = sorted((r['path'], r['option'], r['M']) for r in T.ROWS.values())
    assert have == want and len(T.ROWS) == len(want) == 40
    assert set(T.PATH_OPTIONS['sparse']) == set(T.PATH_OPTIONS['exit_shift']) == set(T.OPTIONS)
    assert set(T.OPTIONS) - set(T.PATH_OPTIONS['fanout']) == {'real_imag_poisson'}
    # the detectors of the shapes table: all three in front of the sparse path, Fresnel and exit wave behind the offsets
    assert {r['det'] for r in T.ROWS.values() if r['path'] == 'sparse'} == {'inf', T.FRESNEL_CM, 0}
    assert {r['det'] for r in T.ROWS.values() if r['path'] == 'exit_shift'} == {T.PO.FREE_PROP_CM, 0}
    # normalize_fft acts on a far-field detector only
    for n, r in T.ROWS.items():
        assert (r['kind'] == 'identity') == (r['option'] == 'ortho' and r['det'] != 'inf'), n
    assert sorted(T.settings(r['kw'].get('option_of', r['option']))['loss'] for r in T.FAR_ROWS.values()) == ['lsq', 'poisson']
    assert all(r['det'] == 'inf' for r in T.FAR_ROWS.values())


def test_shapes_are_the_smallest_with_a_clipped_last_column_group():
    geo = T.FM.SM.geometry(*T.FIELD)
    assert T.FIELD == (24, 20) and geo['cw'] == 8 and geo['cw_last'] == 4
    for name in list(T.ROWS) + list(T.FAR_ROWS):
        c = T.build(name)
        path = c['row']['path']
        assert c['probes'].shape == (c['row']['M'],) + T.FIELD
        assert (c['obj'].shape[2], len(c['pos'])) == {'sparse': (3, 3), 'exit_shift': (2, 5), 'fanout': (2, 3)}[path], name
        if path == 'exit_shift':
            assert list(c['index']) == [0, 1, 2, 1, 0] and c['shifts'].shape == (3, 2)
        if path == 'fanout':
            assert len(c['dists']) == 3 and not any(T.FM.phase_step_at_nyquist(d, T.FIELD) > 1 for d in c['dists'])
    for name in T.Z_ROWS:
        assert T.build(name)['obj'].shape[2] == 4


def test_gpu_module_names_only_rows_of_the_table():
    from tests import test_gpu_smallgrad_options as G
    named = G.OPTION_ROWS + G.IDENTITY_ROWS + G.FAR_ROWS + G.MASKED_ROWS + G.TWICE_ROWS + G.Z_ROWS + G.ZERO_ROWS + [n for pair in G.MOVED_PAIRS for n in pair]
    assert all(n in T.ALL_ROWS for n in named)
    assert sorted(G.OPTION_ROWS) == sorted(REFERENCE_ROWS) and sorted(G.IDENTITY_ROWS) == sorted(IDENTITY_ROWS)
    assert sorted(G.FAR_ROWS) == sorted(T.FAR_ROWS) and sorted(G.ZERO_ROWS) == sorted(T.ZERO_ROWS)
    assert sorted(G.MASKED_ROWS) == sorted(n for n in REFERENCE_ROWS if T.build(n)['beamstop'] is not None)
    assert sorted(G.Z_ROWS + [m for _, m in G.MOVED_PAIRS]) == sorted(T.Z_ROWS)
    assert {T.ROWS[n]['path'] for n in G.TWICE_ROWS} == set(T.PATHS) and all(T.build(n)['loss'] == 'poisson' for n in G.TWICE_ROWS)


# ------------------------------------------------------------------------------------------------------------------ neutral parameters
def _close(a, b, what):
    e = rel(a, b)
    assert e <= T.NEUTRAL, (what, e)


@pytest.mark.parametrize('name', list(T.PLAIN_ROWS) + list(T.ROWS))
def test_neutral_parameters_reproduce_the_oracle(name):
    case = T.build(name)
    path = case['row']['path']
    phys = T.physics(case)
    kw = T.loss_kw(case)
    tiles, _ = O.extract_tiles(case['obj'].astype(np.float64), case['pos'], T.FIELD, case['unknown_type'])
    probes = case['probes'].astype(np.complex128)
    if path == 'sparse':
        S = tiles.shape[3]
        got = SR.forward_adjoint_tiles(tiles, probes, case['meas'], phys, np.arange(S) * T.PSIZE_CM, **kw)
        want = O.forward_adjoint_tiles(tiles, probes, case['meas'], phys, **kw)
        for k, g, w in zip(('loss', 'pred', 'grad_tiles', 'grad_probes'), got, want):
            _close(g, w, (name, k))
    elif path == 'exit_shift':
        got = PR.forward_adjoint_tiles(tiles, probes, case['meas'], phys, np.zeros((3, 2)), case['index'], **kw)
        want = O.forward_adjoint_tiles(tiles, probes, case['meas'], phys, **kw)
        for k, g, w in zip(('loss', 'pred', 'grad_tiles', 'grad_probes'), got, want):
            _close(g, w, (name, k))
    else:
        D = len(case['dists'])
        for d, dist in enumerate(case['dists']):
            one = O.Physics(T.FIELD, T.ENERGY_EV, T.PSIZE_CM, free_prop_cm=dist, sign_convention=case['sign_convention'],
                            normalize_fft=case['normalize_fft'])
            want = O.forward_adjoint_tiles(tiles, probes, case['meas'][d::D], one, **kw)
            got = MR.forward_adjoint_tiles(tiles, probes, case['meas'][d::D], phys, [dist], **kw)
            for k, g, w in zip(('loss', 'pred', 'grad_tiles', 'grad_probes'), got, want):
                _close(g, w, (name, d, k))
            dd = DR.forward_dist_grad(tiles, probes, case['meas'][d::D], phys, [dist], **kw)
            _close(dd[0], want[0], (name, d, 'loss of the distance restatement'))
            _close(dd[1], want[1], (name, d, 'pred of the distance restatement'))


def test_the_far_field_restatement_has_no_offset_gradient():
    for name in T.FAR_ROWS:
        r = T.ref(T.build(name))
        assert np.all(r['small'] == 0) and np.isfinite(r['loss'])


@pytest.mark.parametrize('name', IDENTITY_ROWS)
def test_normalize_fft_cannot_act_behind_a_fresnel_or_exit_wave_detector(name):
    case = T.build(name)
    on, off = T.ref(case), T.ref(case, normalize_fft=False)
    for k in on:
        assert np.array_equal(np.asarray(on[k]), np.asarray(off[k])), (name, k)


# ------------------------------------------------------------------------------------------------------------------ finite differences
@pytest.mark.parametrize('name', list(T.PLAIN_ROWS) + REFERENCE_ROWS)
def test_small_gradients_vs_finite_differences(name):
    case = T.build(name)
    path = case['row']['path']
    g = T.yardstick(name)[0]['small']
    fd = T.central_differences(case, T.FD_STEP[path])
    n = np.linalg.norm(fd)
    e = np.linalg.norm(g - fd) / n
    bar = T.FD_PLAIN if name in T.PLAIN_ROWS else T.FD_OPTION
    print(name, 'finite differences %.2e (bar %.0e)' % (e, bar))
    assert n > 0 and e <= bar, (name, e)
    muts = T.mutants(case)
    assert (name in T.PLAIN_ROWS) == (not muts), name              # every option row shows the mistake it guards against
    for what, over in muts.items():
        em = np.linalg.norm(T.ref(case, **over)['small'] - fd) / n
        print(name, what, '%.2e' % em)
        assert em >= T.FD_MUTANT, (name, what, em)


# ------------------------------------------------------------------------------------------------------------------ yardsticks
JUDGED_Z_ROWS = [n for n, r in T.Z_ROWS.items() if r['kw']['z'] in ('base', 'zero_gap', 'negative_gap')]


@pytest.mark.parametrize('name', REFERENCE_ROWS + JUDGED_Z_ROWS)
def test_fp32_yardsticks(name):
    """The float32 restatement on every row: a third of GENERIC's bars at most for what has bars, MIN_YARDSTICK at least on the
    small gradient.  (The ladder rows are there to leave that range; 'moved_1cm' is compared with 'base' bit for bit.)"""
    e = T.yardstick(name)[2]
    B = MM.GENERIC
    print(name, 'pred %.1e loss %.1e grad %.1e gprobe %.1e small %.2e' % tuple(e[:5]))
    assert e[0] <= T.YARD_FRACTION * B['pred'] and e[1] <= T.YARD_FRACTION * B['loss'], (name, e)
    assert e[2] <= T.YARD_FRACTION * B['grad'] and e[3] <= T.YARD_FRACTION * B['grad'], (name, e)
    assert e[4] >= T.MIN_YARDSTICK, (name, e[4])


# ------------------------------------------------------------------------------------------------------------------ slice positions
def test_slice_position_values():
    z = {k: np.asarray(v, np.float32) for k, v in T.Z_VALUES.items()}
    assert np.any(np.diff(z['zero_gap']) == 0) and np.any(np.diff(z['negative_gap']) < 0)
    assert np.array_equal(z['base'].astype(np.float64), T.Z_VALUES['base']) and np.array_equal(z['moved_1cm'].astype(np.float64), T.Z_VALUES['moved_1cm'])
    assert np.array_equal(np.diff(z['moved_1cm'].astype(np.float64)), np.diff(z['base'].astype(np.float64)))      # the same gaps, exactly
    for o in T.Z_LOSSES:
        a, b = T.build('sparse-z-base-' + o), T.build('sparse-z-moved_1cm-' + o)
        for k in ('obj', 'pos', 'probes', 'meas', 'target'):
            assert np.array_equal(a[k], b[k]), k


@pytest.mark.parametrize('loss', T.Z_LOSSES)
def test_the_top_rung_of_the_gap_ladder(loss):
    """The float32 restatement's own dL/dz error stays at or below LADDER_BAR up to the top rung and is above it one rung further."""
    rungs = T.LADDER[loss]
    assert all(b == 10 * a for a, b in zip(rungs, rungs[1:])) and rungs[0] == 10
    for k in rungs:
        e = T.yardstick('sparse-z-gaps_x%d-%s' % (k, loss))[2][4]
        print(loss, 'gaps x%d: %.2e' % (k, e))
        assert T.MIN_YARDSTICK <= e <= T.LADDER_BAR, (loss, k, e)
    e = T.yardstick('sparse-z-gaps_x%d-%s' % (10 * rungs[-1], loss))[2][4]
    print(loss, 'gaps x%d: %.2e' % (10 * rungs[-1], e))
    assert e > T.LADDER_BAR, (loss, e)


# ------------------------------------------------------------------------------------------------------------------ zero predictions
@pytest.mark.parametrize('name', list(T.ZERO_ROWS))
def test_zero_rows_have_nothing_to_predict_outside_the_disc(name):
    """Both probes exactly zero outside the disc and nothing that moves the field sideways: the fp64 restatement's prediction
    there is the rounding of a transform pair.  With those pixels under the mask it is finite in fp64 and in fp32."""
    case = T.build(name)
    out = ~T.disc()
    assert np.all(case['probes'][:, out] == 0) and np.all(np.abs(case['probes'][:, ~out]) > 0)
    masked = T.with_mask(case, T.zero_mask())
    r64, r32 = T.ref(masked), T.ref(masked, 'float32')
    print(name, 'largest prediction outside the disc %.1e of %.1e' % (r64['pred'][:, out].max(), r64['pred'].max()))
    assert r64['pred'][:, out].max() <= 1e-12 * r64['pred'].max()
    for r in (r64, r32):
        assert all(np.all(np.isfinite(np.asarray(v))) for v in r.values())
    assert np.linalg.norm(r64['small']) > 0
