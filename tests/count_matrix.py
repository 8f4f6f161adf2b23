"""The COUNT axis of the multislice paths (test infrastructure only): batch sizes, probe-mode counts and shift-entry counts beyond what
the shape matrices run (tests/ms_matrix.py and its users hold B <= 11 and M <= 3 against the oracle).

* mirrors of the arithmetic that changes with the counts: ``xcd_position`` (adm_multislice.hip), ``pgr_chunks`` and ``uses_slots``
  (adm_api.hip), ``loss_reduce_workgroups`` and the trip counts of st_shift_reduce_kernel (adm_ms_streamed.hip).  The coverage
  test (tests/test_count_domain_coverage.py) parses the sources and fails when one of them moves away from its mirror.
* ``CASES``: one row per case with the fields the smallest at which its class exists (8 x 8 for the tuned kernels, 33 x 31 for the
  any-size kernel, 24 x 24 / 24 x 20 for the streamed path); ``classes_of`` computes from B, M, the column geometry and the index
  which side of every threshold a case is on.
* ``INDEX_PATTERNS``: the shift-entry indices of the large shift cases, as ``index_fn`` of ms_matrix.oracle_case.
* positions are spread with oracle_case's ``margin`` (``spread_margin``) so that no padded pixel is covered by more than 64 tiles
  (``cover_max``); ONE case (DENSE) keeps the default margin and runs through the engine's overflow passes.
* ``check_counts``: every position's prediction and loss sum, every mode's probe gradient and every entry's shift gradient on its
  own, under the band rule of the other matrices (3 x the fp32 oracle on the same item + the whole-array bar).
"""
import functools
import os
import re

import numpy as np

from tests import ms_matrix as MM
from tests import st_matrix as SM
from tests import prj_offset_ref as PR
from tests import sparse_ref as SR

O = MM.O
CSRC = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), 'adorym_amd', 'csrc')

# what the sources hold (compared with them by the coverage test)
PGR_CHUNK = 32          # adm_api.hip
SLOT_PAIRS = 256        # adm_probe_shift_adj: slots beyond this many (position, mode) pairs
MAX_MODES = 64          # adm_plan_create
RED_NT = 256            # st_loss_reduce_kernel's positions per workgroup, the strides of st_shift_reduce_kernel's two loops
MAX_COVER = 64          # ADM_MAXCOVER of adm_host.h


# ---------------------------------------------------------------------------------------------------------------- mirrors
def xcd_position(wg, B):
    """Position of workgroup ``wg`` of a launch of B (adm_multislice.hip)."""
    k, slot = wg & 7, wg >> 3
    q, r = B >> 3, B & 7
    return k * q + min(k, r) + slot


def pgr_chunks(batch, chunk=PGR_CHUNK):
    """[first, end) slots of every chunk of probe_grad_reduce_large; the second level adds the first slots in chunk order."""
    chunks = (batch + chunk - 1) // chunk
    return [(c * chunk, min(c * chunk + chunk, batch)) for c in range(chunks)]


def uses_slots(B, M):
    return B * M > SLOT_PAIRS


def loss_reduce_workgroups(B):
    return (B + RED_NT - 1) // RED_NT


def shift_reduce_trips(b, per):
    """Trips of thread 0 through the two loops of st_shift_reduce_kernel's workgroup b: the search of index[0 .. b) for an
    earlier user of the entry, and the sum over the ``per`` = M * column groups partials of a position."""
    return -(-b // RED_NT), -(-per // RED_NT)


def cover_max(pos, P):
    """How many tiles cover the most-covered pixel."""
    Py, Px = (P, P) if np.isscalar(P) else P
    pos = np.asarray(pos)
    y0, x0 = pos[:, 0] - pos[:, 0].min(), pos[:, 1] - pos[:, 1].min()
    d = np.zeros((int(y0.max()) + Py + 1, int(x0.max()) + Px + 1), np.int64)
    for dy, dx, s in ((0, 0, 1), (Py, 0, -1), (0, Px, -1), (Py, Px, 1)):
        np.add.at(d, (y0 + dy, x0 + dx), s)
    return int(d.cumsum(0).cumsum(1).max())


def spread_margin(P, B):
    """oracle_case's ``margin`` for B positions of a P field: the default up to MAX_COVER positions (they cannot cover a pixel more
    often than that), else the smallest square one whose (margin + 7)^2 corners hold the batch at a mean cover of 24 -- a
    uniform draw then stays below 64 (cover_max of every case is asserted by the coverage test)."""
    if B <= MAX_COVER:
        return (9, 13)
    Py, Px = (P, P) if np.isscalar(P) else P
    m = int(np.ceil(np.sqrt(B * Py * Px / 24.))) - 7
    return (m, m)


# ---------------------------------------------------------------------------------------------------------------- index patterns
def _idx_none(B):
    return B, None


def _idx_identity(B):
    return B, np.arange(B)


def _idx_reversed(B):
    return B, np.arange(B)[::-1].copy()


def _idx_one_entry(B):
    return 3, np.full(B, 1)          # entries 0 and 2 are not used


def _idx_mixed(B):
    """16 entries: entry 0 is used by position 0 and position B - 1 only; entries 2 and 3 by nobody; entry 5 by positions 256, 258
    and B - 2 only, entries 12 ... 15 by the pairs (257, 259), (260, 262), (261, 263), (264, 266) only -- their first users and the
    search for them lie beyond the first 256 positions (five such entries: a search that misses the first user makes two workgroups
    add to one entry, and which of the two sums survives that race is open for each).  Below B = 270 there is no room for that:
    entry 5 goes to positions B - 3 and B - 2, entries 12 ... 15 to nobody.  The rest go round 1, 4, 6 ... 11."""
    assert B >= 16
    rest = np.array([1, 4, 6, 7, 8, 9, 10, 11])
    idx = rest[np.arange(B) % len(rest)]
    idx[[0, B - 1]] = 0
    if B >= 270:
        idx[[256, 258, B - 2]] = 5
        for e, pair in zip((12, 13, 14, 15), ((257, 259), (260, 262), (261, 263), (264, 266))):
            idx[list(pair)] = e
    else:
        idx[[B - 3, B - 2]] = 5
    return 16, idx


INDEX_PATTERNS = {'none': _idx_none, 'identity': _idx_identity, 'reversed': _idx_reversed, 'one_entry': _idx_one_entry, 'mixed': _idx_mixed}


def index_of(case):
    """(n_entries, index [B]) of a built case (an index of None spelled out)."""
    B = case['kw']['B']
    return len(case['shifts']), (np.arange(B) if case['idx'] is None else np.asarray(case['idx']))


# ---------------------------------------------------------------------------------------------------------------- cases
FRESNEL, DISTS = 1e-4, (1e-4, 2e-4, 3.5e-4)
DENSE = 'tuned_B300_dense'


def _row(name, family, P, index=None, **kw):
    return name, dict(family=family, P=P, index=index, kw=kw)


def _cases():
    rows = []
    # tuned, B (8 x 8, S = 2): q = 0; r = 7; r = 0; q = 1, r = 1; q = 2, r = 0; r = 7 with q > 0; a second round of workgroups
    for B in (1, 7, 8, 9, 16, 23, 257):
        rows.append(_row('tuned_B%d' % B, 'tuned', 8, S=2, B=B))
    rows.append(_row(DENSE, 'tuned', 8, S=2, B=300, margin=(9, 13)))             # cover > 64: the overflow passes
    # tuned, M: the MULTI branch on its act2 (far field) and act1 (Fresnel) sides, odd R1, four waves, the other two modes
    for M in (4, 64):
        rows.append(_row('tuned_M%d_far' % M, 'tuned', 8, S=2, B=5, n_modes=M))
        rows.append(_row('tuned_M%d_fresnel' % M, 'tuned', 8, S=2, B=5, n_modes=M, free_prop=FRESNEL))
    rows.append(_row('tuned_M8_P27', 'tuned', 27, S=2, B=5, n_modes=8))
    rows.append(_row('tuned_M8_P32', 'tuned', 32, S=2, B=5, n_modes=8))
    rows.append(_row('tuned_M4_real_imag', 'tuned', 8, S=2, B=5, n_modes=4, unknown_type='real_imag'))
    rows.append(_row('tuned_M4_no_cache', 'tuned', 8, S=2, B=5, n_modes=4, transmission_cache=False))
    rows.append(_row('tuned_B9_M5_three_distances', 'tuned', 8, S=2, B=9, n_modes=5, free_prop=list(DISTS), pp='probes'))
    # tuned, shift adjoint: atomics below and at the boundary; slots with a last chunk of 1; one chunk (second level of one); one
    # full chunk; two chunks; B = 300
    for B, M in ((127, 2), (128, 2), (129, 2), (5, 64), (32, 9), (33, 8), (300, 1)):
        rows.append(_row('tuned_shift_B%d_M%d' % (B, M), 'tuned', 8, S=2, B=B, n_modes=M, pp='shifts'))
    # the any-size kernel (33 x 31 is no tuned size)
    for B in (1, 257):
        rows.append(_row('generic_B%d' % B, 'generic', (33, 31), S=2, B=B))
    for M in (4, 33, 64):
        rows.append(_row('generic_M%d' % M, 'generic', (33, 31), S=2, B=5, n_modes=M))
    rows.append(_row('generic_B9_M5_three_distances', 'generic', (33, 31), S=2, B=9, n_modes=5, free_prop=list(DISTS)))
    # streamed
    for B in (256, 257):
        rows.append(_row('streamed_B%d' % B, 'streamed', (24, 24), S=2, B=B))
    for M in (4, 64):
        rows.append(_row('streamed_24x20_M%d' % M, 'streamed', (24, 20), S=2, B=3, n_modes=M))
    rows.append(_row('streamed_shift_4x1024_M2', 'streamed', (4, 1024), S=2, B=3, n_modes=2, pp='shifts'))      # per = 256
    rows.append(_row('streamed_shift_4x1032_M2', 'streamed', (4, 1032), S=2, B=3, n_modes=2, pp='shifts'))      # per = 258
    for B in (257, 300):
        rows.append(_row('streamed_shift_B%d' % B, 'streamed', (24, 24), S=2, B=B, pp='shifts'))
    # the index patterns of every shift case with B >= 257
    for base in ('tuned_shift_B300_M1', 'streamed_shift_B257', 'streamed_shift_B300'):
        spec = dict(rows)[base]
        for pat in INDEX_PATTERNS:
            rows.append(_row('%s_%s' % (base, pat), spec['family'], spec['P'], index=pat, **spec['kw']))
    # exit-wave shifts and sparse multislice have references of their own (tests/prj_offset_ref.py, tests/sparse_ref.py)
    rows.append(_row('exit_shift_B257', 'exit', (24, 20), S=2, B=257, M=1))
    rows.append(_row('sparse_B257', 'sparse', (24, 24), S=3, B=257, M=1))
    rows.append(_row('sparse_B3_M5', 'sparse', (24, 24), S=3, B=3, M=5, seed=2))      # (seed 0: the fp32 yardstick of dL/dz is 4e-7, below 1e-6)
    return dict(rows)


CASES = _cases()
ORACLE_FAMILIES = ('tuned', 'generic', 'streamed')
ORACLE_CASES = [n for n, c in CASES.items() if c['family'] in ORACLE_FAMILIES]
LARGE = 257             # 'large-count' cases: B >= LARGE


def modes_of(spec):
    return spec['kw'].get('n_modes', spec['kw'].get('M', 1))


def case_kw(name):
    """The oracle_case arguments of a row."""
    spec = CASES[name]
    kw = dict(spec['kw'])
    kw.setdefault('margin', spread_margin(spec['P'], kw['B']))
    if spec['index'] is not None:
        kw['index_fn'] = INDEX_PATTERNS[spec['index']]
    return kw


@functools.lru_cache(maxsize=None)
def build(name):
    """The inputs and oracle results of a row, computed once per process and left unchanged by everyone."""
    spec = CASES[name]
    if spec['family'] == 'exit':
        return exit_case(spec['P'], **spec['kw'])
    if spec['family'] == 'sparse':
        return sparse_case(spec['P'], **spec['kw'])
    return MM.oracle_case(spec['P'], **case_kw(name))


def bars_of(family):
    return MM.TUNED if family == 'tuned' else MM.GENERIC


def _own_inputs(P, S, B, M, seed):
    """Inputs drawn like make_case of test_gpu_prj_offset.py / test_gpu_sparse_multislice.py, with the positions spread."""
    Py, Px = P
    r = np.random.default_rng([Py, Px, S, B, M, seed])
    my, mx = spread_margin(P, B)
    Y, X = Py + my, Px + mx
    mk = lambda c: np.stack([2e-3 * c * r.uniform(size=(Y, X, S)), 2e-4 * c * r.uniform(size=(Y, X, S))], -1)
    obj, truth = mk(1).astype(np.float32), mk(10).astype(np.float32)
    pos = MM.edge_positions(r, B, Y, X, Py, Px)
    probes = ((0.5 + r.uniform(0, 1, (M, Py, Px))) * np.exp(1j * r.uniform(-np.pi, np.pi, (M, Py, Px)))).astype(np.complex64)
    tiles, _ = O.extract_tiles(truth.astype(np.float64), pos, (Py, Px), 'delta_beta')
    return r, obj, pos, probes, tiles


EXIT_FREE_PROP_CM = 2e-4            # FREE_PROP_CM of test_gpu_prj_offset.py


def exit_case(P, S, B, M, seed=0):
    """A case for run_shifted / yardstick / check_3x of test_gpu_prj_offset.py: 16 offset entries under the 'mixed' index."""
    r, obj, pos, probes, tiles = _own_inputs(P, S, B, M, seed)
    n, index = _idx_mixed(B)
    shifts = r.uniform(-2, 2, (n, 2)).astype(np.float32)
    phys = O.Physics(P, MM.ENERGY_EV, MM.PSIZE_CM, free_prop_cm=EXIT_FREE_PROP_CM)
    meas = PR.predict(tiles, probes.astype(np.complex128), phys, shifts.astype(np.float64) + r.uniform(-0.3, 0.3, (n, 2)), index)
    return dict(obj=obj, pos=pos, probes=probes, shifts=shifts, index=index.astype(np.int32), meas=meas.astype(np.float32),
                unknown_type='delta_beta', free_prop=EXIT_FREE_PROP_CM, sign_convention=1)


def sparse_case(P, S, B, M, seed=0):
    """A case for run_sparse / yardstick / check_3x of test_gpu_sparse_multislice.py."""
    r, obj, pos, probes, tiles = _own_inputs(P, S, B, M, seed)
    z = np.concatenate([[0.], np.cumsum(r.uniform(3e-4, 3e-3, S - 1))]).astype(np.float32)
    phys = O.Physics(P, MM.ENERGY_EV, MM.PSIZE_CM, free_prop_cm='inf')
    meas = SR.predict(tiles, probes.astype(np.complex128), phys, (z * np.float32(1.03)).astype(np.float64))
    return dict(obj=obj, pos=pos, probes=probes, z=z, meas=meas.astype(np.float32), unknown_type='delta_beta', free_prop='inf',
                sign_convention=1)


def loss_sums_of(pred, meas):
    """Per-position sums of the LSQ loss terms of a prediction [B, Py, Px] (what the engine's loss_sums holds)."""
    return ((np.asarray(pred, np.float64) - np.asarray(meas, np.float64)) ** 2).sum(axis=(1, 2))


# ---------------------------------------------------------------------------------------------------------------- classes
def classes_of(name):
    """The sides of the count thresholds a row is on, computed from B, M, the column geometry and the index."""
    spec = CASES[name]
    fam, kw = spec['family'], spec['kw']
    B, M = kw['B'], modes_of(spec)
    P = spec['P'] if not np.isscalar(spec['P']) else (spec['P'], spec['P'])
    out = {'modes_1' if M == 1 else 'modes_max' if M == MAX_MODES else 'modes_4_to_63' if M > 3 else 'modes_2_3'}
    if fam == 'tuned':
        q, r = B >> 3, B & 7
        out |= {'xcd_q0' if q == 0 else 'xcd_q_pos', 'xcd_r0' if r == 0 else 'xcd_r7' if r == 7 else 'xcd_r_mid'}
        if B > 256:
            out.add('tuned_second_round_of_workgroups')
        if kw.get('pp') == 'shifts':
            pairs = B * M
            out.add('pairs_below_256' if pairs < SLOT_PAIRS else 'pairs_at_256' if pairs == SLOT_PAIRS else 'pairs_above_256')
            if uses_slots(B, M):
                ch = pgr_chunks(B)
                out.add('one_chunk' if len(ch) == 1 else 'several_chunks')
                out.add('ragged_last_chunk' if ch[-1][1] - ch[-1][0] < PGR_CHUNK else 'full_last_chunk')
    if fam == 'generic':
        out.add('generic_grid_1' if B == 1 else 'generic_grid_gt_256' if B > 256 else 'generic_grid_small')
    if isinstance(kw.get('free_prop'), list):
        out.add('distances_%s' % ('per_position_probes' if kw.get('pp') == 'probes' else 'shared_probes'))
    if fam in ('streamed', 'exit', 'sparse'):
        ncg = SM.geometry(*P)['n_col_groups']
        wg = loss_reduce_workgroups(B)
        out.add('loss_reduce_one_workgroup_full' if (wg == 1 and B == RED_NT) else 'loss_reduce_one_workgroup' if wg == 1
                else 'loss_reduce_two_workgroups')
        if SM.geometry(*P)['cw_last'] < SM.geometry(*P)['cw']:
            out.add('ragged_last_column_group')
        if fam == 'exit' or kw.get('pp') == 'shifts':
            per = M * ncg
            out.add('per_below_256' if per < RED_NT else 'per_at_256' if per == RED_NT else 'per_above_256')
            last = B - 1                # the last workgroup searches index[0 .. B - 1)
            out.add('search_below_256' if last < RED_NT else 'search_at_256' if last == RED_NT else 'search_two_trips')
    if fam == 'exit' or kw.get('pp') == 'shifts':
        pat = spec['index'] if fam != 'exit' else 'mixed'
        out.add('index_%s' % (pat or 'default'))
        if pat is not None and fam != 'tuned':
            n, idx = INDEX_PATTERNS[pat](B)
            idx = np.arange(B) if idx is None else idx
            first = {int(e): int(np.flatnonzero(idx == e)[0]) for e in np.unique(idx)}
            if any(f >= RED_NT and (idx == e).sum() > 1 and np.flatnonzero(idx == e)[1] > RED_NT for e, f in first.items()):
                out.add('first_user_beyond_256_found_by_a_later_one')
            if n - len(first) >= 2:
                out.add('two_unused_entries')
    return out


# both sides of every threshold: each of these classes needs a row
REQUIRED_CLASSES = (
    'xcd_q0', 'xcd_q_pos', 'xcd_r0', 'xcd_r7', 'xcd_r_mid', 'tuned_second_round_of_workgroups',
    'modes_1', 'modes_4_to_63', 'modes_max',
    'pairs_below_256', 'pairs_at_256', 'pairs_above_256', 'one_chunk', 'several_chunks', 'ragged_last_chunk', 'full_last_chunk',
    'generic_grid_1', 'generic_grid_gt_256', 'generic_grid_small', 'distances_per_position_probes', 'distances_shared_probes',
    'loss_reduce_one_workgroup', 'loss_reduce_one_workgroup_full', 'loss_reduce_two_workgroups', 'ragged_last_column_group',
    'per_below_256', 'per_at_256', 'per_above_256', 'search_below_256', 'search_at_256', 'search_two_trips',
    'first_user_beyond_256_found_by_a_later_one', 'two_unused_entries',
) + tuple('index_' + p for p in INDEX_PATTERNS)
# every __global__ kernel of the multislice files whose grid or loops take B, M or an index -> the rows that run it
KERNEL_ROWS = {
    'ms_fwd_adj_kernel': ('adm_multislice.hip', 'test_tuned', ['tuned_B257', DENSE, 'tuned_M64_far', 'tuned_M64_fresnel']),
    'probe_shift_kernel': ('adm_multislice.hip', 'test_tuned', ['tuned_shift_B300_M1', 'tuned_shift_B5_M64']),
    'probe_shift_adj_kernel': ('adm_multislice.hip', 'test_tuned', ['tuned_shift_B128_M2', 'tuned_shift_B129_M2', 'tuned_shift_B5_M64']),
    'probe_grad_reduce_kernel': ('adm_api.hip', 'test_tuned', ['tuned_shift_B5_M64', 'tuned_shift_B33_M8']),
    'probe_grad_reduce_chunks_kernel': ('adm_api.hip', 'test_tuned', ['tuned_shift_B129_M2', 'tuned_shift_B32_M9']),
    'ms_generic_kernel': ('adm_ms_generic.hip', 'test_generic', ['generic_B257', 'generic_M64', 'generic_B9_M5_three_distances']),
    'st_row_kernel': ('adm_ms_streamed.hip', 'test_streamed', ['streamed_B257', 'streamed_24x20_M64']),
    'st_col_conv_kernel': ('adm_ms_streamed.hip', 'test_streamed', ['streamed_B257', 'streamed_24x20_M64']),
    'st_det_kernel': ('adm_ms_streamed.hip', 'test_streamed', ['streamed_B257', 'streamed_24x20_M64']),
    'st_loss_reduce_kernel': ('adm_ms_streamed.hip', 'test_streamed', ['streamed_B256', 'streamed_B257']),
    'st_shift_reduce_kernel': ('adm_ms_streamed.hip', 'test_streamed', ['streamed_shift_4x1032_M2', 'streamed_shift_B300_mixed']),
    'st_col_conv_sparse_kernel': ('adm_ms_streamed.hip', 'test_sparse', ['sparse_B257', 'sparse_B3_M5']),
    'st_dd_reduce_kernel': ('adm_ms_streamed.hip', 'test_sparse', ['sparse_B257', 'sparse_B3_M5']),
    'es_col_conv_kernel': ('adm_ms_exitshift.hip', 'test_exit_shift', ['exit_shift_B257']),
    'ps_col_kernel': ('adm_ms_probeshift.hip', 'test_streamed', ['streamed_shift_B257', 'streamed_shift_4x1032_M2']),
}
# kernels of those files that take no count: one workgroup per row group of ONE probe set, a table per slice, one anchor
NO_COUNT = {'ps_colfft_kernel': 'the spectrum of the M shared probe modes: its grid is M * column groups, run with M = 2 by '
                                'streamed_shift_4x1032_M2 but never beyond the modes the shape matrix runs',
            'st_fresnel_table_kernel': 'one thread per element of the S - 1 (a fan-out: D) transfer functions', 'st_sparse_anchor_kernel': 'one workgroup'}


# ---------------------------------------------------------------------------------------------------------------- the engine
UNUSED_SEED = np.float32(3.25)
ROUND_CAPS = (43,)      # 300 positions in rounds of at most 43: six of 43 and a last one of 42


def seeded_gs(case):
    """The start of grad_shifts: 0 for the entries some position uses, a seed for the others (they must come back bit for bit)."""
    n, idx = index_of(case)
    g = np.full((n, 2), UNUSED_SEED, np.float32)
    g[np.unique(idx)] = 0
    return g


def run(A, ctx, case, family, **engine_kw):
    """rotate -> multislice -> rotate_adjoint on an engine of the row's family; a copy of the case with pred, loss, loss_sum,
    grad, gprobe (and its raw words), gshift / gs_raw / gs_seed, n_rounds added."""
    out, k = dict(case), case['kw']
    obj, pos, probes, pprobes, target, bs, shifts, idx = [case[n] for n in ('obj', 'pos', 'probes', 'pprobes', 'target', 'beamstop',
                                                                            'shifts', 'idx')]
    (Py, Px), S, B, M, pp = k['shape'], k['S'], k['B'], k['n_modes'], k['pp']
    Y, X = obj.shape[:2]
    streamed = family == 'streamed'
    eng = A.MultisliceEngine(ctx, (Y, X, S), (Py, Px), pos, MM.ENERGY_EV, MM.PSIZE_CM, free_prop_cm=k['free_prop'], binning=k['binning'],
                             fresnel_approx=k['fresnel_approx'], sign_convention=k['sign_convention'], normalize_fft=k['normalize_fft'],
                             n_probe_modes=M, max_batch=B, loss_function_type=k['loss'], poisson_multiplier=k['poisson_multiplier'],
                             unknown_type=k['unknown_type'], beamstop=bs, generic=k['generic'], transmission_cache=k['transmission_cache'],
                             streamed=streamed, probe_shift=streamed and pp == 'shifts', **engine_kw)
    assert eng.streamed is streamed
    d_grad, d_gp = ctx.zeros(obj.shape), ctx.zeros((M, Py, Px, 2))
    eng.set_batch(pos, target)
    eng.rotate(ctx.array(obj, np.float32), None)
    if pp == 'shifts':
        seed = seeded_gs(case)
        d_gs = ctx.array(seed)
        d_idx = ctx.array(np.ascontiguousarray(idx, np.int32)) if idx is not None else None
        eng.multislice(ctx.array(MM.c2(probes)), grad_probe=d_gp, want_pred=True, shifts=ctx.array(shifts, np.float32), shift_index=d_idx,
                       grad_shifts=d_gs)
        out['gs_raw'], out['gs_seed'] = d_gs.get(), seed
        out['gshift'] = out['gs_raw'].astype(np.float64) - seed            # (exact: one of the two is zero everywhere)
        if not streamed and not uses_slots(B, M):
            out['gprobe_b'] = MM.cplx(eng._gprobes_b.get()[:B])             # (the slot path sums in this buffer: nothing to read)
    elif pp == 'probes':
        eng.multislice(None, want_pred=True, probes_b=ctx.array(MM.c2(pprobes)))
    else:
        eng.multislice(ctx.array(MM.c2(probes)), grad_probe=d_gp, want_pred=True)
    eng.rotate_adjoint(d_grad, None)
    out['pred'] = eng.pred()
    out['loss'] = eng.loss()
    out['loss_sum'] = eng.loss_sums(B)
    out['grad'] = d_grad.get()
    out['gprobe_raw'] = d_gp.get()
    out['gprobe'] = MM.cplx(out['gprobe_raw']) if pp != 'probes' else None
    out['n_rounds'] = len(eng.rounds(B))
    out['cover'] = eng._check_cover(eng._pos_host)
    out['ws_bytes'] = {n: eng.plan.workspace_bytes(n) for n in ROUND_CAPS}
    eng.plan.close()
    return out


# ---------------------------------------------------------------------------------------------------------------- each count
def _items(x, x64, x32, floor, what, cap=None, absolute=False):
    """The band rule with one band per item of the leading axis: an item's distance from the fp64 oracle is at most 3 x the fp32
    oracle's on the same item + ``floor`` (relative to the item's own norm); items below 1e-3 of the largest item's norm carry no
    signal and are not judged.  Returns (judged items, worst error, the fp32 oracle's there, items without signal)."""
    x, x64, x32 = [np.asarray(a).reshape(len(x64), -1) for a in (x, x64, x32)]
    n = np.sqrt((np.abs(x64) ** 2).sum(1))
    judged = n >= 1e-3 * n.max()
    nn = np.where(judged, n, 1.)
    e = np.sqrt((np.abs(x - x64) ** 2).sum(1)) / nn
    e32 = np.sqrt((np.abs(x32 - x64) ** 2).sum(1)) / nn
    margin = np.where(judged, e - (3 * e32 + floor), -np.inf)
    k = int(np.argmax(margin))
    assert margin[k] <= 0, (what, 'item %d of %d' % (k, len(n)), float(e[k]), float(e32[k]), floor)
    if cap is not None:
        assert e[judged].max() < cap, (what, float(e[judged].max()), cap)
    return int(judged.sum()), float(e[k]), float(e32[k]), int((~judged).sum())


def used_entries(case):
    n, idx = index_of(case)
    used = np.zeros(n, bool)
    used[idx] = True
    return used


def check_counts(res, bars, what='', quiet=False):
    """Every position's prediction and loss sum, every mode's probe gradient, every USED entry's shift gradient on its own."""
    out = {}
    out['pred'] = _items(res['pred'], res['pred_o'], res['pred_32'], bars['pred'], what + ' pred of a position')
    n_det = res['n_det']
    out['loss_sum'] = _items(res['loss_sum'], res['loss_b_o'] * n_det, res['loss_b_32'] * n_det, bars['loss'], what + ' loss sum of a position')
    if res.get('gprobe') is not None:
        out['gprobe'] = _items(res['gprobe'], res['gprobe_o'], res['gprobe_32'], bars['grad_abs'], what + ' probe gradient of a mode',
                               cap=bars['grad'])
    if res.get('gshift') is not None and res.get('shifts') is not None:
        u = used_entries(res)
        out['gshift'] = _items(np.asarray(res['gshift'])[u], res['gshift_o'][u], res['gshift_32'][u], bars['shift'],
                               what + ' shift gradient of an entry')
    if not quiet:
        print(what, 'each count (items judged, worst, fp32 oracle there, without signal):',
              {k: '%d %.2e (%.2e) %d' % v for k, v in out.items()})
    return out


def as_engine(case, family, sfx='_32'):
    """The oracle's own run dressed as an engine result (the coverage test judges the fp32 oracle, and perturbed fp64 results,
    with the GPU module's checks)."""
    out = dict(case)
    n_det = case['n_det']
    for k in ('pred', 'loss', 'grad', 'gprobe', 'gprobe_b', 'gshift'):
        out[k] = case[k + sfx]
    out['loss_sum'] = case['loss_b' + sfx] * n_det
    pp = case['kw']['pp']
    if pp != 'shifts':
        del out['gprobe_b'], out['gshift']
    elif family != 'tuned' or uses_slots(case['kw']['B'], case['kw']['n_modes']):
        del out['gprobe_b']
    if pp == 'probes':
        out['gprobe'] = None
    return out


# ---------------------------------------------------------------------------------------------------------------- perturbations
def position_terms(case, b, entry=None, dist=None):
    """What position b adds to the fp64 oracle's results (loss, pred, tile gradient, probe gradient, shift gradient), evaluated as
    oracle_case does -- with another shift entry or another detector distance when asked."""
    k = case['kw']
    Py, Px = k['shape']
    dists = list(k['free_prop']) if isinstance(k['free_prop'], (list, tuple)) else [k['free_prop']]
    d = dists[(b if dist is None else dist) % len(dists)]
    ph = O.Physics((Py, Px), MM.ENERGY_EV, MM.PSIZE_CM, free_prop_cm=d, binning=k['binning'], fresnel_approx=k['fresnel_approx'],
                   sign_convention=k['sign_convention'], normalize_fft=k['normalize_fft'], unknown_type=k['unknown_type'])
    tiles, _ = O.extract_tiles(case['obj'].astype('float64'), case['pos'][b:b + 1], (Py, Px), k['unknown_type'])
    lkw = dict(loss_function_type=k['loss'], raw_data_type='magnitude', poisson_multiplier=k['poisson_multiplier'], beamstop=case['beamstop'])
    mb = case['meas'][b:b + 1]
    if k['pp'] == 'shifts':
        e = index_of(case)[1][b] if entry is None else entry
        l, pr, gt, g, gsh = O.forward_adjoint_tiles(tiles, case['probes'], mb, ph, 'float64', shifts=case['shifts'][e][None], **lkw)
        return l, pr, gt, g, (e, gsh[0])
    l, pr, gt, g = O.forward_adjoint_tiles(tiles, case['pprobes'][b], mb, ph, 'float64', **lkw)
    return l, pr, gt, g, None


def perturbed(case, family, b, kind):
    """The fp64 oracle's results with position b wrong in one way, dressed as an engine result: 'drop' (the position is never run:
    its outputs stay zero and its terms are missing), 'entry' (it takes position b + 1's shift entry), 'distance' (it takes
    position b + 1's detector distance)."""
    B = case['kw']['B']
    out = as_engine(case, family, '_o')
    for key in ('pred', 'grad', 'gprobe', 'gshift', 'loss_sum'):
        if out.get(key) is not None:
            out[key] = np.array(out[key])
    right = position_terms(case, b)
    if kind == 'drop':
        wrong = (0., np.zeros_like(right[1]), np.zeros_like(right[2]), np.zeros_like(right[3]), None if right[4] is None else (right[4][0], 0.))
    elif kind == 'entry':
        wrong = position_terms(case, b, entry=index_of(case)[1][(b + 1) % B])
    elif kind == 'distance':
        wrong = position_terms(case, b, dist=b + 1)
    else:
        raise KeyError(kind)
    out['loss'] = out['loss'] + (wrong[0] - right[0]) / B
    out['loss_sum'][b] = wrong[0] * case['n_det']
    out['pred'][b] = wrong[1][0]
    out['grad'] += O.scatter_tiles_adj(wrong[2] - right[2], case['pos'][b:b + 1], case['obj'].shape) / B
    if out.get('gprobe') is not None:
        out['gprobe'] += (wrong[3] - right[3]) / B
    if right[4] is not None:
        out['gshift'][right[4][0]] -= right[4][1] / B
        out['gshift'][wrong[4][0]] += np.asarray(wrong[4][1]) / B
    out.pop('gprobe_b', None)
    return out


# ---------------------------------------------------------------------------------------------------------------- the sources
def read(name):
    with open(os.path.join(CSRC, name)) as f:
        return f.read()


def function_body(src, signature):
    """Text of the brace-balanced body of the first function whose head matches ``signature``."""
    m = re.search(signature, src)
    assert m, signature
    i = src.index('{', m.end())
    depth = 0
    for j in range(i, len(src)):
        depth += {'{': 1, '}': -1}.get(src[j], 0)
        if depth == 0:
            return src[i:j + 1]
    raise AssertionError('unbalanced body: ' + signature)


def parsed_xcd_position(src=None):
    """xcd_position of adm_multislice.hip as a Python function built from its source text (its integer expressions -- &, >>, *, +,
    min -- read the same in both languages), and that text."""
    body = function_body(read('adm_multislice.hip') if src is None else src, r'int\s+xcd_position\s*\(\s*int\s+wg\s*,\s*int\s+B\s*\)')
    stmts = [s.strip() for s in body.strip('{} \n').split(';') if s.strip()]
    assert all(re.fullmatch(r'(const int [\w =&>*+(),\s]+|return [\w =&>*+(),\s]+)', s) for s in stmts), stmts
    lines = []
    for s in stmts:
        if s.startswith('return '):
            lines.append(s)
        else:
            # 'const int a = X, b = Y' -> 'a = X; b = Y' (the commas inside min(...) stay)
            parts = re.split(r',\s*(?=\w+\s*=)', s[len('const int '):])
            lines.extend(p.strip() for p in parts)
    code = 'def f(wg, B):\n' + ''.join('    %s\n' % ln for ln in lines)
    env = {'min': np.minimum}           # (workgroup numbers may come as an array)
    exec(code, env)
    return env['f'], ' '.join(body.split())
