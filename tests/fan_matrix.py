"""The COUNT axis of the multi-distance detector fan-out (test infrastructure only): with ``detector_fanout`` the row launches of the
detector step, st_det_kernel and st_loss_reduce_kernel run over E = B * D detector entries instead of B positions, the workspace,
targets, predictions and loss sums scale with E, and md_fanout_kernel / md_fanin_kernel loop over D (adm_ms_multidist.hip).
tests/test_gpu_multidist3d.py holds B = 3, M <= 2, D <= 4; this matrix sweeps B, D and M over every threshold of that code.

* mirrors of what the sources hold: the fan-out limit, the entries per workgroup of st_loss_reduce_kernel, the chunk of the probe
  gradient reduction (count_matrix's), the entry index b * D + d and the detector-field index (b * D + d) * M + m.  The coverage
  test (tests/test_fanout_domain_coverage.py) parses the sources and fails when one of them moves away from its mirror.
* ``make_case``: make_case of test_gpu_multidist3d.py with explicit distances, a sign convention and count_matrix's ``margin``
  (no pixel covered by more than 64 tiles); ``build`` adds the restatement's fp64 and fp32 runs (tests/multidist3d_ref.py through
  ref_fanout) and every entry's loss sum.
* ``CASES``: one row per case, the field 24 x 20 (a ragged last column group) and S = 2 unless the row says otherwise;
  ``classes_of`` computes from B, M, D, the distances and the column geometry which side of every threshold a row is on.
* ``check_entries``: ms_matrix.check with GENERIC, then every entry's prediction and loss sum and every mode's probe gradient on
  its own under the band rule of the other matrices (count_matrix._items: 3 x the fp32 restatement on the same item + the
  whole-array bar); every item must have been judged.
"""
import functools
import time

import numpy as np

from tests import count_matrix as CM
from tests import ms_matrix as MM
from tests import st_matrix as SM
from tests import multidist3d_ref as MR
from tests import test_gpu_multidist3d as MD

O = MD.O
BARS = MM.GENERIC

# what the sources hold (compared with them by the coverage test)
MAX_FAN = 64                    # adm_plan_set_detector_fanout (adm_api.hip): n <= 64
RED_NT = CM.RED_NT              # st_loss_reduce_kernel: entries per workgroup
PGR_CHUNK = CM.PGR_CHUNK        # adm_api.hip: positions per chunk of probe_grad_reduce_large
MAX_MODES = CM.MAX_MODES
FIELD = (24, 20)


def entry_index(b, d, D):
    """The detector entry (target, prediction, loss sum) of position b at distance d: position-major."""
    return b * D + d


def det_field_index(b, d, m, D, M):
    """The detector-plane field of (position, distance, mode) in the fan-out's buffers (md_fanout_kernel, md_fanin_kernel)."""
    return (b * D + d) * M + m


def loss_reduce_workgroups(E):
    return CM.loss_reduce_workgroups(E)


def default_dists(D):
    """The mild distances of test_gpu_multidist3d.py up to four planes, beyond that D distinct ones from 1 um to 50 um."""
    return list(MD.DISTS_CM[:D]) if D <= len(MD.DISTS_CM) else [float(d) for d in np.geomspace(1e-4, 5e-3, D)]


# ---------------------------------------------------------------------------------------------------------------- the case builder
def make_case(P=FIELD, S=2, B=3, M=1, D=2, dists=None, sign_convention=1, margin=None, seed=0):
    """Built like make_case of test_gpu_multidist3d.py (positions over the object's edges, a truth with ten times the guess's contrast
    makes the data), with explicit ``dists`` (cm), ``sign_convention`` and ``margin`` (default count_matrix.spread_margin)."""
    Py, Px = (P, P) if np.isscalar(P) else tuple(P)
    dists = default_dists(D) if dists is None else [float(d) for d in dists]
    assert len(dists) == D, (D, dists)
    r = np.random.default_rng([Py, Px, S, B, M, D, seed])
    my, mx = CM.spread_margin((Py, Px), B) if margin is None else margin
    Y, X = Py + my, Px + mx
    mk = lambda c: np.stack([2e-3 * c * r.uniform(size=(Y, X, S)), 2e-4 * c * r.uniform(size=(Y, X, S))], -1)
    obj, truth = mk(1).astype(np.float32), mk(10).astype(np.float32)
    pos = MM.edge_positions(r, B, Y, X, Py, Px)
    probes = ((0.5 + r.uniform(0, 1, (M, Py, Px))) * np.exp(1j * r.uniform(-np.pi, np.pi, (M, Py, Px)))).astype(np.complex64)
    phys = O.Physics((Py, Px), MD.ENERGY_EV, MD.PSIZE_CM, free_prop_cm=dists[0], sign_convention=sign_convention)
    tiles, _ = O.extract_tiles(truth.astype(np.float64), pos, (Py, Px))
    meas = MR.predict(tiles, probes.astype(np.complex128), phys, dists).astype(np.float32)
    return dict(obj=obj, pos=pos, probes=probes, dists=dists, meas=meas, target=meas, sign_convention=sign_convention, loss='lsq',
                poisson_multiplier=1., beamstop=None, raw_data_type='magnitude')


def with_refs(case):
    """A copy of ``case`` with what ref_fanout returns in fp64 (``*_o``) and fp32 (``*_32``) and every entry's loss sum
    (``loss_e_*``: what the engine's loss_sums holds), in the layout ms_matrix.check reads."""
    r64, r32 = MD.ref_fanout(case, 'float64'), MD.ref_fanout(case, 'float32')
    out = MD.as_res(case, r64, r32, case)
    out['loss_e_o'], out['loss_e_32'] = CM.loss_sums_of(r64['pred'], case['meas']), CM.loss_sums_of(r32['pred'], case['meas'])
    return out


# ---------------------------------------------------------------------------------------------------------------- cases
def _row(name, B, D, M, P=FIELD, **kw):
    return name, dict(P=P, B=B, D=D, M=M, kw=kw)


# the distance axis, at (3, D, 2) under both sign conventions
DISTANCE_SETS = {
    'descending': [5e-4, 3.5e-4, 2e-4, 1e-4],
    'repeated': [2e-4, 2e-4, 1e-4],
    'near_field': [1e-6, 1e-5, 1e-4],
    'aliased': [1e-4, 2e-2, 5e-2],
}
TALL = (1025, 12)               # the smallest cw = 4 column geometry


def _cases():
    rows = []
    counts = [
        (64, 4, 1), (65, 4, 1),                         # E = 256, 260 by the batch
        (4, 64, 1), (5, 64, 1),                         # E = 256, 320 by the distances
        (16, 16, 1), (17, 16, 1),                       # E = 256, 272 by both
        (129, 2, 1),                                    # E = 258 with D small
        (257, 2, 1),                                    # E = 514: a third loss-reduce workgroup, B itself over 256
        (3, 63, 1), (3, 64, 1), (3, 33, 1), (3, 3, 1),  # D below, at and at the odd middle of the limit
        (3, 2, 64), (3, 33, 4), (1, 64, 64),            # many modes with a fan-out
        (32, 3, 2), (33, 3, 2), (65, 2, 2),             # probe-gradient chunks with a fan-out
    ]
    for B, D, M in counts:
        rows.append(_row('B%d_D%d_M%d' % (B, D, M), B, D, M))
    rows.append(_row('tall_B2_D33_M1', 2, 33, 1, P=TALL))
    for what, dists in DISTANCE_SETS.items():
        for sg in (1, -1):
            rows.append(_row('%s_%s' % (what, 'p1' if sg == 1 else 'm1'), 3, len(dists), 2, dists=dists, sign_convention=sg))
    return dict(rows)


CASES = _cases()
TWICE = ('B5_D64_M1', 'B257_D2_M1')
BUILD_SECONDS = {}              # CPU time of a row's inputs and its fp64 + fp32 yardsticks
ROUNDS = {          # name -> (B, D, M, positions the workspace budget holds, the split of the batch)
    'rounds_B7_D3_M2': (7, 3, 2, 3, [3, 2, 2]),
    'rounds_B5_D64_M1': (5, 64, 1, 2, [2, 2, 1]),
}


def case_kw(name):
    spec = CASES[name]
    return dict(P=spec['P'], B=spec['B'], D=spec['D'], M=spec['M'], **spec['kw'])


@functools.lru_cache(maxsize=None)
def build(name):
    """The inputs of a row and the restatement's results on them, computed once per process and left unchanged by everyone."""
    t0 = time.perf_counter()
    out = with_refs(make_case(**case_kw(name)))
    BUILD_SECONDS[name] = time.perf_counter() - t0
    return out


@functools.lru_cache(maxsize=None)
def build_counts(B, D, M, seed=0):
    """The same for a (B, D, M) that is no row (rounds, the engine re-used over batch sizes, the loss read-backs)."""
    return with_refs(make_case(B=B, D=D, M=M, seed=seed))


# ---------------------------------------------------------------------------------------------------------------- classes
def phase_step_at_nyquist(dist_cm, P):
    """The largest phase step between neighbouring frequencies of the Fresnel kernel exp(-i pi lambda z (u^2 + v^2)) on a P field,
    in units of pi: lambda z / (N psize^2) at the Nyquist frequency of the shorter side.  Above 1 the kernel is aliased."""
    lam_nm, ps_nm = 1240. / MD.ENERGY_EV, MD.PSIZE_CM * 1e7
    return lam_nm * dist_cm * 1e7 / (min(P) * ps_nm ** 2)


def is_near_field(dist_cm):
    """lambda z < psize^2: the kernel's phase stays below pi / 2 over the whole band."""
    return (1240. / MD.ENERGY_EV) * dist_cm * 1e7 < (MD.PSIZE_CM * 1e7) ** 2


def classes_of(name):
    """The sides of the thresholds a row is on, computed from B, D, M, the distances and the column geometry."""
    spec = CASES[name]
    B, D, M, P = spec['B'], spec['D'], spec['M'], spec['P']
    E = B * D
    dists = spec['kw'].get('dists') or default_dists(D)
    out = {'modes_1' if M == 1 else 'modes_max' if M == MAX_MODES else 'modes_4_to_63' if M > 3 else 'modes_2_3'}
    out.add('entries_below_256' if E < RED_NT else 'entries_at_256' if E == RED_NT else 'entries_above_256')
    if E >= RED_NT:
        side = 'at' if E == RED_NT else 'above'
        out.add('entries_%s_256_by_%s' % (side, 'batch' if D <= 4 else 'distances' if D == MAX_FAN else 'both'))
    wg = loss_reduce_workgroups(E)
    out.add('loss_reduce_one_workgroup' if wg == 1 else 'loss_reduce_two_workgroups' if wg == 2 else 'loss_reduce_three_workgroups')
    out.add('batch_up_to_256' if B <= 256 else 'batch_above_256')
    out.add('fan_max' if D == MAX_FAN else 'fan_max_less_1' if D == MAX_FAN - 1 else 'fan_odd_middle' if D == MAX_FAN // 2 + 1
            else 'fan_2_to_4' if D <= 4 else 'fan_other')
    out.add('batch_below_32' if B < PGR_CHUNK else 'batch_at_32' if B == PGR_CHUNK else 'batch_above_32')
    if B > PGR_CHUNK:
        ch = CM.pgr_chunks(B)
        out.add('ragged_last_chunk' if ch[-1][1] - ch[-1][0] < PGR_CHUNK else 'full_last_chunk')
        out.add('two_chunks' if len(ch) == 2 else 'three_or_more_chunks')
    if M > 1 and D > 1:
        out.add('parked_fields_per_entry')           # w.det = E * M fields, w.fan_field = E * M fields
    geo = SM.geometry(*P)
    out.add('cw%d' % geo['cw'])
    if geo['cw_last'] < geo['cw']:
        out.add('ragged_last_column_group')
    if D > 4 and geo['cw'] == 4:
        out.add('tall_columns_large_fan')
    d = np.asarray(dists)
    if len(set(dists)) < D:
        out.add('distances_repeated')
    elif np.all(np.diff(d) > 0):
        out.add('distances_ascending')
    elif np.all(np.diff(d) < 0):
        out.add('distances_descending')
    if any(is_near_field(z) for z in dists):
        out.add('distances_near_field')
    if any(phase_step_at_nyquist(z, P) > 1 for z in dists):
        out.add('distances_aliased')
    out.add('sign_%s' % ('p1' if spec['kw'].get('sign_convention', 1) == 1 else 'm1'))
    return out


# both sides of every threshold: each of these classes needs a row
REQUIRED_CLASSES = (
    'entries_below_256', 'entries_at_256', 'entries_above_256',
    'entries_at_256_by_batch', 'entries_above_256_by_batch', 'entries_at_256_by_distances', 'entries_above_256_by_distances',
    'entries_at_256_by_both', 'entries_above_256_by_both',
    'loss_reduce_one_workgroup', 'loss_reduce_two_workgroups', 'loss_reduce_three_workgroups', 'batch_up_to_256', 'batch_above_256',
    'fan_2_to_4', 'fan_odd_middle', 'fan_max_less_1', 'fan_max', 'modes_1', 'modes_2_3', 'modes_4_to_63', 'modes_max',
    'batch_below_32', 'batch_at_32', 'batch_above_32', 'ragged_last_chunk', 'two_chunks', 'three_or_more_chunks',
    'parked_fields_per_entry', 'cw8', 'cw4', 'ragged_last_column_group', 'tall_columns_large_fan',
    'distances_ascending', 'distances_descending', 'distances_repeated', 'distances_near_field', 'distances_aliased',
    'sign_p1', 'sign_m1',
)
# every __global__ kernel of adm_ms_multidist.hip, and every kernel of adm_ms_streamed.hip that a fan-out runs over the E detector
# entries instead of the B positions -> the rows that take it over its thresholds (all of them run by test_counts)
KERNEL_ROWS = {
    'md_fanout_kernel': ('adm_ms_multidist.hip', ['B3_D63_M1', 'B3_D64_M1', 'B1_D64_M64', 'B257_D2_M1', 'tall_B2_D33_M1']),
    'md_fanin_kernel': ('adm_ms_multidist.hip', ['B3_D63_M1', 'B3_D64_M1', 'B1_D64_M64', 'B257_D2_M1', 'tall_B2_D33_M1']),
    'st_row_kernel': ('adm_ms_streamed.hip', ['B5_D64_M1', 'B257_D2_M1', 'B1_D64_M64']),
    'st_det_kernel': ('adm_ms_streamed.hip', ['B5_D64_M1', 'B257_D2_M1', 'B1_D64_M64', 'B3_D33_M4']),
    'st_loss_reduce_kernel': ('adm_ms_streamed.hip', ['B64_D4_M1', 'B65_D4_M1', 'B4_D64_M1', 'B5_D64_M1', 'B129_D2_M1', 'B257_D2_M1']),
}


# ---------------------------------------------------------------------------------------------------------------- the engine
def run(A, ctx, case, engine=None, target=None, **engine_kw):
    """launch of test_gpu_multidist3d.py on a fan-out engine (a new one, closed afterwards, unless ``engine`` is given), with every
    entry's loss sum beside its results."""
    eng = MD._engine(A, ctx, case, case['dists'], **engine_kw) if engine is None else engine
    assert eng.streamed is True and eng.n_dists == eng.det_per_pos == len(case['dists'])
    out = MD.launch(ctx, eng, case, case['target'] if target is None else target)
    out['loss_sum'] = eng.loss_sums(len(case['pos']) * eng.det_per_pos)
    out['gprobe_raw'] = MM.c2(out['gprobe'])
    if engine is None:
        eng.plan.close()
    return out


def dressed(case, res):
    """A built case with an engine's (or a stand-in's) results in the layout check_entries reads."""
    out = dict(case)
    out.update(res)
    return out


def as_engine(case, sfx='_32'):
    """The restatement's own run dressed as an engine result (the coverage test judges the fp32 restatement, and perturbed fp64
    results, with the GPU module's checks)."""
    return dressed(case, dict(pred=case['pred' + sfx], loss=case['loss' + sfx], grad=case['grad' + sfx], gprobe=case['gprobe' + sfx],
                              loss_sum=case['loss_e' + sfx]))


# ---------------------------------------------------------------------------------------------------------------- each entry
def check_entries(res, bars=BARS, what='', quiet=False):
    """ms_matrix.check, then every entry's prediction and loss sum and every mode's probe gradient on its own.  Every item is
    judged: one without signal (below 1e-3 of the largest) fails here."""
    MM.check(res, bars)
    E, M = len(res['pred_o']), len(res['gprobe_o'])
    assert len(res['pred']) == E and len(res['loss_sum']) == E and len(res['loss_e_o']) == E and len(res['gprobe']) == M, what
    out = {}
    out['pred'] = CM._items(res['pred'], res['pred_o'], res['pred_32'], bars['pred'], what + ' pred of an entry')
    out['loss_sum'] = CM._items(res['loss_sum'], res['loss_e_o'], res['loss_e_32'], bars['loss'], what + ' loss sum of an entry')
    out['gprobe'] = CM._items(res['gprobe'], res['gprobe_o'], res['gprobe_32'], bars['grad_abs'], what + ' probe gradient of a mode',
                              cap=bars['grad'])
    for k, n in (('pred', E), ('loss_sum', E), ('gprobe', M)):
        judged, _, _, silent = out[k]
        assert judged == n and silent == 0, (what, k, 'items without signal', silent, 'of', n)
    if not quiet:
        print(what, 'each item (judged, worst, fp32 restatement there, without signal):', {k: '%d %.2e (%.2e) %d' % v for k, v in out.items()})
    return out


def fractions(res, bars=BARS):
    """How much of every bar check_entries applies a result uses: whole arrays and the worst item."""
    item = lambda x, x64: np.sqrt((np.abs(np.asarray(x) - x64) ** 2).reshape(len(x64), -1).sum(1) / (np.abs(x64) ** 2).reshape(len(x64), -1).sum(1))
    return dict(pred=MM.rel(res['pred'], res['pred_o']) / bars['pred'],
                pred_each=item(res['pred'], res['pred_o']).max() / bars['pred'],
                loss=abs(res['loss'] - res['loss_o']) / (bars['loss'] * abs(res['loss_o'])),
                loss_each=item(res['loss_sum'], res['loss_e_o']).max() / bars['loss'],
                grad=MM.rel(res['grad'], res['grad_o']) / bars['grad'],
                gprobe=MM.rel(res['gprobe'], res['gprobe_o']) / bars['grad'],
                gprobe_each=item(res['gprobe'], res['gprobe_o']).max() / bars['grad'])


# ---------------------------------------------------------------------------------------------------------------- perturbations
def _copy(res):
    out = dict(res)
    for k in ('pred', 'loss_sum', 'grad', 'gprobe'):
        out[k] = np.array(out[k])
    return out


def perturbed(case, kind, **kw):
    """The fp64 restatement's result made wrong in ONE way, dressed as an engine result:
    'drop_last_entry'  the last entry is never run: its prediction and loss sum stay zero;
    'distance_major'   the entries come back in the order d * B + b;
    'wrong_distance'   entry (b, d) is predicted with distance d + 1;
    'fanin_short'      the fan-in sums D - 1 distances: the gradients miss the last distance's term;
    'mode_swapped'     mode m's probe gradient is mode m + 1's."""
    out = _copy(as_engine(case, '_o'))
    D = len(case['dists'])
    B = len(case['pos'])
    if kind == 'drop_last_entry':
        out['pred'][-1] = 0
        out['loss_sum'][-1] = 0
    elif kind == 'distance_major':
        order = np.arange(B * D).reshape(B, D).T.reshape(-1)          # place d * B + b holds entry b * D + d
        out['pred'], out['loss_sum'] = out['pred'][order], out['loss_sum'][order]
    elif kind == 'wrong_distance':
        b, d = kw['b'], kw['d']
        Py, Px = case['probes'].shape[-2:]
        phys = O.Physics((Py, Px), MD.ENERGY_EV, MD.PSIZE_CM, free_prop_cm=case['dists'][0], sign_convention=case['sign_convention'])
        tiles, _ = O.extract_tiles(case['obj'].astype(np.float64), case['pos'][b:b + 1], (Py, Px))
        e = entry_index(b, d, D)
        out['pred'][e] = MR.predict(tiles, case['probes'].astype(np.complex128), phys, [case['dists'][d + 1]])[0]
        out['loss_sum'][e] = CM.loss_sums_of(out['pred'][e:e + 1], case['meas'][e:e + 1])[0]
    elif kind == 'fanin_short':
        # the last distance's entries with a residual of exactly zero add nothing to the gradients
        meas = np.array(case['meas'], np.float64)
        meas[D - 1::D] = case['pred_o'][D - 1::D]
        short = MD.ref_fanout(dict(case, meas=meas), 'float64')
        out['grad'], out['gprobe'] = short['grad'], short['gprobe']
    elif kind == 'mode_swapped':
        m = kw['m']
        out['gprobe'][m] = out['gprobe'][m + 1]
    else:
        raise KeyError(kind)
    return out
