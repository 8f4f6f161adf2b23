"""CPU: the fan-out count matrix (tests/fan_matrix.py, tests/test_gpu_fanout_domain.py) against the sources and against the restatement alone.

* the thresholds and index expressions of the sources are parsed and compared with the mirrors: a changed limit, stride or index
  fails here until the mirror and the rows follow;
* the rows stand on both sides of every threshold; every __global__ kernel of adm_ms_multidist.hip and every kernel the fan-out
  re-runs over entries has rows; no pixel of any row is covered by more than 64 tiles;
* on the restatement alone: its fp32 run stays within a third of every bar the GPU module applies, whole and item by item, and
  passes the GPU module's own judgement; the fp64 run made wrong in one entry, order, distance, term or mode does not.
"""
import os
import re

import numpy as np
import pytest

from tests import count_matrix as CM
from tests import fan_matrix as FM
from tests import st_matrix as SM

HERE = os.path.dirname(os.path.abspath(__file__))
squeeze = lambda text: ' '.join(text.split())


# ------------------------------------------------------------------------------------------------------------ the sources
def test_thresholds_of_the_sources_are_the_mirrors():
    api = CM.read('adm_api.hip')
    fan = squeeze(CM.function_body(api, r'int\s+adm_plan_set_detector_fanout\s*\('))
    assert 'if (n < 0 || n > %d) return fail(ADM_ERR_INVALID, "adm_plan_set_detector_fanout: n must be in [1, %d]' % (FM.MAX_FAN, FM.MAX_FAN) in fan
    m = re.search(r'#define\s+PGR_CHUNK\s+(\d+)', api)
    assert m and int(m.group(1)) == FM.PGR_CHUNK == 32
    assert 'd.n_modes < 1 || d.n_modes > %d' % FM.MAX_MODES in api
    # the sections of the workspace that scale with the E = B * D entries
    lay = squeeze(CM.function_body(api, r'WsLayout\s+ws_layout\s*\('))
    assert 'const size_t E = fan ? B * (size_t)plan->n_fan : B;' in lay
    for line in ('w.det = take(E * M * det);', 'w.fan_field = take(fan ? E * M * fld : 0);', 'w.fan_pos = take(fan ? E * sizeof(int2) : 0);'):
        assert line in lay, line
    assert re.search(r'w\.loss_part = take\(E \* \(', lay)
    # a launch with a shared probe set sums its B probe-gradient slots with the one-level kernel, fan-out or not
    assert 'ADM_HIP(probe_grad_reduce(p.grad_probe, batch, probe_elems, (float2*)grad_probe, plan->ctx->stream));' in squeeze(api)
    st = squeeze(CM.read('adm_ms_streamed.hip'))
    loss = squeeze(CM.function_body(CM.read('adm_ms_streamed.hip'), r'void\s+st_loss_reduce_kernel\s*\('))
    assert 'const int b = blockIdx.x * %d + threadIdx.x; if (b >= batch) return;' % FM.RED_NT in loss
    assert 'hipLaunchKernelGGL(st_loss_reduce_kernel, dim3((batch + %d) / %d), dim3(%d), 0, st, part, ncg, batch, p.loss_sum);' % (
        FM.RED_NT - 1, FM.RED_NT, FM.RED_NT) in st
    # with a fan-out the detector's row launches, st_det_kernel and the loss reduction take batch * n entries
    assert 'hipLaunchKernelGGL(st_row_kernel, dim3(batch * fo->n * ngr), dim3(ST_ROW_NT), 0, st, pd, r, fo->fld);' in st
    assert 'e = fo ? detect(pd, batch * fo->n, fo->fld) : detect(p, batch, fld);' in st
    assert FM.loss_reduce_workgroups(256) == 1 and FM.loss_reduce_workgroups(257) == 2 and FM.loss_reduce_workgroups(514) == 3


def _c_index(expr):
    """A C index expression of the kernels as a Python function of (b, d, m, D, M)."""
    expr = expr.replace('(size_t)', '').replace('q.n', 'D').replace('p.n_modes', 'M')
    assert re.fullmatch(r'[bdmDM+*() ]+', expr), expr
    return eval('lambda b, d, m, D, M: ' + expr)


def test_index_expressions_of_the_sources_are_the_mirrors():
    md = CM.read('adm_ms_multidist.hip')
    for kernel, access in (('md_fanout_kernel', 'st_col_store'), ('md_fanin_kernel', 'st_col_load')):
        body = squeeze(CM.function_body(md, r'void\s+%s\s*\(' % kernel))
        assert 'const int b = bm / p.n_modes, m = bm - b * p.n_modes;' in body and 'for (int d = 0; d < q.n; ++d) {' in body, kernel
        assert 'const float2* hs = q.hs + (size_t)d * row;' in body, kernel
        found = re.findall(r'%s\(g, q\.dfld \+ \((.+?)\) \* row, Px, c0\);' % access, body)
        assert len(found) == 1, (kernel, found)
        f = _c_index(found[0])
        for B, D, M in ((3, 64, 1), (1, 64, 64), (5, 3, 2), (257, 2, 1)):
            got = [f(b, d, m, D, M) for b in range(B) for d in range(D) for m in range(M)]
            assert got == [FM.det_field_index(b, d, m, D, M) for b in range(B) for d in range(D) for m in range(M)], (kernel, B, D, M)
            assert got == list(range(B * D * M)), (kernel, B, D, M)                 # every field once, none outside the buffer
            assert all(f(b, d, 0, D, M) // M == FM.entry_index(b, d, D) for b in range(B) for d in range(D))
    # the fan-out multiplies with H, the fan-in with conj(H), and adds in ascending d
    assert 'g.fld[i] = cmul(sp[j], hs[(size_t)y * Px + c0 + (i - y * g.Px)]);' in squeeze(CM.function_body(md, r'void\s+md_fanout_kernel\s*\('))
    assert 'acc[j] = cadd(acc[j], cmulc(g.fld[i], hs[(size_t)y * Px + c0 + (i - y * g.Px)]));' in squeeze(CM.function_body(md, r'void\s+md_fanin_kernel\s*\('))
    # st_det_kernel reads field (entry * M + m), target / pred pixel (entry * Py + y) * Px + x and parks at (entry * M + m)
    det = squeeze(CM.function_body(CM.read('adm_ms_streamed.hip'), r'void\s+st_det_kernel\s*\('))
    assert 'st_col_load(g, fld + ((size_t)b * M + m) * row, Px, c0);' in det and 'float2* dq = p.det + ((size_t)b * M + m) * row;' in det
    assert 'const size_t di = ((size_t)b * Py + my) * Px + mx;' in det
    # the host: offsets of a round and the loss read-backs count entries
    with open(os.path.join(os.path.dirname(HERE), 'adorym_amd', 'propagate.py')) as fh:
        host = fh.read()
    for line in ('e = o * self.det_per_pos', 'ent = batch * self.det_per_pos',
                 'B, last = self._B * self.det_per_pos, None if last is None else last * self.det_per_pos',
                 "'B': self._B * per, 'last': None if last is None else last * per",
                 'return self._pred.view(0, (self._B * self.det_per_pos,) + self.probe_size).get()'):
        assert line in host, line


# ------------------------------------------------------------------------------------------------------------ the rows
def test_rows_on_both_sides_of_every_threshold():
    have = {}
    for name in FM.CASES:
        for c in FM.classes_of(name):
            have.setdefault(c, []).append(name)
    missing = [c for c in FM.REQUIRED_CLASSES if c not in have]
    assert not missing, missing
    # the figures the issue names
    counts = {(s['B'], s['D'], s['M']) for s in FM.CASES.values() if s['P'] == FM.FIELD and not s['kw']}
    assert {(64, 4, 1), (65, 4, 1), (4, 64, 1), (5, 64, 1), (129, 2, 1), (257, 2, 1), (3, 63, 1), (3, 64, 1), (3, 33, 1), (3, 3, 1),
            (3, 2, 64), (3, 33, 4), (1, 64, 64), (32, 3, 2), (33, 3, 2), (65, 2, 2)} <= counts
    assert [B * D for B, D, _ in ((64, 4, 1), (65, 4, 1), (4, 64, 1), (5, 64, 1), (129, 2, 1), (257, 2, 1))] == [256, 260, 256, 320, 258, 514]
    tall = FM.CASES['tall_B2_D33_M1']
    assert (tall['P'], tall['B'], tall['D'], tall['M']) == ((1025, 12), 2, 33, 1) and SM.geometry(1025, 12)['cw'] == 4
    assert SM.geometry(*FM.FIELD)['cw_last'] == 4 and SM.geometry(*FM.FIELD)['cw'] == 8
    # the distance axis: every set at (3, D, 2) under both sign conventions
    assert FM.DISTANCE_SETS == {'descending': [5e-4, 3.5e-4, 2e-4, 1e-4], 'repeated': [2e-4, 2e-4, 1e-4], 'near_field': [1e-6, 1e-5, 1e-4],
                                'aliased': [1e-4, 2e-2, 5e-2]}
    for what, dists in FM.DISTANCE_SETS.items():
        for sfx, sg in (('p1', 1), ('m1', -1)):
            s = FM.CASES['%s_%s' % (what, sfx)]
            assert (s['B'], s['D'], s['M']) == (3, len(dists), 2) and s['kw'] == dict(dists=dists, sign_convention=sg)
            cl = FM.classes_of('%s_%s' % (what, sfx))
            assert 'distances_' + what in cl and 'sign_' + sfx in cl
    assert 'distances_aliased' not in FM.classes_of('near_field_p1') and 'distances_near_field' not in FM.classes_of('aliased_p1')
    assert FM.phase_step_at_nyquist(5e-2, FM.FIELD) > 30 and FM.phase_step_at_nyquist(5e-4, FM.FIELD) < 1
    # the rounds and the launches repeated bit for bit
    assert set(FM.TWICE) == {'B5_D64_M1', 'B257_D2_M1'} and set(FM.TWICE) <= set(FM.CASES)
    assert FM.ROUNDS == {'rounds_B7_D3_M2': (7, 3, 2, 3, [3, 2, 2]), 'rounds_B5_D64_M1': (5, 64, 1, 2, [2, 2, 1])}
    assert FM.default_dists(3) == [1e-4, 2e-4, 3.5e-4] and len(set(FM.default_dists(64))) == 64
    assert np.allclose(FM.default_dists(64)[0], 1e-4) and np.allclose(FM.default_dists(64)[-1], 5e-3)


def test_every_fanout_kernel_has_rows():
    found = {}
    md = CM.read('adm_ms_multidist.hip')
    for m in re.finditer(r'__global__\s+(?:__launch_bounds__\((?:[^()]|\([^()]*\))*\)\s+)?void\s+(\w+)\s*\(', md):
        found[m.group(1)] = 'adm_ms_multidist.hip'
    assert md.count('__global__') == len(found) == 2, 'a kernel head the pattern does not read'
    st = CM.read('adm_ms_streamed.hip')
    for k in ('st_row_kernel', 'st_det_kernel', 'st_loss_reduce_kernel'):          # what the fan-out runs over entries
        assert re.search(r'__global__[^;{]*void\s+%s\s*\(' % k, st), k
        found[k] = 'adm_ms_streamed.hip'
    assert found == {k: v[0] for k, v in FM.KERNEL_ROWS.items()}, set(found) ^ set(FM.KERNEL_ROWS)
    for k, (_, rows) in FM.KERNEL_ROWS.items():
        assert rows and all(r in FM.CASES for r in rows), (k, rows)
    with open(os.path.join(HERE, 'test_gpu_fanout_domain.py')) as f:
        gpu = f.read()
    assert "@pytest.mark.parametrize('name', list(FM.CASES))\ndef test_counts(" in gpu
    # the count-domain matrix's own rows of the three streamed kernels stay as they are
    for k in ('st_row_kernel', 'st_det_kernel', 'st_loss_reduce_kernel'):
        assert k in CM.KERNEL_ROWS


def test_cover_bound():
    for name, spec in FM.CASES.items():
        c = CM.cover_max(FM.build(name)['pos'], spec['P'])
        assert c <= CM.MAX_COVER, (name, c)
    for B, D, M, _, _ in FM.ROUNDS.values():
        assert CM.cover_max(FM.build_counts(B, D, M, seed=4)['pos'], FM.FIELD) <= CM.MAX_COVER


# ------------------------------------------------------------------------------------------------------------ the restatement alone
@pytest.mark.parametrize('name', list(FM.CASES))
def test_fp32_restatement_leaves_room_under_every_bar(name):
    case = FM.build(name)
    res = FM.as_engine(case, '_32')
    room = FM.fractions(res)
    print(name, 'yardsticks built in %.2f s; fp32 restatement, fractions of the bars:' % FM.BUILD_SECONDS[name], {k: round(float(v), 4) for k, v in room.items()})
    bad = {k: v for k, v in room.items() if not v <= 1 / 3.}
    assert not bad, (name, bad)
    FM.check_entries(res, FM.BARS, name)                # and the GPU module's own judgement passes on it
    n = np.sqrt((np.abs(case['gprobe_o']) ** 2).reshape(len(case['gprobe_o']), -1).sum(1))
    print(name, 'weakest mode %.2f of the strongest' % (n.min() / n.max()))


def _must_fail(res, what):
    with pytest.raises(AssertionError):
        FM.check_entries(res, FM.BARS, what, quiet=True)


def _measure(case, bad):
    ok = FM.as_engine(case, '_o')
    item = lambda k, i: float(np.linalg.norm(np.asarray(bad[k][i]) - ok[k][i]) / np.linalg.norm(ok[k][i]))
    return item, {k: float(FM.MM.rel(bad[k], ok[k])) for k in ('pred', 'grad', 'gprobe')}


def test_the_bars_see_a_dropped_entry():
    """One entry of 258, 260, 320 or 514 never run (the last one: the second or third workgroup of the loss reduction)."""
    for name in ('B65_D4_M1', 'B5_D64_M1', 'B129_D2_M1', 'B257_D2_M1'):
        case = FM.build(name)
        assert len(case['pred_o']) >= 257
        FM.check_entries(FM.as_engine(case, '_o'), FM.BARS, name + ' fp64', quiet=True)
        _must_fail(FM.perturbed(case, 'drop_last_entry'), name + ' drop')


def test_the_bars_see_distance_major_entries():
    for name in ('B3_D3_M1', 'B5_D64_M1', 'B33_D3_M2', 'repeated_p1'):
        _must_fail(FM.perturbed(FM.build(name), 'distance_major'), name + ' distance-major')


def test_the_bars_see_a_neighbours_distance():
    """Entry (1, 40) of (3, 64, 1) predicted with distance 41 (the geometric ladder: 6 % further)."""
    case = FM.build('B3_D64_M1')
    FM.check_entries(FM.as_engine(case, '_o'), FM.BARS, 'B3_D64_M1 fp64', quiet=True)
    bad = FM.perturbed(case, 'wrong_distance', b=1, d=40)
    item, whole = _measure(case, bad)
    e = item('pred', FM.entry_index(1, 40, 64))
    print('distance 41 at entry (1, 40): %.2e on the entry, %.2e on the whole prediction (bar %.0e)' % (e, whole['pred'], FM.BARS['pred']))
    assert e > 100 * FM.BARS['pred'] and whole['pred'] > 100 * FM.BARS['pred']
    _must_fail(bad, 'wrong distance')


def test_the_bars_see_a_short_fan_in():
    """The fan-in's sum without its last distance, at D = 64 and at D = 2."""
    for name in ('B3_D64_M1', 'B1_D64_M64', 'B257_D2_M1'):
        case = FM.build(name)
        bad = FM.perturbed(case, 'fanin_short')
        _, whole = _measure(case, bad)
        print(name, 'fan-in without the last distance: grad %.2e  gprobe %.2e (bar %.0e)' % (whole['grad'], whole['gprobe'], FM.BARS['grad']))
        assert whole['grad'] > 10 * FM.BARS['grad']
        _must_fail(bad, name + ' short fan-in')


def test_the_bars_see_a_neighbours_mode():
    for name, m in (('B3_D2_M64', 62), ('B1_D64_M64', 0), ('B3_D33_M4', 2)):
        _must_fail(FM.perturbed(FM.build(name), 'mode_swapped', m=m), name + ' mode swapped')
