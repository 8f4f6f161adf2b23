"""The CTF value-domain table (tests/ctf_value_matrix.py) against the references and the kernel sources, on the CPU:

* every referenced case leaves room: the float32 restatements' own distance from fp64 stays within one third of BARS (pred, loss,
  grad, gkappa) and within BARS['grad'] element-wise for dL/dd; every figure of V.ROOM, V.INV_ERR32 and of DESIGN.md's table is
  recomputed;
* the free ranges are what the rule admits, recomputed: the lowest min I per field (V.LOW_I_MIN), the smallest data scale per raw
  type (V.DATA_SMALL); the crossing cases meet their cap and the restatement pair agrees on I > 0 wherever a case needs it;
* every class feeds the kernels what it promises;
* each mistake of V.FWD_MUTANTS / V.INV_MUTANTS, switched on in a float32 mirror that unmutated gives the restatement's bits, is
  rejected by a named case by at least ten bars; the same mutant against every case of ctf_matrix, ctf_dist_matrix and ctfinv_matrix
  gives what V.CAUGHT_BEFORE records -- None for those the existing tables accept, which is the gap, and the old case that already
  rejects each of the others;
* the texts of the sources the classes are there for are still there, every class has its GPU test and every GPU test names the
  kernels it reaches."""
import os
import re

import numpy as np
import pytest

from tests import ctf_dist_ref as DR
from tests import ctf_matrix as CM
from tests import ctf_value_matrix as V
from tests import ctfinv_matrix as IM

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ALL = [p for cls in V.CASES for p in V.params(cls)]
REFERENCED = [p for p in ALL if V.judged(p)]
all_ids = lambda p: '%s-%s' % (p[0], V.case_id(p))
INV_ALL = [p for cls in V.INV_CASES for p in V.inv_params(cls)]


def _read(*p):
    with open(os.path.join(ROOT, *p)) as f:
        return f.read()


# ------------------------------------------------------------------------------------------------------------ the reference pair alone
@pytest.mark.parametrize('p', REFERENCED, ids=all_ids)
def test_the_reference_pair_leaves_room(p):
    """The one-third rule for every quantity a case is judged by, and what else its judgement needs."""
    c = V.case(*p)
    keys = V.judged(p)
    r = V.room(c, keys)
    print(all_ids(p), {k: '%.3f' % v for k, v in r.items()}, 'min I %.4g' % c['o64']['I'].min())
    for k, v in r.items():
        assert v <= (1. if k == 'gdists' else V.THIRD), (all_ids(p), k, v)
    for o in ('o32', 'o32h'):                      # the prediction clips the same pixels in all three runs
        assert np.array_equal(c[o]['I'] > 0, c['o64']['I'] > 0), (all_ids(p), o)
    if 'gkappa' in keys:                           # a normal float32 with room: its one rounding is a relative 6e-8
        assert abs(c['o64']['grad_lg_kappa']) >= V.GKAPPA_FLOOR, (all_ids(p), c['o64']['grad_lg_kappa'])
    if 'gdists' in keys:
        assert np.abs(c['o64']['grad_dists']).max() > 0 and np.isfinite(c['o64']['grad_dists']).all()
    assert np.array_equal(c['model_dists'], DR.round32(c['model_dists'])) and len(c['model_dists']) == c['nd']


def test_the_stated_figures_are_the_recomputed_ones():
    """V.ROOM per class, and the same figures in DESIGN.md's table."""
    worst = {}
    for p in REFERENCED:
        for k, v in V.room(V.case(*p), V.judged(p)).items():
            worst.setdefault(p[0], {})[k] = max(worst.get(p[0], {}).get(k, 0.), v)
    assert set(worst) == set(V.ROOM)
    for cls, w in worst.items():
        print(cls, {k: '%.4f' % v for k, v in w.items()})
        assert set(w) == set(V.ROOM[cls])
        for k, v in w.items():
            assert v <= V.ROOM[cls][k] <= 2 * v + 0.002, (cls, k, v, V.ROOM[cls][k])
    design = _read('DESIGN.md')
    assert 'the CTF value-domain matrix' in design
    rows = dict(re.findall(r'^  \| `(\w+)` \| ([^\n]*?) \|$', design, re.M))
    for cls, w in V.ROOM.items():
        assert cls in rows, cls
        assert [float(x) for x in rows[cls].split(' | ')[:5]] == [w[k] for k in ('pred', 'loss', 'grad', 'gkappa', 'gdists')], (cls, rows[cls])
    for (cls, name), e in V.INV_ERR32.items():
        assert re.search(r'^  \| `%s` `%s` \| %s \|' % (cls, re.escape(name), re.escape('%.1e' % e)), design, re.M), (cls, name)


def test_the_low_I_ladder():
    """V.LOW_I_MIN is the lowest rung at and above which the rule holds, per field; the next rung breaks it (the delta gradient)."""
    for f in V.FIELDS:
        fr = {}
        for rung in V.LOW_I_LADDER:
            c = V.ref_pair(V.low_I(f, rung))
            assert abs(c['o64']['I'].min() / rung - 1) < 1e-2, (f, rung, c['o64']['I'].min())
            fr[rung] = V.room(c)
            print(f, rung, {k: '%.3f' % v for k, v in fr[rung].items()})
        ok = [all(v <= (1. if k == 'gdists' else V.THIRD) for k, v in fr[r].items()) for r in V.LOW_I_LADDER]
        admitted = [r for r, good in zip(V.LOW_I_LADDER, np.cumprod(ok)) if good]
        assert admitted and admitted[-1] == V.LOW_I_MIN[f], (f, admitted)
        assert admitted[-1] != V.LOW_I_LADDER[-1] and fr[V.LOW_I_LADDER[len(admitted)]]['grad'] > 1, f
        assert [kw['rung'] for ff, kw in V.CASES['low_I'] if ff == f] == admitted
    assert V.LOW_I_MIN == {(32, 16, 2): 0.01, (16, 16, 3): 1e-3}


def test_the_small_data_ladder():
    """V.DATA_SMALL: the smallest scale of the ladder at which dL/dd of the restatement keeps within its bar, per raw type."""
    for raw in V.RAWS:
        ok = []
        for s in V.DATA_SMALL_LADDER:
            good = all(V.leaves_room(V.ref_pair(V.data(f, raw, 'small', scale=s)), ('pred', 'loss', 'grad', 'gkappa', 'gdists')) for f in V.FIELDS)
            ok.append(good)
        admitted = [s for s, good in zip(V.DATA_SMALL_LADDER, np.cumprod(ok)) if good]
        assert admitted and admitted[-1] == V.DATA_SMALL[raw], (raw, ok)
    worst = max(V.room(V.ref_pair(V.data(f, 'intensity', 'small', scale=1e-4)))['gdists'] for f in V.FIELDS)
    print('intensity x 1e-4: dL/dd %.2f bars' % worst)
    assert worst > 1.5


def test_the_crossing_cases():
    """I passes through 0 (pixels at and below -tol, none within tol: the cap is met with room), and both float32 restatements pass
    the judgement the GPU gets; the gapped clip cases clip an eighth of the pixels of a distance and keep |I| >= 0.01."""
    for p in V.params('crossing_zero'):
        c = V.case(*p)
        I = c['o64']['I']
        if p[2].get('clip'):
            assert (I <= 0).sum() >= I[0].size // 8 and np.abs(I).min() >= 0.01, (all_ids(p), np.abs(I).min())
            continue
        for o in ('o32', 'o32h'):
            f = V.judge_crossing(c[o]['pred'], c[o]['loss'], c)
            assert f['pred'] <= V.BARS['pred'] * V.THIRD and f['loss'] <= V.BARS['loss'] * V.THIRD, (all_ids(p), f)
        print(all_ids(p), f)
        assert f['clipped'] >= 3 and f['within_tol'] == 0 and f['tol'] < 1e-4
        assert I.min() < -0.2 and V.crossing_tol(c) == f['tol']
        with np.errstate(all='ignore'):           # what a dropped guard does there
            assert np.isfinite(V.mirror(c)['grad_delta']).all() and not np.isfinite(V.mirror(c, 'q_not_zeroed')['grad_delta']).all()


def test_the_classes_are_what_they_claim():
    fields = {f for cls in V.CASES for f, _ in V.CASES[cls]}
    assert fields == set(V.XI_FIELDS) and set(V.FIELDS) == set(CM.FIELDS[1:3]) and all(f in CM.FIELDS for f in V.XI_FIELDS)
    for f in V.FIELDS:                                          # several distances in one C3 block, idle C4 slots
        assert {'c3_block_spans_distances', 'c4_idle_slots'} <= CM.classes(*f), f
        assert {ff for ff, _ in V.CASES['distances']} == {ff for ff, _ in V.CASES['physical_scales']} == set(V.XI_FIELDS)
    for cls in ('kappa_ladder', 'contrast', 'low_I', 'crossing_zero', 'data', 'exact', 'nonfinite_data'):
        assert {ff for ff, _ in V.CASES[cls]} == set(V.FIELDS), cls
    for p in V.params('kappa_ladder'):
        c, k = V.case(*p), p[2]['lg_kappa']
        assert float(c['lg_kappa']) == float(np.float32(k)) and 0.9 < c['o64']['I'].min() and c['o64']['I'].max() < 1.1
        assert (np.float32(1. / 10. ** float(c['lg_kappa'])) == 0) == (k == V.KAPPA_ZERO)
    assert min(V.KAPPA_LADDER) < 0 and 0. in V.KAPPA_LADDER and max(V.KAPPA_LADDER) >= 8      # kappa < 1, = 1, >= 1e8
    for p in V.params('contrast'):
        lo = V.case(*p)['o64']['I'].min()
        assert (0.75 < lo < 0.85) if p[2]['scale'] == 3. else (0.3 < lo < 0.45), (all_ids(p), lo)
    for p in V.params('distances'):
        c, kind = V.case(*p), p[2]['kind']
        if kind in V.DIST_SCALES:
            assert abs(V.max_xi(c) / (V.DIST_SCALES[kind] * CM.max_xi(c['ny'], c['nx'], CM.dists_for(c['nd']))) - 1) < 0.11
        elif kind == 'zero':
            assert c['model_dists'][1] == 0 and (np.delete(c['model_dists'], 1) > 0).all()
            # the fp64 restatement reproduces the closed form
            assert np.abs(c['o64']['pred'][1] - V.closed_form_at_zero_distance(c)).max() < 1e-14
        else:
            assert c['model_dists'][0] < 0 and (c['model_dists'][1:] > 0).all()
    assert min(V.max_xi(V.case(*p)) for p in V.params('distances')) < 0.15
    for p in V.params('physical_scales'):
        c = V.case(*p)
        t = V.case('plain', p[1], {})
        assert abs(V.max_xi(c) / V.max_xi(t) - 1) < 1e-6 and V.rel(c['o64']['pred'], t['o64']['pred']) < 1e-6
        assert (c['energy'], c['psize']) == (p[2]['energy'], p[2]['psize']) != (CM.ENERGY_EV, CM.PSIZE_CM)
    g = [np.abs(V.case('physical_scales', V.FIELDS[0], dict(energy=e, psize=q))['o64']['grad_dists']).max() for e, q in V.PHYSICAL]
    assert max(g) / min(g) > 1e5, g
    for p in V.params('data'):
        c, kind = V.case(*p), p[2]['kind']
        if kind == 'zeros':
            assert 0.1 < (c['data'] == 0).mean() < 0.2 and (c['data'] >= 0).all()
        elif kind == 'negated':
            assert abs((c['data'] < 0).mean() - V.NEGATED_SHARE) < 0.06 and np.array_equal(np.abs(c['data']), c['plain_data'])
        else:
            s = V.DATA_LARGE if kind == 'x1e4' else V.DATA_SMALL[c['raw']]
            assert abs(c['data'].mean() / c['plain_data'].mean() / s - 1) < 1e-6
    for p in V.params('exact'):
        c, kind = V.case(*p), p[2]['kind']
        t = V.case('plain', p[1], {})
        if kind in V.BETA:
            b = c['obj'][..., 1]
            assert (np.isnan(b).all() if kind == 'beta_nan' else (b == np.float32(V.BETA[kind])).all())
            assert np.array_equal(c['obj'][..., 0], t['obj'][..., 0]) and t['obj'][..., 1].any()
        else:
            assert not c['obj'][..., 0].any() and (c['o64']['pred'] == 1).all() and not c['o64']['grad_dists'].any()
            assert c['o64']['grad_lg_kappa'] == 0 and ((c['data'] == 1).all() == (kind == 'zero_object_unit_data'))
    for p in V.params('nonfinite_data'):
        c = V.case(*p)
        bad = ~np.isfinite(c['data'])
        assert bad.sum() == 2 and bad[1].sum() == 2 and np.isnan(c['data']).sum() == 1
    c = V.inv_nonfinite()
    bad = ~np.isfinite(c['data'])
    assert c['data'].shape[0] == c['max_batch'] == 3 and bad.sum() == 2 and bad[1].sum() == 2
    assert IM.geometry(c['ny'], c['nx'], c['nd'], 3)['i1_spans_batch'][0]


# ------------------------------------------------------------------------------------------------------------ the inversion
@pytest.mark.parametrize('p', INV_ALL, ids=lambda p: '%s-%s' % p)
def test_the_inversion_figures(p):
    """V.INV_ERR32 per case: not below what is recomputed, not above twice that; no case beyond 1e-4."""
    c = V.inv_case(*p)
    e = V.rel(c['o32'], c['o64'])
    print(c['name'], '%.2e (stated %.1e)' % (e, V.INV_ERR32[p]))
    assert e <= V.INV_ERR32[p] <= 2 * e and V.INV_ERR32[p] <= V.INV_ADMIT, (p, e)
    assert np.isfinite(c['o64']).all() and c['bar'] == 3 * V.INV_ERR32[p]
    if p[0] == 'inv_data':
        assert (np.abs(c['o64']).max() > 600) == (p[1] == 'contrast_x1e4')
        if p[1] != 'contrast_x1e4':
            assert (c['data'] < 0).mean() > 0.25 and (c['data'] == 0).any()


def test_the_inversion_table():
    assert set(V.INV_ERR32) == set(INV_ALL)
    assert {kw['field'] for kw in V.INV_CASES['inv_kappa_ladder'].values()} == {IM.PHASE_FIELD, (16, 32, 2)}
    assert all(kw['field'] == IM.PHASE_FIELD for cls in ('inv_alpha_ladder', 'inv_data') for kw in V.INV_CASES[cls].values())
    assert V.INV_KAPPA_LADDER == (-0.5, 0., 0.7, 3., 8., 50.) and V.INV_ALPHA_LADDER == (1e-30, 1e-20, 1e-6, 1., 1e3, 1e6)
    # alpha from nothing beside the denominator to all of it: the phase shrinks by five decades and more
    top = [np.abs(V.inv_case('inv_alpha_ladder', 'alpha-%g' % a)['o64']).max() for a in V.INV_ALPHA_LADDER]
    assert top[0] / top[-1] > 1e5 and np.float32(V.INV_ALPHA_LADDER[0]) > np.finfo(np.float32).tiny


# ------------------------------------------------------------------------------------------------------------ mutations
def test_the_mirrors_restate_the_references():
    """Unmutated, the mirrors give the bits of the committed float32 restatements."""
    for p in REFERENCED[::3]:
        c = V.case(*p)
        for rounding, o in (('device', 'o32'), ('host', 'o32h')):
            m = V.mirror(c, rounding=rounding)
            for k in ('pred', 'grad_delta') + (('grad_dists',) if rounding == 'device' else ()):
                assert np.array_equal(m[k], c[o][k]), (all_ids(p), rounding, k)
            assert m['loss'] == c[o]['loss'] and m['grad_lg_kappa'] == c[o]['grad_lg_kappa'], (all_ids(p), rounding)
    for p in INV_ALL:
        c = V.inv_case(*p)
        assert np.array_equal(V.inv_mirror(c), c['o32'].reshape(c['nb'], c['ny'], c['nx'])), p


@pytest.mark.parametrize('mut', V.FWD_MUTANTS + V.INV_MUTANTS)
def test_every_mistake_is_rejected_here_and_what_the_old_tables_make_of_it(mut):
    """At least ten bars in every case named for the mutant; and the first case of the existing tables that rejects it, or none."""
    assert V.MUTANT_CASES[mut]
    for p in V.MUTANT_CASES[mut]:
        assert (p in INV_ALL) if len(p) == 2 else ((p[1], p[2]) in V.CASES[p[0]]), p
        with np.errstate(all='ignore'):
            n = V.rejection(mut, p)
        print('%s at %s: %.3g bars' % (mut, p, n))
        assert n >= V.REJECT, (mut, p, n)
        assert V.rejection(None, p) <= 1, p                    # ... and the unmutated mirror passes it
    with np.errstate(all='ignore'):
        before = V.rejected_before(mut)
    print('%s in the existing tables: %s' % (mut, before or 'accepted by every case'))
    assert before == V.CAUGHT_BEFORE[mut], (mut, before)


def test_the_gap_is_real():
    assert set(V.CAUGHT_BEFORE) == set(V.MUTANT_CASES) == set(V.FWD_MUTANTS + V.INV_MUTANTS)
    gap = {m for m, old in V.CAUGHT_BEFORE.items() if old is None}
    assert gap == {'no_abs_on_data', 'abs_in_inversion', 'clipped_kept_in_gdists', 'inv_kappa_clamped_to_1', 'inv_kappa_flushed_below_1e-7',
                   'dscale_at_table_energy'}
    with np.errstate(all='ignore'):
        assert V.rejected_before(None) is None                                        # the unmutated mirrors pass every old case


# ------------------------------------------------------------------------------------------------------------ the sources
def test_the_sources_still_hold_what_the_classes_are_there_for():
    src = {n: _read('adorym_amd', 'csrc', n) for n in {f for f, _, _ in V.SOURCE_TIES.values()}}
    reached = set()
    for what, (name, text, classes) in V.SOURCE_TIES.items():
        assert text in src[name], '%s: %r left %s; the classes %s were there for it' % (what, text, name, classes)
        assert classes and all(c in V.CLASS_TESTS for c in classes), what
        reached |= set(classes)
    assert reached == set(V.CLASS_TESTS), set(V.CLASS_TESTS) ^ reached
    assert set(V.CLASS_TESTS) == set(V.CASES) | set(V.INV_CASES) | {'inv_nonfinite_batch_entry'}
    # fabsf appears once in the forward group (the measured value) and nowhere in the inversion, which uses the data as given
    code = lambda n: re.sub(r'//[^\n]*', '', src[n])
    assert len(re.findall(r'\bfabsf?\(', code('adm_holo_ctf.hip'))) == 1 and not re.search(r'\bfabsf?\(', code('adm_ctf_invert.hip'))
    assert len(re.findall(r'I > 0\.f', code('adm_holo_ctf.hip'))) == 2               # the prediction and q
    assert 'The data are used as given' in src['adm_ctf_invert.hip'] and 'the model never reads beta' in src['adm_holo_ctf.hip']


def test_every_class_has_its_gpu_test_and_every_gpu_test_names_its_kernels():
    text = _read('tests', 'test_gpu_ctf_value_domain.py')
    tests = dict(re.findall(r'^def (test_\w+)\([^)]*\):\n    """(.*?)"""', text, re.M | re.S))
    assert set(tests) == set(V.CLASS_TESTS.values()), set(tests) ^ set(V.CLASS_TESTS.values())
    for cls, name in V.CLASS_TESTS.items():
        kernels = V.INV_KERNELS if cls.startswith('inv_') else V.FWD_KERNELS
        m = re.match(r'Reaches: (\w+(?:, \w+)*)', tests[name])
        assert m and tuple(m.group(1).split(', ')) == kernels, (name, tests[name][:80])
        if cls in V.CASES:
            assert re.search(r"^@pytest\.mark\.parametrize\(\*\*cases_of\('%s'\)\)\ndef %s\(" % (cls, name), text, re.M), cls
        elif cls in V.INV_CASES:
            assert re.search(r"^@pytest\.mark\.parametrize\(\*\*inv_cases_of\('%s'\)\)\ndef %s\(" % (cls, name), text, re.M), cls
    # the kernels named exist, and the module goes through both forward/adjoint entries and the inversion's
    for n, ks in (('adm_holo_ctf.hip', V.FWD_KERNELS), ('adm_ctf_invert.hip', V.INV_KERNELS)):
        s = _read('adorym_amd', 'csrc', n)
        assert all(re.search(r'__global__ __launch_bounds__\(\d+\) void %s\(' % k, s) for k in ks), n
    assert 'adm_ctf_fwd_adj(' in _read('tests', 'test_gpu_ctf.py') and 'adm_ctfd_fwd_adj(' in _read('tests', 'test_gpu_ctf_dist.py')
    assert 'calls = dict(host=(host_launch, dict(c, dists=c[\'model_dists\'])), device=(device_launch, c))' in text
    assert "overwrite=True, seed='nan')" in text and "want_grad=False, seed='nan')" in text
