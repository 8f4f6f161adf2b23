"""The holography value-domain table (tests/holo_value_matrix.py) against the oracle and the kernel source, on the CPU:

* every case leaves room under every bar it is judged by: the float32 oracle's own distance from the fp64 oracle stays within
  one third of it (the cases that cannot be judged in full are exactly those HV.UNJUDGED lists), no band cap is exceeded, and a
  shifted case keeps its registered holograms away from zero;
* PHASE_MAX is the largest rung of the ladder the one-third rule admits, recomputed here;
* every class feeds the kernels what it promises: the share of negative, exactly zero, sign-straddling and masked samples,
  the phases and exponents of the delta/beta objects, the arguments of holo_h;
* four mutations of a float32 restatement of the forward chain (HV.mirror) each move a named case past its bar, so the case is
  shown to bite;
* the guards, masks and transcendental calls of adm_holo.hip the classes are there for are still in the source as the table
  quotes them."""
import os
import re

import numpy as np
import pytest

from tests import holo_matrix as HM
from tests import holo_value_matrix as HV
from tests import value_matrix as VM

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ALL = [p for cls in HV.CASES for p in HV.params(cls)]
all_ids = lambda p: '%s-%s' % (p[0], HV.case_id(p))
THIRD = 1. / 3


# ------------------------------------------------------------------------------------------------------------ the oracle pair alone
@pytest.mark.parametrize('p', ALL, ids=all_ids)
def test_the_oracle_pair_leaves_room(p):
    """The one-third rule for every bar of every case; the exceptions are HV.UNJUDGED, no more and no fewer."""
    c = HV.case(*p)
    cls = p[0]
    if cls == 'zero_probe':
        o, s = c['o64'], c['o32']
        assert not o['pred'].any() and not o['g_obj'].any() and not o['g_probe'].any() and not o['g_dists'].any()
        assert np.isfinite(s['g_aff']).all() and HM.rel(s['g_aff'], o['g_aff']) < HM.BARS['gaff'] * THIRD
        assert abs(o['loss'] / np.mean(o['target'] ** 2) - 1) < 1e-12
        return
    room = HV.room(c)
    print(all_ids(p), {k: '%.3f' % v for k, v in room.items()})
    if cls in HV.UNJUDGED_AGAINST_THE_ORACLE:
        assert HV.max_arg(c) > HV.SINCOS_CLAIM and max(room.values()) > THIRD          # no yardstick: it is not used as one
        e32 = np.abs(HV.energy_defect(c['o32']['pred'], c, np.float32))
        assert e32.max() < 1e-6 and np.abs(HV.energy_defect(c['o64']['pred'], c)).max() < 1e-12
        for k in ('pred', 'g_obj', 'g_probe', 'g_dists', 'g_aff'):
            assert np.isfinite(c['o32'][k]).all()
        return
    if cls == 'all_clamped' and p[2]['axes'] == 'xy':
        assert not c['o64']['g_aff'].any() and not c['o32']['g_aff'].any()
        room.pop('gaff')
    over = tuple(k for k in ('loss', 'grad', 'gaff', 'pred', 'gdists', 'gshift', 'target') if room.get(k, 0) > THIRD)
    assert over == HV.unjudged(p), (all_ids(p), room)
    if not over or over == ('gaff',):
        print(HM.oracle_conditions(c))           # the band caps, and min |T| >= MIN_TARGET of a shifted case


def test_phase_max_is_the_ladders():
    """PHASE_MAX for the smooth and for the broadband inputs: the largest rung at and below which the float32 oracle keeps
    within a third of every bar on all three fields and both sigma; the next rung does not."""
    for broadband, stated in ((False, HV.PHASE_MAX), (True, HV.PHASE_MAX_BROADBAND)):
        ladder = HV.phase_ladder(broadband)
        for rad in HV.LADDER:
            print('broadband %s  %6.0f rad: %s' % (broadband, rad, '  '.join('%s %.3f' % kv for kv in ladder[rad].items())))
        assert HV.phase_max_of(ladder) == stated, (broadband, ladder)
        nxt = HV.LADDER[HV.LADDER.index(stated) + 1]
        assert max(ladder[nxt].values()) > THIRD
    assert HV.RUNGS['max'] == HV.PHASE_MAX and HV.RUNGS['max_broadband'] == HV.PHASE_MAX_BROADBAND
    assert HV.LADDER[-1] < HV.SINCOS_CLAIM < HV.UNITARITY_ARG


def test_the_fresnel_cases_reach_their_rungs():
    k = VM.parse_constants()
    seen = set()
    for p in HV.params('fresnel_phase') + HV.params('unitarity'):
        c = HV.case(*p)
        want = HV.UNITARITY_ARG if p[0] == 'unitarity' else HV.RUNGS[p[2]['rung']]
        assert abs(HV.max_arg(c) / want - 1) < 1e-6, (p, HV.max_arg(c))
        # what holo_h forms in float32 is that argument, and sincos_fast's quotient stays an exact integer of a float
        arg = (np.float32(-(c['sigma'] * HM.O.PI * HV.LAMBDA_NM)) * (c['dists'].max() * np.float32(1e7))) * HV.uv2_of(c['ny'], c['nx'], np.float32)
        assert abs(np.abs(arg).max() / want - 1) < 1e-5 and np.abs(arg).max() * k['two_over_pi'] < 2 ** 23
        seen.add((p[1], p[2].get('rung', 'unitarity'), c['sigma']))
        assert HV.max_arg(HM.inputs(c['ny'], c['nx'], c['nd'])) < 10.3          # the matrix's own inputs
    for f in HV.PHASE_FIELDS:
        assert {(f, r, s) for r in ('100', '1000', 'max', 'unitarity') for s in (1, -1)} <= seen
    assert {ny > nx for ny, nx in HV.PHASE_FIELDS} == {True, False}


def test_the_delta_beta_objects_are_what_they_claim():
    for p in HV.params('delta_beta_turns') + HV.params('delta_beta_absorbing') + HV.params('delta_beta_amplifying'):
        c = HV.case(*p)
        ph, kb = HV.k1_phase(c)
        assert c['unknown_type'] == 'delta_beta'
        if p[0] == 'delta_beta_turns':
            assert 0.95 * HV.PHI_MAX < np.abs(ph).max() <= HV.PHI_MAX * (1 + 1e-6) and (ph > 0).any() and (ph < 0).any()
            assert HV.PHI_MAX >= 6 * 2 * np.pi - 1e-9
        elif p[0] == 'delta_beta_absorbing':
            deep = kb > HV.K1B_UNDERFLOW[0]
            assert deep.sum() >= 4 and kb.max() > 104 and kb.max() <= 120 * (1 + 1e-6) and kb.min() >= 0
            assert 25 < kb[~deep].max() <= HV.K1B_MAX * (1 + 1e-6)
            t = HM.transmission(c['obj'], 'delta_beta', 1, np.float32)
            assert (np.abs(t[deep[:, :, 0]]) < 2.0 ** -126).all() and (np.abs(t) == 0).any()        # denormal, and exactly 0
        else:
            assert abs((kb < 0).mean() - HV.AMPLIFYING_SHARE) < 0.01 and HV.K1B_MIN <= kb.min() < 0.9 * HV.K1B_MIN
    assert {p[2].get('sigma') for p in HV.params('delta_beta_turns')} == {1, -1}


def test_the_data_and_matrices_are_what_they_claim():
    """Shares of negative, exactly zero, sign-straddling and masked samples, recomputed from the inputs alone."""
    for p in HV.params('zero_block'):
        c = HV.case(*p)
        st = HV.sample_stats(c)
        per = c['ny'] * c['nx']
        # (identity: the coordinates miss the pixel centres by an ulp in places, fp64 included; the rim of the block may mix in a neighbour)
        want = (HV.BLOCK - 1) ** 2 if p[2]['matrices'] == 'identity' else (HV.BLOCK - 2) ** 2
        assert st['zero'] * per >= want and st['negative'] == 0, (p, st)
        assert not c['data'][0][HV.block_of(c['ny'], c['nx'], 0)].any() and (c['plain_data'] > 0).all()
        if p[2]['matrices'] == 'offset':
            assert st['min_abs'] >= HM.MIN_TARGET, (p, st)                    # away from the block nothing is near zero
        else:
            assert np.array_equal(c['affine'], np.tile(np.array([[1, 0, 0], [0, 1, 0]], np.float32), [c['nd'], 1, 1]))
    for p in HV.params('negative_data'):
        st = HV.sample_stats(HV.case(*p))
        assert st['negative'] >= 0.01 and st['mixed'] >= 0.01 and st['zero'] == 0 and st['min_abs'] >= HM.MIN_TARGET, (p, st)
        assert abs((HV.case(*p)['data'] < 0).mean() - HV.NEGATED_SHARE) < 0.02
    for p in HV.params('all_clamped'):
        c = HV.case(*p)
        st = HV.sample_stats(c)
        axes = p[2]['axes']
        assert (st['masked_x'] == 1) == ('x' in axes) and (st['masked_y'] == 1) == ('y' in axes), (p, st)
        assert st['masked_x'] >= 0.01 and st['masked_y'] >= 0.01                   # the free axis still has its clamped rim
        cx, cy = HM.clamped_samples(c)
        assert (cx == c['data'].size) == ('x' in axes) and (cy == c['data'].size) == ('y' in axes)
        # nothing but the border pixels reaches the target: bit for bit the target of the border-replicated data
        edge = dict(c, data=HV.border_data(c))
        assert (edge['data'] != c['data']).mean() > 0.5
        t = HM.oracle_run(edge, 'float32')['target']
        assert np.array_equal(HM.bits(t), HM.bits(c['o32']['target'])), p
        if axes == 'xy':       # ... the corner pixel itself
            for d in range(c['nd']):
                y = c['ny'] - 1 if c['affine'][d, 1, 2] > 0 else 0
                x = c['nx'] - 1 if c['affine'][d, 0, 2] > 0 else 0
                assert np.array_equal(HM.bits(c['o32']['target'][d]), HM.bits(np.full((c['ny'], c['nx']), np.sqrt(np.abs(c['data'][d, y, x])))))
    for p in HV.params('zero_probe'):
        assert not HV.case(*p)['probe'].any()
    for p in HV.params('large_shifts'):
        c = HV.case(*p)
        n = np.array([c['ny'], c['nx']])
        assert (np.abs(c['shifts']).max(0) > n).all() and c['shifts'].shape == (c['nd'], 2)
        if p[2]['kind'] == 'integer':
            assert not c['shifts'][0].any()
            assert HM.rel(c['o64']['target'], HV.rolled_targets(c)) < 1e-12
        else:
            assert (np.abs(c['shifts'] - np.rint(c['shifts'])) > 0.2).any(1).all()


# ------------------------------------------------------------------------------------------------------------ mutations
def _fast(**mut):
    k = VM.parse_constants()
    return lambda x: VM.sincos_fast_mirror(x, k=k, **mut)


def test_the_mirror_restates_the_chain():
    """The unmutated mirror is a float32 evaluation like the oracle's: within the bars wherever it is used below."""
    for p in (('fresnel_phase', (64, 16), dict(rung='max', sigma=1)), ('negative_data', (32, 32), dict(raw='intensity')),
              ('zero_block', (64, 16), dict(raw='intensity', matrices='offset')), ('all_clamped', (32, 32), dict(axes='x'))):
        c = HV.case(*p)
        m = HV.mirror(c, sincos=_fast())
        assert HM.rel(m['pred'], c['o64']['pred']) < HM.BARS['pred'] * THIRD and HM.rel(m['g_aff'], c['o64']['g_aff']) < HM.BARS['gaff'] * THIRD, p


@pytest.mark.parametrize('p', [p for p in HV.params('fresnel_phase') if p[2]['rung'] in ('max', 'max_broadband') and p[2].get('sigma', 1) == 1], ids=all_ids)
def test_mutation_wrong_quadrant_at_large_arguments(p):
    """sincos_fast's cosine with the quadrant test of the sine (no + 1) moves the prediction of the top rung past BARS['pred'];
    the unmutated mirror of sincos_fast does not."""
    c = HV.case(*p)
    good, bad = HV.mirror(c, sincos=_fast()), HV.mirror(c, sincos=_fast(cs_quadrant_plus_one=False))
    e, eb = HM.rel(good['pred'], c['o64']['pred']), HM.rel(bad['pred'], c['o64']['pred'])
    print('%s: mirror %.2e, wrong quadrant %.2e' % (all_ids(p), e, eb))
    assert e < HM.BARS['pred'] * THIRD and eb > HM.BARS['pred']


def test_fewer_cody_waite_terms_are_below_the_arguments_own_rounding():
    """Why no case is asked to see a dropped Cody-Waite term.  The third term is q * 5.4e-15: at PHASE_MAX (q = 1910) 1e-11 rad
    against the argument's own float32 spacing of 2.4e-4 rad -- the mirror with two terms gives the prediction of the mirror with
    three to 1e-9.  With ONE term the reduced argument is off by q * 3.1e-7 = Phi * 2.0e-7 rad, three float32 roundings of Phi:
    measured, the prediction moves from 4.8e-7 to 1.8e-6 of its norm at 3000 rad (bar 5e-6) and from 1.0e-6 to 2.1e-6 on the
    broadband inputs at 300 rad.  An error of the reduction that stays proportional to the argument's rounding cannot be told
    from it by any float32 yardstick; what these cases see is an error that does not -- a wrong quadrant (above), an overflowing
    quotient, a path that loses the argument."""
    k = VM.parse_constants()
    q = HV.PHASE_MAX * float(k['two_over_pi'])
    assert q * abs(float(k['cw'][2])) < 1e-4 * np.spacing(np.float32(100.))
    for p in (('fresnel_phase', (64, 16), dict(rung='max', sigma=1)), ('fresnel_phase', (32, 32), dict(rung='max_broadband', broadband=True))):
        c = HV.case(*p)
        three, two, one = (HV.mirror(c, sincos=_fast(terms=t))['pred'] for t in (3, 2, 1))
        e = [HM.rel(x, c['o64']['pred']) for x in (three, two, one)]
        print('%s: three terms %.2e, two %.2e, one %.2e' % ((all_ids(p),) + tuple(e)))
        assert HM.rel(two, three) < 1e-8
        assert e[0] < e[2] < HM.BARS['pred']


@pytest.mark.parametrize('p', HV.params('negative_data'), ids=all_ids)
def test_mutation_dropped_sign(p):
    """Without sign(samp) in the cotangent the matrix gradient of negative_data is past its bar (3 x the float32 oracle or 2e-3)."""
    c = HV.case(*p)
    o, s = c['o64'], c['o32']
    bar = max(HM.BARS['gaff'], 3 * HM.rel(s['g_aff'], o['g_aff']))
    e, eb = HM.rel(HV.mirror(c)['g_aff'], o['g_aff']), HM.rel(HV.mirror(c, keep_sign=False)['g_aff'], o['g_aff'])
    print('%s: mirror %.2e, without the sign %.2e, bar %.1e' % (all_ids(p), e, eb, bar))
    assert e < bar and eb > bar


@pytest.mark.parametrize('p', [p for p in HV.params('zero_block') if p[2]['raw'] == 'intensity'], ids=all_ids)
def test_mutation_no_guard(p):
    """Without the non-finite guard the exactly zero samples of zero_block under intensity data make the matrix gradient NaN."""
    c = HV.case(*p)
    assert np.isfinite(HV.mirror(c)['g_aff']).all()
    assert not np.isfinite(HV.mirror(c, guard=False)['g_aff']).all()


@pytest.mark.parametrize('p', [p for p in HV.params('all_clamped') if p[2]['axes'] != 'xy'], ids=all_ids)
def test_mutation_swapped_masks(p):
    """With mx and my exchanged the masked row of all_clamped's one-axis cases is not zero (and the other one is) -- at the
    distances whose translation is negative: clamped to pixel 0 the two corners of the interpolation are pixels 0 and 1 and only
    the mask makes the derivative zero; clamped to the last pixel both corners are that pixel.  The table has both."""
    c = HV.case(*p)
    q = 'xy'.index(p[2]['axes'])
    near = c['affine'][:, q, 2] < 0
    assert near.any() and (~near).any()
    good, bad = HV.mirror(c)['g_aff'], HV.mirror(c, swap_masks=True)['g_aff']
    assert not good[:, q].any() and np.abs(good[:, 1 - q]).min() > 0
    assert np.abs(bad[near, q]).min() > 0 and not bad[:, 1 - q].any()


# ------------------------------------------------------------------------------------------------------------ the source
def _body(src, name):
    return VM.function_body(src, r'\b%s\s*\(' % name)


def test_the_source_still_holds_what_the_classes_are_there_for():
    with open(os.path.join(ROOT, 'adorym_amd', 'csrc', 'adm_holo.hip')) as f:
        src = f.read()
    for what, (fn, text, classes) in HV.SOURCE_TIES.items():
        assert text in _body(src, fn), '%s: %r left %s; the classes %s were there for it' % (what, text, fn, classes)
        assert classes and all(c in HV.CASES for c in classes), what
    reached = {c for _, _, classes in HV.SOURCE_TIES.values() for c in classes}
    assert reached == set(HV.CASES), set(HV.CASES) ^ reached
    # every transcendental call of the file is one the table names: a new call site fails here until a class covers it
    code = re.sub(r'//[^\n]*', '', src)
    for call, n in HV.CALL_COUNTS.items():
        assert len(re.findall(r'(?<![\w.])' + re.escape(call), code)) == n, call
        assert sum(call in text for _, text, _ in HV.SOURCE_TIES.values()) == n, call
    assert not re.search(r'(?<![\w.])(sinf|cosf|__sinf|__cosf|__expf|exp2f|exp_fast)\(', code)
    # sincos_fast's stated range (adm_ms_math.h) is the one the unitarity class goes beyond
    with open(os.path.join(ROOT, 'adorym_amd', 'csrc', 'adm_ms_math.h')) as f:
        assert re.search(r'up to \|x\| = 1e5; nothing is claimed beyond', f.read())
    # the GPU module has a test per class
    with open(os.path.join(ROOT, 'tests', 'test_gpu_holo_value_domain.py')) as f:
        text = f.read()
    for cls in HV.CASES:
        assert re.search(r"cases_of\('%s'\)\)\ndef test_%s\(" % (cls, cls), text), cls
