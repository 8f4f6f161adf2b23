"""The value-domain tables (tests/value_matrix.py) against the kernel sources and the oracle, on the CPU:

* the float32 mirrors of sincos_fast / exp_fast, built from the constants parsed out of adm_ms_math.h, hold the accuracy the
  source comments state, and the small path of modulate<> gives the general path's bits wherever it is taken;
* every object class reaches the path of modulate<> it claims, recomputed from k1 and the generated object;
* every case leaves room under its cap: the fp32 oracle's own distance from the fp64 oracle stays within one third of it;
* the mask, the dirt under it and the large shifts are what tests/test_gpu_value_domain.py says they are, and the oracle itself
  never reads a dropped pixel.
"""
import hashlib
import re

import numpy as np
import pytest

from tests import ms_matrix as MM
from tests import value_matrix as VM

F32 = np.float32


# ------------------------------------------------------------------------------------------------------------ B. the mirrors
def test_fmaf_rounds_once():
    """The mirror's fmaf against exact rational arithmetic on products that a double-rounded a * b + c gets wrong."""
    from fractions import Fraction
    r = np.random.default_rng(0)
    a = r.standard_normal(4000).astype(F32)
    b = r.standard_normal(4000).astype(F32)
    c = (-(a.astype(np.float64) * b.astype(np.float64)) * (1 + r.uniform(-1e-6, 1e-6, 4000))).astype(F32)      # heavy cancellation
    c[::2] = r.standard_normal(2000).astype(F32)
    got = VM.fmaf(a, b, c)
    for i in range(len(a)):
        exact = Fraction(float(a[i])) * Fraction(float(b[i])) + Fraction(float(c[i]))
        lo, hi = np.nextafter(got[i], F32(-np.inf)), np.nextafter(got[i], F32(np.inf))
        d = abs(Fraction(float(got[i])) - exact)
        assert d <= abs(Fraction(float(lo)) - exact) and d <= abs(Fraction(float(hi)) - exact), (i, a[i], b[i], c[i], got[i])


def test_constants_are_parsed_from_the_header():
    k = VM.parse_constants()
    assert k['two_over_pi'] == F32(2 / np.pi) and k['log2e'] == F32(np.log2(np.e)) and k['ln2'] == F32(np.log(2))
    assert abs(float(sum(np.float64(c) for c in k['cw'])) + np.pi / 2) < 1e-20 + 1e-15
    assert abs(np.float64(k['log2e']) + np.float64(k['log2e_lo']) - np.log2(np.e)) < 1e-15
    # modulate<>'s small path restates the polynomials: the same constants, or the bits differ
    assert list(k['mod_sin_poly']) == list(k['sin_poly']) and list(k['mod_cos_poly']) == list(k['cos_poly'])
    assert list(k['mod_cos_tail']) == list(k['cos_tail'])
    assert k['threshold'] == F32(0.78539816) and k['threshold'] <= F32(np.pi / 4)
    # a changed constant moves the mirror
    src = VM._read('adm_ms_math.h').replace('8.3321608736e-3f', '8.3321608737e-2f')
    assert VM.parse_constants(src)['sin_poly'][1] != k['sin_poly'][1]
    # the any-size kernels' modulator and the rotation's are the same two calls with the same signs
    gen = VM.function_body(VM._read('adm_ms_gen.h'), r'cf\s+gen_modulator\s*\(')
    one = VM.function_body(VM._read('adm_ms_math.h'), r'float2\s+slice_transmission\s*\(')
    for body in (gen, one):
        assert 'sincos_fast(-sigma * k1 * db.x, sn, cs)' in body and 'exp_fast(-k1 * db.y)' in body, body
        assert 'make_float2(e * cs, e * sn)' in body, body


def test_sincos_mirror_accuracy():
    """The comment of sincos_fast: at most 1.55 ulp / 9.3e-8 on these sets (measured: dense 1.49 / 1.54 ulp (sin / cos), boundaries
    1.39 / 1.55, log-spaced to 1e5 1.45 / 1.48).  The mirror performs the kernel's own operations, so the bar is the measured
    figure rounded up, 1.6 ulp."""
    k = VM.parse_constants()
    for name, x in VM.sincos_inputs().items():
        u = VM.sincos_ulps(x, k=k)
        print('%s: %d arguments, sin %.3f ulp, cos %.3f ulp, absolute %.3e' % (name, x.size, u['sin'].max(), u['cos'].max(), u['abs'].max()))
        assert u['sin'].max() <= 1.6 and u['cos'].max() <= 1.6 and u['abs'].max() <= 1e-7, name


def test_exp_mirror_accuracy():
    """The comment of exp_fast: below 1.0 ulp around an exactly rounded 2^t (measured 0.9991), below 2.0 with 2^t one ulp off either
    way (measured 1.9982 / 1.9991): the one-ulp margin covers the mirror's substitution for v_exp_f32.  Where exp(x) is no normal
    float32 the result is within one denormal step of it -- or 0, should the instruction flush."""
    k = VM.parse_constants()
    x = VM.exp_inputs()
    for d, bar in ((0, 1.0), (1, 2.0), (-1, 2.0)):
        u = VM.exp_ulps(x, d, k=k)
        print('exp, 2^t moved by %+d ulp: %.4f ulp; below the normal range %.2e absolute' % (d, u['ulp'].max(), u['sub_abs'].max()))
        assert u['ulp'].max() <= bar, d
        assert u['sub_abs'].max() <= 2.0 ** -148, d
    got = VM.exp_fast_mirror(x, k=k)
    assert np.isfinite(got).all() and (got >= 0).all()


def test_small_path_gives_the_general_paths_bits():
    """modulate<>'s promise, on the mirror: wherever the small path may run (|phi| <= threshold) the general path reduces by q = 0
    and both give the same bits; one float32 beyond the threshold the reduction is no longer the identity."""
    k = VM.parse_constants()
    thr = k['threshold']
    x = np.concatenate([np.linspace(-thr, thr, 200001).astype(F32), [thr, -thr, np.nextafter(thr, F32(0)), F32(0), F32(1e-30), F32(-1e-30)]]).astype(F32)
    assert (np.abs(x) <= thr).all()
    sg, cg = VM.sincos_fast_mirror(x, k=k)
    ss, cs = VM.sincos_small_mirror(x, k=k)
    assert np.array_equal(sg.view(np.uint32), ss.view(np.uint32)) and np.array_equal(cg.view(np.uint32), cs.view(np.uint32))
    above = np.nextafter(thr, F32(1), dtype=F32)
    assert np.rint(above * k['two_over_pi']) == 1 and np.rint(thr * k['two_over_pi']) == 0


@pytest.mark.parametrize('mutation', ['two_cody_waite_terms', 'cs_quadrant_without_plus_one', 'exp_without_low_part'])
def test_the_accuracy_bars_bite(mutation):
    """Each mutation of the issue's list that changes the functions themselves moves the mirror beyond the bars above."""
    k = VM.parse_constants()
    if mutation == 'two_cody_waite_terms':
        # the third term is 5.4e-15 * q: it shows where the reduced argument is small, next to the boundaries
        u = VM.sincos_ulps(VM.sincos_inputs()['boundaries'], k=k, terms=2)
        assert max(u['sin'].max(), u['cos'].max()) > 1.6
    elif mutation == 'cs_quadrant_without_plus_one':
        u = VM.sincos_ulps(VM.sincos_inputs()['dense'], k=k, cs_quadrant_plus_one=False)
        assert u['abs'].max() > 1
    else:
        x = VM.exp_inputs()
        got = VM.exp_fast_mirror(x, k=k, low_part=False).astype(np.float64)
        n = x >= VM.EXP_NORMAL_MIN
        assert VM.ulps(got[n], np.exp(x[n].astype(np.float64))).max() > 2.0


# ------------------------------------------------------------------------------------------------------------ A. the objects
def _case(cls, P, M=1, sigma=None, **kw):
    with np.errstate(all='ignore'):
        return MM.oracle_case(P, **dict(VM.object_case_kw(cls, P, M, sigma), **kw))


_CASES = {}


def _object_case(ev, P, cls, M, sg):
    key = (P, cls, M, sg)
    if key not in _CASES:
        _CASES[key] = _case(cls, P, M, sg)
    return _CASES[key]


@pytest.mark.parametrize('cls', list(VM.OBJECT_CLASSES))
@pytest.mark.parametrize('P', VM.TUNED_SIZES)
def test_every_class_reaches_its_path(P, cls):
    """Which path of modulate<> every wave of every workgroup takes, recomputed from k1 and the object as float32 holds it."""
    sg = VM.SIGMA_OF.get(cls, 1)
    c = _object_case('tuned', P, cls, 1, sg)
    obj = c['obj'].astype(F32)
    general, seen = VM.wave_paths(obj, c['pos'], P, sg)
    ph = np.abs(VM.phase32(obj[..., 0], sg))
    thr = VM.parse_constants()['threshold']
    n_waves = general.shape[-1]
    claim = VM.OBJECT_CLASSES[cls]
    print(cls, P, claim, 'waves per workgroup', n_waves, 'general %d of %d' % (general.sum(), general.size), 'max phase %.4f' % ph.max())
    if claim == 'small':
        assert not general.any() and ph.max() <= thr
    elif claim == 'general':
        assert (general | ~seen).all() and general.any()                   # every wave that sees a voxel of the object
        if cls == 'all_general':
            assert ph.min() > thr and ph.max() <= 3.0
            assert (obj[..., 0] > 0).any() and (obj[..., 0] < 0).any()
        if cls == 'many_turns':
            assert 0.97 * VM.PHI_MAX < ph.max() <= VM.PHI_MAX * (1 + 1e-6)
        if cls == 'quadrants':
            got = np.unique(np.rint(VM.phase32(obj[..., 0], sg).astype(np.float64) / (np.pi / 2)).astype(int))
            assert list(got) == list(range(-9, 10))
    elif cls == 'one_lane':
        assert general.any(axis=(1, 2)).all()                               # every workgroup has a wave on the general path
        assert (ph > thr).sum() <= len(c['pos']) and abs(ph.max() - VM.ONE_LANE_PHASE) < 1e-6
        if n_waves > 1:
            assert (~general).any(axis=2)[general.any(axis=2)].all()        # ... beside waves on the small path, in the same step
            assert general[..., 0].any() and general[..., -1].any()         # the first and the last wave of a workgroup
            assert (general.sum(axis=2) <= 2).all()
    else:
        assert cls == 'threshold'
        below = np.nextafter(thr, F32(0), dtype=F32)
        above = np.nextafter(thr, F32(1), dtype=F32)
        for s, want in ((0, {thr, below}), (1, {above})):
            assert set(np.unique(ph[:, :, s])) == want, (s, np.unique(ph[:, :, s]))
        assert set(np.unique(ph[:, :, 2])) == {thr, below, above}
        assert not general[:, 0].any() and (general[:, 1] | ~seen[:, 1]).all()
        if n_waves > 1:
            mixed = general[:, 2].any(axis=1) & (~general[:, 2] & seen[:, 2]).any(axis=1)
            assert mixed.any()                                               # both paths in one workgroup and step


def test_absorbing_class_spans_its_range():
    c = _object_case('tuned', 32, 'absorbing', 1, 1)
    kb = VM.K1F * c['obj'][..., 1].astype(F32)
    assert kb.min() < 0.9 * VM.K1B_MIN and kb.min() >= VM.K1B_MIN * (1 + 1e-6)
    assert ((kb > 0.9 * VM.K1B_MAX) & (kb <= VM.K1B_MAX)).any()
    under = kb > VM.K1B_UNDERFLOW[0]
    assert 0 < under.sum() < 0.02 * kb.size and kb.max() <= VM.K1B_UNDERFLOW[1]
    t = VM.exp_fast_mirror(-kb[under])
    assert (t < F32(1.17549435e-38)).all() and (t == 0).any() and (t > 0).any()        # denormal, and exactly 0 beyond k1 beta = 104
    v = _object_case('tuned', 32, 'vacuum', 1, 1)
    assert not v['obj'].any()


@pytest.mark.parametrize('ev,P,cls,M,sg', VM.object_cases(), ids=lambda v: str(v).replace(' ', ''))
def test_every_object_case_leaves_room_under_its_cap(ev, P, cls, M, sg):
    """The fp32 oracle's own distance from the fp64 oracle is within one third of every cap (an fp32 phase of Phi rad carries
    Phi * 6e-8 rad of rounding): the 3x rule and the cap then cannot contradict each other.  PHI_MAX and the beta range of
    'absorbing' are the largest that pass here (tests/value_matrix.py)."""
    c = _object_case(ev, P, cls, M, sg)
    room = VM.oracle_room(c, VM.bars_of(ev))
    print(ev, P, cls, M, sg, ' '.join('%s %.3f' % kv for kv in room.items()))
    for k in ('pred_o', 'pred_32', 'grad_o', 'grad_32', 'gprobe_o', 'gprobe_32'):
        assert np.isfinite(c[k]).all(), k
    assert max(room.values()) <= 1 / 3., room


@pytest.mark.parametrize('cls', list(VM.OBJECT_CLASSES))
def test_every_control_case_leaves_room_under_its_cap(cls):
    """The real_imag control of every class, at every field it runs."""
    for ev, P in VM.CONTROL_FIELDS:
        with np.errstate(all='ignore'):
            c = MM.oracle_case(P, **VM.object_case_kw(cls, P, 1, 1, 'real_imag'))
        room = VM.oracle_room(c, VM.bars_of(ev))
        print(ev, P, cls, ' '.join('%s %.3f' % kv for kv in room.items()))
        assert max(room.values()) <= 1 / 3., (ev, P, room)


# ------------------------------------------------------------------------------------------------------------ C. the shifts
@pytest.mark.parametrize('P', [8, 32, (24, 20), (640, 12), (640, 136)], ids=str)
def test_large_shifts_hold_what_the_issue_lists(P):
    Py, Px = (P, P) if np.isscalar(P) else P
    s = VM.large_shifts(P, 6)
    assert (s[1] == 0).all()
    for ax, N in ((0, Py), (1, Px)):
        mags = set(np.round(np.abs(s[:, ax]), 6))
        assert {7.3, round(N / 2 - 0.25, 6), round(N + 3.6, 6)} <= mags, (ax, mags)
        assert (s[:, ax] > 0).any() and (s[:, ax] < 0).any()
        assert np.abs(s[:, ax]).max() > N                                    # beyond the field: it wraps
    assert np.pi * max(Py, Px) > 16                                          # the fp32 argument leaves what the other tests reach


@pytest.mark.parametrize('P', [8, 32])
def test_large_shift_cases_leave_room_under_their_caps(P):
    for M in (1, 3):
        c = MM.oracle_case(P, S=3, B=10, n_modes=M, pp='shifts', shifts_fn=lambda n: VM.large_shifts(P, n))
        room = VM.oracle_room(c, MM.TUNED)
        print(P, M, ' '.join('%s %.3f' % kv for kv in room.items()))
        assert max(room.values()) <= 1 / 3., room


# ------------------------------------------------------------------------------------------------------------ D. the mask
def test_mask_and_dirt():
    for P in (8, 27, (127, 129), (24, 24), (640, 136)):
        Py, Px = (P, P) if np.isscalar(P) else P
        bs = VM.value_beamstop(P)
        drop = bs < 1e-5
        assert drop[1].all()                                                 # one whole row
        assert drop[Py // 2, Px // 2] and drop[Py // 2, Px // 2 - 1]         # a disc
        y, x = Py - 1, Px - 1
        assert drop[y, x] and drop[y - 1:, x - 1:].sum() == 1                # one isolated pixel
        assert 0 < drop.sum() < 0.5 * drop.size
        meas = np.arange(3 * Py * Px, dtype=np.float64).reshape(3, Py, Px) + 1
        d = VM.dirty(meas, bs)
        assert np.array_equal(d[:, ~drop], meas[:, ~drop])
        under = d[:, drop]
        assert np.isnan(under).any() and np.isposinf(under).any() and (under == -1).any() and (under == 0).any() and (under == 3e38).any()
        assert np.isnan(d[:, 1, :]).any() and not np.isfinite(d[:, y, x]).all()


@pytest.mark.parametrize('variant', list(VM.MASK_VARIANTS))
def test_the_oracle_drops_masked_pixels(variant):
    """The yardstick itself: with NaN, inf, -1, 0 and 3e38 under the mask the oracle's loss, gradients and prediction are the
    clean run's bit for bit, in fp64 and in fp32."""
    kw = dict(VM.OBJ_KW, beamstop=VM.value_beamstop(8), **VM.MASK_VARIANTS[variant])
    clean = MM.oracle_case(8, **kw)
    with np.errstate(all='ignore'):
        dirt = MM.oracle_case(8, meas_edit=VM.dirty, **kw)
    assert not np.isfinite(dirt['target']).all()
    for k in ('loss_o', 'loss_32', 'pred_o', 'grad_o', 'grad_32', 'gprobe_o', 'gprobe_32'):
        assert np.isfinite(clean[k]).all() and np.array_equal(np.asarray(clean[k]), np.asarray(dirt[k])), k


@pytest.mark.parametrize('ev,P', VM.MASK_FIELDS, ids=str)
def test_every_mask_case_leaves_room_under_its_cap(ev, P):
    for v, kw in VM.MASK_VARIANTS.items():
        c = MM.oracle_case(P, beamstop=VM.value_beamstop(P), **dict(VM.OBJ_KW, **kw))
        room = VM.oracle_room(c, VM.bars_of(ev))
        print(ev, P, v, ' '.join('%s %.3f' % kv for kv in room.items()))
        assert max(room.values()) <= 1 / 3., (v, room)


def test_every_loss_site_selects():
    """A dropped pixel contributes 0.f to the sum and 0.f to the gradient factor whatever loss_term returned: no loss site of
    the three kernels multiplies a weight into either (0 * NaN = NaN)."""
    for name, sites in VM.LOSS_SITES.items():
        src = VM._read(name)
        calls = re.findall(r'loss_term(?:_nz)?\(', src)
        assert len(re.findall(r'lsum \+= drop \? 0\.f : term;', src)) == sites, name
        assert len(re.findall(r'const bool drop = p\.det_weight && p\.det_weight\[[^\]]+\] == 0\.f;', src)) == sites, name
        assert sites <= len(calls) <= 2 * sites, (name, len(calls))
        assert not re.search(r'lsum \+= \w+ \* ', src) and 'wq' not in src, name
    evs = {(ev, v) for ev, _, v in VM.MASK_CASES}
    for ev in ('tuned', 'generic', 'streamed'):
        for v in VM.MASK_VARIANTS:                                          # far / exit wave x one / three modes x both losses
            assert (ev, v) in evs
    kinds = {(kw.get('free_prop', 'inf'), kw.get('n_modes', 1), kw.get('loss', 'lsq')) for kw in VM.MASK_VARIANTS.values()}
    assert kinds == {(f, m, l) for f in ('inf', 0) for m in (1, 3) for l in ('lsq', 'poisson')}


# ------------------------------------------------------------------------------------------------------------ the builder
def test_oracle_case_defaults_draw_what_they_drew():
    """obj_fn / meas_edit / shifts_fn left out: the inputs of a case are the bytes they were before the arguments existed
    (digests of the generator's draws, taken on the commit before)."""
    want = {12: '96159040100e362129553ef4c3985cd2b1e0022f2e1d99c3c1bb9dbab2d201a8',
            16: 'b6ad44def974430c8d7719493136ef4340dfbe9dd3a63b3ca894c191e66e7a4a'}
    for P, kw in ((12, dict(S=3, B=6)), (16, dict(S=3, B=6, pp='shifts', n_modes=3, beamstop=True, unknown_type='real_imag'))):
        c = MM.oracle_case(P, **kw)
        h = hashlib.sha256()
        for k in ('obj', 'pos', 'probes', 'shifts', 'idx', 'beamstop'):
            if c[k] is not None:
                h.update(np.ascontiguousarray(c[k]).tobytes())
        assert h.hexdigest() == want[P], P
