"""The VALUE axis of the multislice kernels (test infrastructure only): objects, shifts and measured data beyond what the shape
matrices feed them (tests/ms_matrix.py, tests/st_matrix.py draw |sigma k1 delta| <= 0.05 rad, shifts within 2.5 px and finite data).

* ``sincos_fast_mirror`` / ``exp_fast_mirror``: float32 NumPy mirrors of sincos_fast and exp_fast (adm_ms_math.h) with an exact
  fmaf; the polynomial and reduction constants are parsed from the header (``parse_constants``), so a changed constant moves
  the mirror.  v_exp_f32 is replaced by the exact 2^t rounded to float32 (and perturbed by +-1 ulp to bound its share).
* ``OBJECT_CLASSES``: the object value classes, as ``obj_fn`` arguments of ms_matrix.oracle_case; ``wave_paths`` recomputes
  from k1 and the generated object which path of modulate<> every wave of every workgroup takes.
* ``large_shifts``: sub-pixel shifts up to beyond the field; ``value_beamstop`` / ``dirty``: the mask (a disc, a whole row, an
  isolated pixel) and the invalid numbers put under it.

Chosen ranges (measured by tests/test_value_domain_coverage.py on the CPU, which recomputes them and fails when a case leaves
no room under its cap: the fp32 oracle's own distance from the fp64 oracle must stay within one third of every cap of
ms_matrix.TUNED / GENERIC):

  PHI_MAX   = 6 turns = 37.7 rad (many_turns).  An fp32 phase of Phi rad carries ~Phi * 6e-8 rad of rounding, which goes straight
              into the prediction.  Worst fraction of the prediction's cap (TUNED: 2e-6) that the fp32 oracle uses up, over the six
              fields: 0.21 at 4 turns, 0.32 at 6 (6.3e-7 at P = 27), 0.36 at 7, 0.39 at 8, 0.49 at 10; loss, object and probe
              gradient stay below 0.1 throughout.  6 is the largest whole number of turns within one third.
  k1 beta   in [0, 30] (absorbing; exp(-30) = 9e-14 of the incident amplitude), 1 % of the voxels in (88, 120] (the transmission is a
              denormal, beyond 104 exactly 0) and 15 % in [-2, 0) (an unconstrained iterate: amplification by up to e^2 per slice).
              The amplifying voxels set the limit -- the few bright paths dominate every norm and carry the rounding of their
              exponents: down to k1 beta = -3 the fp32 oracle uses 0.67 of the prediction's cap and 0.88 of the loss's (P = 8),
              at -2.5 0.33 / 0.44, at -2 0.24 / 0.08 (gradients 0.08 / 0.14).  The upper end does not matter (0.21 ... 0.24 from 15 to 30).
  the fp32 oracle's errors at these values are listed in DESIGN.md section 2 ("the value-domain matrix").
"""
import os
import re

import numpy as np

from tests import ms_matrix as MM

CSRC = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), 'adorym_amd', 'csrc')
K1 = 2. * np.pi * 1.0 / (1240. / MM.ENERGY_EV)            # voxel 1 nm (PSIZE_CM = 1e-7), as the engine and the oracle form it
K1F = np.float32(K1)
F32 = np.float32


# ---------------------------------------------------------------------------------------------------------------- the source
def _read(name):
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


_FLOAT = r'(-?\d+\.\d*(?:e[-+]?\d+)?)f'


def _floats(text):
    return [F32(v) for v in re.findall(_FLOAT, text)]


def parse_constants(src=None):
    """The constants of sincos_fast, exp_fast and modulate<> in the order the source names them (float32, as the compiler rounds
    the literals)."""
    src = _read('adm_ms_math.h') if src is None else src
    sc = _floats(function_body(src, r'void\s+sincos_fast\s*\('))
    ex = _floats(function_body(src, r'float\s+exp_fast\s*\('))
    mo = _floats(function_body(src, r'void\s+modulate\s*\('))
    assert len(sc) == 12 and len(ex) == 3 and len(mo) == 9, (len(sc), len(ex), len(mo))
    return dict(two_over_pi=sc[0], cw=sc[1:4], sin_poly=sc[4:7], cos_poly=sc[7:10], cos_tail=sc[10:12],
                log2e=ex[0], log2e_lo=ex[1], ln2=ex[2],
                threshold=mo[0], mod_sin_poly=mo[1:4], mod_cos_poly=mo[4:7], mod_cos_tail=mo[7:9])


# ---------------------------------------------------------------------------------------------------------------- the mirrors
def fmaf(a, b, c):
    """fl32(a * b + c) with ONE rounding.  The product of two float32 is exact in float64; the sum is rounded to odd in float64
    (two-sum gives its error exactly), which the final rounding to float32 then sees as the exact value would be seen."""
    a, b, c = (np.asarray(v, F32).astype(np.float64) for v in (a, b, c))
    p = a * b
    s = p + c
    bb = s - p
    err = (p - (s - bb)) + (c - bb)
    fix = np.isfinite(s) & (err != 0) & ((np.atleast_1d(s).view(np.int64).reshape(np.shape(s)) & 1) == 0)
    s = np.where(fix, np.nextafter(s, np.where(err > 0, np.inf, -np.inf)), s)
    return s.astype(F32)


def _poly_sincos(r, k):
    r = np.asarray(r, F32)
    r2 = r * r
    sp = fmaf(r2, k['sin_poly'][0], k['sin_poly'][1])
    sp = fmaf(sp, r2, k['sin_poly'][2])
    sp = fmaf(sp * r2, r, r)
    cp = fmaf(r2, k['cos_poly'][0], k['cos_poly'][1])
    cp = fmaf(cp, r2, k['cos_poly'][2])
    cp = fmaf(cp * r2, r2, fmaf(r2, k['cos_tail'][0], k['cos_tail'][1]))
    return sp, cp


def sincos_fast_mirror(x, k=None, terms=3, cs_quadrant_plus_one=True):
    """(sin, cos) as sincos_fast computes them.  ``terms`` / ``cs_quadrant_plus_one``: the mutations of the coverage test (fewer
    Cody-Waite terms, the cosine's quadrant test without its + 1)."""
    k = k or parse_constants()
    x = np.asarray(x, F32)
    q = np.rint(x * k['two_over_pi']).astype(F32)
    r = x
    for c in k['cw'][:terms]:
        r = fmaf(q, c, r)
    iq = q.astype(np.int64)
    sp, cp = _poly_sincos(r, k)
    swap = (iq & 1) != 0
    s0, c0 = np.where(swap, cp, sp), np.where(swap, sp, cp)
    sn = np.where((iq & 2) != 0, -s0, s0)
    cs = np.where(((iq + (1 if cs_quadrant_plus_one else 0)) & 2) != 0, -c0, c0)
    return sn.astype(F32), cs.astype(F32)


def sincos_small_mirror(x, k=None):
    """The small path of modulate<>: the polynomials on the argument itself."""
    return _poly_sincos(x, k or parse_constants())


def exp_fast_mirror(x, k=None, exp2_ulps=0, low_part=True):
    """exp_fast with 2^t evaluated exactly and rounded to float32 (``exp2_ulps``: moved by so many ulps afterwards, the share
    of a 1-ulp hardware instruction); ``low_part`` = False is the mutation without the re-injected low part."""
    k = k or parse_constants()
    x = np.asarray(x, F32)
    t = x * k['log2e']
    e = fmaf(x, k['log2e'], -t)
    e = fmaf(x, k['log2e_lo'], e)
    with np.errstate(under='ignore', over='ignore'):
        r = np.exp2(t.astype(np.float64)).astype(F32)
    for _ in range(abs(exp2_ulps)):
        r = np.nextafter(r, F32(np.inf if exp2_ulps > 0 else 0), dtype=F32)
    if not low_part:
        return r
    return fmaf(r, e * k['ln2'], r)


def ulps(got, ref64):
    """|got - ref| in units of the float32 spacing at |ref|."""
    ref64 = np.asarray(ref64, np.float64)
    with np.errstate(over='ignore'):
        sp = np.spacing(np.abs(ref64).astype(F32)).astype(np.float64)
    return np.abs(np.asarray(got, np.float64) - ref64) / sp


def sincos_inputs():
    """The argument sets of the mirror's measurement: dense over |x| <= 4, the float32 neighbourhoods of every quadrant boundary up
    to 1e5, log-spaced magnitudes to 1e5."""
    dense = np.linspace(-4, 4, 400001).astype(F32)
    kk = np.concatenate([np.arange(-64, 65), np.round(np.geomspace(65, 1e5 * 2 / np.pi - 1, 400)).astype(int),
                         -np.round(np.geomspace(65, 1e5 * 2 / np.pi - 1, 400)).astype(int)])
    b = (kk * (np.pi / 2)).astype(F32)
    boundaries = np.concatenate([b] + [np.nextafter(b, F32(s), dtype=F32) for s in (np.inf, -np.inf)]
                                + [(kk * (np.pi / 2) + d).astype(F32) for d in (1e-6, -1e-6, 1e-3, -1e-3, np.pi / 4, -np.pi / 4)])
    mag = np.geomspace(1e-30, 1e5, 200001)
    log = np.concatenate([mag, -mag]).astype(F32)
    return dict(dense=dense, boundaries=boundaries, log=log)


def sincos_ulps(x, **mut):
    """Error of the mirror against np.sin / np.cos in float64: in float32 ulps of the exact value, and absolute."""
    x = np.asarray(x, F32)
    sn, cs = sincos_fast_mirror(x, **mut)
    x64 = x.astype(np.float64)
    rs, rc = np.sin(x64), np.cos(x64)
    return dict(sin=ulps(sn, rs), cos=ulps(cs, rc), abs=np.maximum(np.abs(sn - rs), np.abs(cs - rc)))


EXP_NORMAL_MIN = -87.3            # exp(x) is a normal float32 above; below, the hardware instruction may flush to 0


def exp_inputs():
    return np.concatenate([np.linspace(-100, 5, 400001), -np.geomspace(1e-30, 100, 20001), np.geomspace(1e-30, 5, 20001)]).astype(F32)


def exp_ulps(x, exp2_ulps=0, **mut):
    """``ulp``: the error where exp(x) is a normal float32, in its ulps; ``sub_abs``: the absolute error below that."""
    x = np.asarray(x, F32)
    got = exp_fast_mirror(x, exp2_ulps=exp2_ulps, **mut).astype(np.float64)
    ref = np.exp(x.astype(np.float64))
    normal = x >= EXP_NORMAL_MIN
    return dict(ulp=ulps(got[normal], ref[normal]), sub_abs=np.abs(got[~normal] - ref[~normal]))


# ---------------------------------------------------------------------------------------------------------------- objects
PHI_MAX_TURNS = 6
PHI_MAX = PHI_MAX_TURNS * 2 * np.pi
K1B_MAX, K1B_UNDERFLOW, K1B_MIN = 30., (88., 120.), -2.
QUADRANT_OFFSETS = (0., 1e-6, -1e-6, 1e-3, -1e-3)
QUADRANT_PHASES = np.array([k * (np.pi / 2) + d for k in range(-9, 10) for d in QUADRANT_OFFSETS])
ONE_LANE_PHASE = 1.2


def phase32(delta, sigma=1):
    """sigma * k1 * delta as the kernels round it (float32 k1, float32 delta); the modulation phase is its negative."""
    return (F32(sigma) * K1F) * np.asarray(delta, F32)


def delta_for_phase(phi, exact=False):
    """float32 delta whose kernel phase fl32(k1 * delta) is nearest the float32 ``phi``; ``exact``: is ``phi`` itself (asserted; near
    pi/4, k1 * ulp(delta) < ulp(phi), so every float32 phase has one)."""
    phi = np.asarray(phi, F32)
    d0 = (phi.astype(np.float64) / np.float64(K1F)).astype(F32)
    cands = [d0]
    for side in (np.inf, -np.inf):
        c = d0
        for _ in range(3):
            c = np.nextafter(c, F32(side), dtype=F32)
            cands.append(c)
    cands = np.stack(cands)
    miss = np.abs((K1F * cands).astype(np.float64) - phi.astype(np.float64))
    best = np.take_along_axis(cands, miss.argmin(0)[None], 0)[0]
    if exact:
        assert ((K1F * best) == phi).all(), 'no float32 delta for some phase'
    return best


def _weak(r, Y, X, S, c=1):
    """ms_matrix's own draw (delta <= 2e-3 c, beta <= 2e-4 c)."""
    return np.stack([2e-3 * c * r.uniform(size=(Y, X, S)), 2e-4 * c * r.uniform(size=(Y, X, S))], -1)


def _f32(a):
    return np.asarray(a, F32).astype(np.float64)


def _finish(obj, pert):
    """The object as float32 holds it (the engine's input and the oracle's are then the same numbers) and a truth for the data:
    the object plus up to 0.25 rad of phase and 0.025 of absorption per voxel, so that the residual is ~10 % of the prediction."""
    obj = _f32(obj)
    return obj, obj + pert


def _signs(r, shape):
    return np.where(r.uniform(size=shape) < 0.5, -1., 1.)


def positions_of(r, B, Y, X, Py, Px):
    """The positions oracle_case will draw AFTER the object function returns (a copy of the generator draws them)."""
    r2 = np.random.default_rng()
    r2.bit_generator.state = r.bit_generator.state
    return MM.edge_positions(r2, B, Y, X, Py, Px)


def wave_rows(P):
    """[start, stop) of the tile rows of every wave of the tuned kernel at size P (Geo<> of adm_ms_math.h: G = max(R1, R2) threads
    per line, 64 / G lines per wave)."""
    src = _read('adm_multislice.hip')
    m = re.search(r'#define\s+ADM_FOR_EACH_SIZE\(X\)(.*)', src)
    sizes = {int(n): (int(r1), int(r2)) for n, r1, r2 in re.findall(r'X\(\s*(\d+)\s*,\s*(\d+)\s*,\s*(\d+)\s*\)', m.group(1))}
    r1, r2 = sizes[P]
    geo = function_body(_read('adm_ms_math.h'), r'struct\s+Geo\s*')
    assert 'G = (R1 > R2) ? R1 : R2' in geo and 'LPW = 64 / G' in geo and 'NWAVES = (N + LPW - 1) / LPW' in geo, 'Geo<> changed'
    lpw = 64 // max(r1, r2)
    return [(lo, min(lo + lpw, P)) for lo in range(0, P, lpw)]


def one_lane_pixels(P):
    """The tile pixels of the one strong voxel: in the first wave and in the last wave of the workgroup (the same wave at P = 8),
    inside the object for every position of edge_positions (which hang over it by at most 3)."""
    rows = wave_rows(P)
    first = min(rows[0][1] - 1, P // 2 - 1)
    last = max(rows[-1][0] + 1, P // 2)
    return (first, 3), (last, P - 4)


def object_fn(cls, P=None, B=None, real_imag=False):
    """``obj_fn`` of ms_matrix.oracle_case for an object class (``P``, ``B``: the case's, for 'one_lane').  ``real_imag``: the
    control -- the same numbers handed to a real_imag plan as the transmission (1 + delta) + i beta, where no transcendental is
    evaluated (vacuum is 1 + 0i there)."""
    def fn(r, Y, X, S):
        w, pert = _weak(r, Y, X, S), _weak(r, Y, X, S, c=5)          # (every draw of 'one_lane' comes before positions_of)
        shape = (Y, X, S)
        if cls == 'weak':
            pass
        elif cls == 'all_general':
            ph = r.uniform(np.pi / 4 + 0.01, 3.0, shape) * _signs(r, shape)
            w[..., 0] = delta_for_phase(ph.astype(F32))
        elif cls == 'many_turns':
            ph = r.uniform(0, PHI_MAX, shape) * _signs(r, shape)
            w[..., 0] = delta_for_phase(ph.astype(F32))
        elif cls == 'quadrants':
            ph = np.resize(QUADRANT_PHASES, Y * X * S).reshape(shape)
            w[..., 0] = delta_for_phase(ph.astype(F32))
        elif cls == 'threshold':
            thr = parse_constants()['threshold']
            below, above = np.nextafter(thr, F32(0), dtype=F32), np.nextafter(thr, F32(1), dtype=F32)
            yy = np.arange(Y)[:, None] + np.arange(X)[None, :]
            for s in range(S):
                if s % 3 == 0:          # the small path at its edge: exactly the threshold and just below it, both signs
                    ph = np.choose(yy % 4, [thr, below, -thr, -below])
                elif s % 3 == 1:        # the general path at its edge
                    ph = np.choose(yy % 2, [above, -above])
                else:                   # both in one workgroup: every sixteenth row just above (a wave holds at most 16 rows)
                    ph = np.where((np.arange(Y) % 16 == 3)[:, None], np.choose(yy % 2, [above, -above]),
                                  np.choose(yy % 4, [thr, below, -thr, -below]))
                w[:, :, s, 0] = delta_for_phase(ph.astype(F32), exact=True)
        elif cls == 'one_lane':
            Py, Px = (P, P) if np.isscalar(P) else P
            pos = positions_of(r, B, Y, X, Py, Px)
            pix = one_lane_pixels(P) if np.isscalar(P) else ((3, 3), (Py - 4, Px - 4))       # (no waves to tell apart off the tuned sizes)
            d = delta_for_phase(F32(ONE_LANE_PHASE))
            for b, (py, px) in enumerate(pos):
                y, x = py + pix[b % 2][0], px + pix[b % 2][1]
                assert 0 <= y < Y and 0 <= x < X, (b, y, x)
                w[y, x, b % S, 0] = d * (1 if b % 4 < 2 else -1)
        elif cls == 'absorbing':
            kb = r.uniform(0, K1B_MAX, shape)
            u = r.uniform(size=shape)
            kb = np.where(u < 0.15, r.uniform(K1B_MIN, 0, shape), kb)
            kb = np.where(u > 0.99, r.uniform(K1B_UNDERFLOW[0] + 0.5, K1B_UNDERFLOW[1], shape), kb)
            w[..., 1] = kb / K1
        elif cls == 'vacuum':
            w[:] = 0
        else:
            raise KeyError(cls)
        if real_imag:
            w[..., 0] += 1
            pert = pert * np.array([10., 100.])          # (a residual of ~10 % here too: up to 0.1 in both parts)
        return _finish(w, pert)
    return fn


def exp_ramp_fn(r, Y, X, S):
    """delta = 0 and k1 beta over [-3, 40], shuffled: with S = 1, an exit-wave detector and a probe of 1 + 0i the prediction IS
    exp_fast(-k1 beta) (cos 0 = 1 and sin 0 = 0 exactly), up to the rounding of |.| = sqrt(e * e)."""
    kb = np.concatenate([np.linspace(-3, 40, Y * X * S - 64), np.linspace(-1e-3, 1e-3, 64)])
    w = np.zeros((Y, X, S, 2))
    w[..., 1] = r.permutation(kb).reshape(Y, X, S) / K1
    w = _f32(w)
    return w, w


# class -> the path of modulate<> its waves take ('small', 'general', 'mixed': both in one workgroup)
OBJECT_CLASSES = {'weak': 'small', 'all_general': 'general', 'one_lane': 'mixed', 'threshold': 'mixed', 'quadrants': 'general',
                  'many_turns': 'general', 'absorbing': 'small', 'vacuum': 'small'}
SIGMA_OF = {'all_general': -1, 'threshold': -1}          # sigma = -1 where the class runs with one sign only (all_general runs both)


def wave_paths(obj, pos, P, sigma=1):
    """[B, S, n_waves] bool: the wave takes the general path of modulate<> (some lane has |sigma k1 delta| > threshold, evaluated
    in float32 as the kernel does); and [B, S, n_waves] bool: the wave sees any voxel of the object at all."""
    thr = parse_constants()['threshold']
    tiles, _ = MM.O.extract_tiles(np.asarray(obj, np.float64), pos, (P, P), 'delta_beta')          # [B, P, P, S, 2], zeros outside
    inside, _ = MM.O.extract_tiles(np.ones_like(obj), pos, (P, P), 'delta_beta')
    big = np.abs(phase32(tiles[..., 0], sigma)) > thr                                               # [B, P, P, S]
    rows = wave_rows(P)
    general = np.stack([big[:, lo:hi].any(axis=(1, 2)) for lo, hi in rows], -1)                     # [B, S, n_waves]
    seen = np.stack([(inside[:, lo:hi, :, :, 0] > 0).any(axis=(1, 2)) for lo, hi in rows], -1)
    return general, seen


# ---------------------------------------------------------------------------------------------------------------- cases
OBJ_KW = dict(S=3, B=6)
TUNED_SIZES = (8, 32, 27)
GENERIC_FIELD = (127, 129)
STREAMED_FIELDS = ((24, 24), (640, 136))
MODES_CLASSES = ('all_general', 'one_lane')             # these also run with three probe modes


def object_case_kw(cls, P, n_modes=1, sigma=None, unknown_type='delta_beta'):
    """oracle_case arguments of an object class at a field."""
    kw = dict(OBJ_KW, n_modes=n_modes, unknown_type=unknown_type, sign_convention=sigma if sigma is not None else SIGMA_OF.get(cls, 1))
    if cls != 'weak' or unknown_type == 'real_imag':              # ('weak' with delta_beta: oracle_case's own draw, today's inputs)
        kw['obj_fn'] = object_fn(cls, P, kw['B'], real_imag=(unknown_type == 'real_imag'))
    return kw


CONTROL_FIELDS = (('tuned', 32), ('tuned', 27), ('generic', GENERIC_FIELD), ('streamed', STREAMED_FIELDS[0]))


def object_cases():
    """(evaluator, P, class, n_modes, sigma) of every run of section A against the oracle."""
    out = []
    for cls in OBJECT_CLASSES:
        sig = [1, -1] if cls == 'all_general' else [SIGMA_OF.get(cls, 1)]
        for P in TUNED_SIZES:
            for s in sig:
                out.append(('tuned', P, cls, 1, s))
            if cls in MODES_CLASSES:
                out.append(('tuned', P, cls, 3, sig[0]))
        out.append(('generic', GENERIC_FIELD, cls, 1, sig[0]))
        for F in STREAMED_FIELDS:
            out.append(('streamed', F, cls, 1, sig[0]))
        if cls in MODES_CLASSES:
            out.append(('generic', GENERIC_FIELD, cls, 3, sig[0]))
            out.append(('streamed', STREAMED_FIELDS[0], cls, 3, sig[0]))
    return out


def bars_of(evaluator):
    return MM.TUNED if evaluator == 'tuned' else MM.GENERIC


def oracle_room(res, bars):
    """The fp32 oracle's own distance from the fp64 oracle, as fractions of the caps: each must stay within one third."""
    out = dict(pred=MM.rel(res['pred_32'], res['pred_o']) / bars['pred'],
               loss=abs(res['loss_32'] - res['loss_o']) / (bars['loss'] * abs(res['loss_o'])),
               grad=MM.rel(res['grad_32'], res['grad_o']) / bars['grad'],
               gprobe=MM.rel(res['gprobe_32'], res['gprobe_o']) / bars['grad'])
    if res.get('shifts') is not None:
        out['gshift'] = MM.rel(res['gshift_32'], res['gshift_o']) / bars['shift']
    return out


# ---------------------------------------------------------------------------------------------------------------- shifts
def large_shifts(P, n_ent):
    """[n_ent, 2] shifts in pixels: +-7.3, +-(P/2 - 0.25), +-(P + 3.6) (beyond the field: it wraps), signs mixed, entry 1 at 0."""
    Py, Px = (P, P) if np.isscalar(P) else P
    base = [(7.3, -7.3), (0., 0.), (-(Py / 2 - 0.25), Px / 2 - 0.25), (Py + 3.6, -(Px + 3.6)), (-7.3, Px + 3.6), (Py / 2 - 0.25, 7.3),
            (-(Py + 3.6), -(Px / 2 - 0.25))]
    return np.array([base[i % len(base)] for i in range(n_ent)], np.float64)


# ---------------------------------------------------------------------------------------------------------------- masks
DIRT = (np.nan, np.inf, -1., 0., 3e38)


def value_beamstop(P):
    """A mask with a disc, one whole row and one isolated pixel dropped (0), everything else kept (1)."""
    Py, Px = (P, P) if np.isscalar(P) else P
    yy, xx = np.meshgrid(np.arange(Py) - Py / 2, np.arange(Px) - Px / 2, indexing='ij')
    bs = np.where(yy ** 2 + xx ** 2 < (min(Py, Px) / 5) ** 2, 0., 1.)
    bs[1, :] = 0
    bs[Py - 1, Px - 1] = 0
    return bs


def dirty(meas, beamstop):
    """``meas_edit`` of oracle_case: the data under the mask replaced by a mix of NaN, +inf, -1, 0 and 3e38."""
    meas = np.array(meas, np.float64)
    drop = np.asarray(beamstop) < 1e-5
    n = int(drop.sum())
    for b in range(len(meas)):
        meas[b][drop] = np.resize(np.roll(DIRT, b), n)
    return meas


MASK_VARIANTS = {
    'lsq_far': dict(),
    'lsq_far_modes': dict(n_modes=3),
    'lsq_exit': dict(free_prop=0),
    'lsq_exit_modes': dict(free_prop=0, n_modes=3),
    'poisson_far': dict(loss='poisson', raw_data_type='intensity', poisson_multiplier=50., seed=1),
    'poisson_far_modes': dict(loss='poisson', raw_data_type='intensity', poisson_multiplier=50., n_modes=3, seed=1),
    'poisson_exit': dict(loss='poisson', raw_data_type='intensity', poisson_multiplier=50., free_prop=0, seed=1),
    'poisson_exit_modes': dict(loss='poisson', raw_data_type='intensity', poisson_multiplier=50., free_prop=0, n_modes=3, seed=1),
}
MASK_FIELDS = (('tuned', 8), ('tuned', 27), ('generic', GENERIC_FIELD), ('streamed', (24, 24)), ('streamed', (640, 136)))
MASK_CASES = [(ev, P, v) for ev, P in MASK_FIELDS for v in MASK_VARIANTS]
# every loss site of the kernels -> the MASK_CASES that run it (checked against the sources by the coverage test)
LOSS_SITES = {'adm_multislice.hip': 4, 'adm_ms_generic.hip': 1, 'adm_ms_streamed.hip': 1}


# ---------------------------------------------------------------------------------------------------------------- the engine
def run(A, ctx, case, evaluator='tuned', cache=None, theta=None, refresh=False, target=None):
    """One minibatch on the engine: rotate -> multislice -> rotate_adjoint.  ``evaluator``: 'tuned', 'generic', 'streamed';
    ``cache``: None (the case's own), 0 (in-loop modulation), 1 (cached transmissions beside the rotated object), 2 (cached
    transmissions only); ``theta``: rotate by this angle (then through a RotationTable, whose adjoint is a deterministic gather)
    instead of the identity; ``refresh``: the rotated object reaches the plan by a plain copy and adm_transmission_refresh;
    ``target``: data in place of the case's.  Returns the case with pred, loss, loss_sum, grad, grad_rot, gprobe added."""
    from adorym_amd._lib import check
    out, k = dict(case), case['kw']
    obj, pos, probes, bs = [case[n] for n in ('obj', 'pos', 'probes', 'beamstop')]
    target = case['target'] if target is None else target
    (Py, Px), S, B, M = k['shape'], k['S'], k['B'], k['n_modes']
    Y, X = obj.shape[:2]
    tc = k['transmission_cache'] if cache is None else bool(cache)
    eng = A.MultisliceEngine(ctx, (Y, X, S), (Py, Px), pos, MM.ENERGY_EV, MM.PSIZE_CM, free_prop_cm=k['free_prop'], binning=k['binning'],
                             fresnel_approx=k['fresnel_approx'], sign_convention=k['sign_convention'], normalize_fft=k['normalize_fft'],
                             n_probe_modes=M, max_batch=B, loss_function_type=k['loss'], poisson_multiplier=k['poisson_multiplier'],
                             unknown_type=k['unknown_type'], beamstop=bs, transmission_cache=tc, transmissions_only=(cache == 2),
                             generic=(evaluator == 'generic'), streamed=(evaluator == 'streamed'))
    assert eng.streamed == (evaluator == 'streamed')
    if cache is not None and k['unknown_type'] == 'delta_beta' and k['binning'] == 1:
        assert eng.transmission_cache == bool(cache) and eng.transmissions_only == (cache == 2)
    tab = A.RotationTable(ctx, (Y, X, S), np.float32(theta)) if theta is not None else None
    coords = tab.coords if tab is not None else None
    d_obj = ctx.array(obj, np.float32)
    eng.set_batch(pos, target)
    if refresh:
        assert cache == 1
        plain = A.MultisliceEngine(ctx, (Y, X, S), (Py, Px), pos, MM.ENERGY_EV, MM.PSIZE_CM, max_batch=B, transmission_cache=False)
        plain.rotate(d_obj, coords)
        rotated = plain.obj_rot.get()
        plain.plan.close()
        eng.rotate(ctx.array(_weak(np.random.default_rng(1), Y, X, S), np.float32), coords)      # the cache holds another object first
        eng.obj_rot.set(rotated)
        check(ctx.lib.adm_transmission_refresh(eng.plan.handle, eng.obj_rot.ptr, 0, Y))
    else:
        eng.rotate(d_obj, coords)
    d_grad, d_probe, d_gp = ctx.zeros(obj.shape), ctx.array(MM.c2(probes)), ctx.zeros((M, Py, Px, 2))
    eng.multislice(d_probe, grad_probe=d_gp, want_pred=True)
    eng.rotate_adjoint(d_grad, tab)
    out['pred'] = eng.pred()
    out['loss'] = eng.loss()
    out['loss_sum'] = eng._loss.view(0, (B,)).get().copy()
    out['grad'] = d_grad.get()
    out['grad_rot'] = eng.grad_rot.get()
    out['gprobe'] = MM.cplx(d_gp.get())
    out['gprobe_raw'] = d_gp.get()
    eng.plan.close()
    return out


BIT_KEYS = ('pred', 'loss_sum', 'grad_rot', 'grad', 'gprobe_raw')


def bits_differ(a, b, keys=BIT_KEYS, where=None):
    """Words that differ between two runs, per result (``where``: [Py, Px] bool, the detector pixels of pred to compare)."""
    out = {}
    for n in keys:
        x, y = np.ascontiguousarray(a[n], np.float32), np.ascontiguousarray(b[n], np.float32)
        if n == 'pred' and where is not None:
            x, y = np.ascontiguousarray(x[:, where]), np.ascontiguousarray(y[:, where])
        out[n] = int((x.view(np.uint32) != y.view(np.uint32)).sum())
    return out


def all_finite(res, keys=BIT_KEYS, where=None):
    return {n: bool(np.isfinite(res[n] if not (n == 'pred' and where is not None) else res[n][:, where]).all()) for n in keys}
