"""The VALUE axis of the holography kernels (adm_holo.hip through HolographyEngine; test infrastructure only, importable without a
GPU).  tests/holo_matrix.py covers every instantiation on one narrow set of numbers: Fresnel phases within 10 rad, delta/beta
phases within 0.2 rad and 3 % absorption, smooth positive data, matrices within 1 % of the identity, shifts within 1.5 px.  The
classes here are edits of ``holo_matrix.inputs`` run through ``holo_matrix.oracle_run`` in fp64 and float32; they share the
matrix's case cache and its BARS.  tests/test_holo_value_coverage.py decides on the CPU what the oracle pair alone decides and
ties the table to the kernel source; tests/test_gpu_holo_value_domain.py launches every case.

Fields: (64, 16) x 3 distances and (32, 32) x 5 (the two small fields of the matrix whose K3 blocks span distances), and
(16, 64) x 3 for the Fresnel phase only (there the long axis is the row stage).  u^2 + v^2 at Nyquist does not depend on the
field's size, so larger fields add nothing to this axis.

Chosen ranges.  The rule is value_matrix.py's: the float32 oracle's own distance from the fp64 oracle stays within ONE THIRD of
every bar (pred, loss, grad, gdists, gaff); the coverage test recomputes every figure and fails when a case leaves no room.

  PHASE_MAX = 3000 rad: the largest |arg| of holo_h = |c1 * (dist_cm * 1e7f) * uv2|, reached by scaling the distances.  An fp32
              argument of Phi rad carries Phi * 6e-8 rad of rounding whatever evaluates its sine.  Largest fraction of a bar the
              float32 oracle uses up, over the three fields and both sigma, on the ladder 100 / 300 / 1000 / 3000 / 10 000 rad
              (the coverage test recomputes them and PHASE_MAX, the largest rung at and below which every fraction is <= 1/3):
                  pred    0.015 / 0.023 / 0.054 / 0.121 / 0.572
                  loss    0.003 / 0.003 / 0.005 / 0.011 / 0.079
                  grad    0.003 / 0.006 / 0.012 / 0.031 / 0.166
                  gdists  0.001 / 0.002 / 0.005 / 0.032 / 0.110
                  gaff    0.001 / 0.001 / 0.003 / 0.004 / 0.021
              The matrix's inputs are smooth: little of the exit wave lies where the phase is large (an error of 6e-4 rad at the
              top of the spectrum moves the prediction by 1.8e-6).  So the class runs on object and data of uncorrelated noise too
              (holo_matrix.inputs(broadband=True)), where the same rule gives PHASE_MAX_BROADBAND = 300 rad:
                  pred    0.042 / 0.215 / 0.623 / 1.338 / 7.557
                  loss    0.009 / 0.013 / 0.008 / 0.026 / 0.115
                  grad    0.010 / 0.030 / 0.074 / 0.174 / 1.007
                  gdists  0.002 / 0.030 / 0.075 / 0.675 / 0.452
                  gaff    0.002 / 0.002 / 0.002 / 0.003 / 0.015
  unitarity   |arg| to 3e5 rad, beyond what sincos_fast claims (1e5): no reference is a yardstick there.  Judged: every output
              finite, and sum pred_d^2 / sum |probe c|^2 - 1 (H is unimodular; Parseval) within 3 x the float32 oracle's own
              figure on the same inputs + BARS['loss'].
  delta/beta  phases to value_matrix.PHI_MAX (6 turns), k1 beta in [0, 30] with 1 % of the voxels (at least four) in (88, 120]
              (the transmission a denormal, beyond 104 exactly 0), 15 % of the voxels in [-2, 0): value_matrix.py's ranges, whose
              reasoning carries over -- the amplifying voxels dominate every norm and carry the rounding of their exponents.
  the figures of every class are in DESIGN.md section 2 ("the holography value-domain matrix").
"""
import numpy as np
import scipy.fft as sfft

from oracle import adorym_oracle as O
from tests import holo_matrix as HM
from tests import value_matrix as VM
from tests.golden import cases

F32 = np.float32
BARS = HM.BARS
FIELDS = {(64, 16): 3, (32, 32): 5}
PHASE_FIELDS = {(64, 16): 3, (32, 32): 5, (16, 64): 3}
LAMBDA_NM = 1240. / HM.ENERGY_EV
K1 = float(HM.k1_of())

LADDER = (100., 300., 1000., 3000., 10000.)
PHASE_MAX = 3000.                   # the smooth inputs of the matrix
PHASE_MAX_BROADBAND = 300.          # object and data of uncorrelated noise (holo_matrix.inputs(broadband=True))
RUNGS = {'100': 100., '1000': 1000., 'max': PHASE_MAX, 'max_broadband': PHASE_MAX_BROADBAND}
UNITARITY_ARG = 3e5                 # beyond sincos_fast's 1e5
SINCOS_CLAIM = 1e5
PHI_MAX = VM.PHI_MAX                # delta/beta: six turns
K1B_MAX, K1B_UNDERFLOW, K1B_MIN = VM.K1B_MAX, VM.K1B_UNDERFLOW, VM.K1B_MIN
AMPLIFYING_SHARE = 0.15
BLOCK = 7                           # zero_block: BLOCK x BLOCK exact zeros per distance
NEGATED_SHARE = 0.1
CLAMP_TRANSLATION = 3.              # one and a half field widths in normalised coordinates


# ------------------------------------------------------------------------------------------------------------ inputs
def uv2_of(ny, nx, dtype=np.float64):
    u, v = O.gen_freq_mesh(np.array([HM.PSIZE_CM * 1e7] * 3), [ny, nx])
    return (u ** 2 + v ** 2).astype(dtype)


def max_arg(c):
    """The largest |arg| holo_h forms for the case: PI lambda d_nm (u^2 + v^2) at Nyquist of both axes and the largest distance."""
    return float(O.PI * LAMBDA_NM * np.abs(c['dists'].astype(np.float64)).max() * 1e7 * uv2_of(c['ny'], c['nx']).max())


def _scale_dists(c, rad):
    c['dists'] = (c['dists'].astype(np.float64) * (rad / max_arg(c))).astype(F32)
    return c


def fresnel_phase(ny, nx, nd, rung='max', sigma=1, broadband=False):
    return _scale_dists(HM.inputs(ny, nx, nd, sigma=sigma, broadband=broadband), RUNGS[rung])


def unitarity(ny, nx, nd, sigma=1):
    return _scale_dists(HM.inputs(ny, nx, nd, sigma=sigma), UNITARITY_ARG)


def _rng(ny, nx, nd, k):
    return cases.rng(9100 + 31 * ny + 7 * nx + nd + 1000 * k)


def _pick(r, n, share, least=0):
    """``share`` of n indices (at least ``least``), drawn without replacement."""
    return r.choice(n, max(int(round(share * n)), least), replace=False)


def delta_beta(ny, nx, nd, kind='turns', sigma=1):
    """delta/beta objects of uncorrelated voxels: 'turns' (phases over +-PHI_MAX, the matrix's weak absorption), 'absorbing'
    (k1 beta over [0, K1B_MAX], 1 % -- at least four voxels -- in K1B_UNDERFLOW), 'amplifying' (15 % of the voxels in [K1B_MIN, 0))."""
    c = HM.inputs(ny, nx, nd, unknown_type='delta_beta', sigma=sigma)
    r = _rng(ny, nx, nd, 1)
    obj = c['obj'].astype(np.float64).reshape(ny * nx, 2)
    if kind == 'turns':
        obj[:, 0] = r.uniform(-PHI_MAX, PHI_MAX, ny * nx) / K1
    elif kind == 'absorbing':
        obj[:, 1] = r.uniform(0, K1B_MAX, ny * nx) / K1
        deep = _pick(r, ny * nx, 0.01, least=4)
        obj[deep, 1] = r.uniform(K1B_UNDERFLOW[0] + 0.5, K1B_UNDERFLOW[1], len(deep)) / K1
    elif kind == 'amplifying':
        amp = _pick(r, ny * nx, AMPLIFYING_SHARE)
        obj[amp, 1] = r.uniform(K1B_MIN, 0, len(amp)) / K1
    else:
        raise KeyError(kind)
    c['obj'] = obj.reshape(ny, nx, 1, 2).astype(F32)
    return c


def k1_phase(c):
    """(k1 delta, k1 beta) as float64 of the float32 object."""
    o = c['obj'].astype(np.float64)
    return K1 * o[..., 0], K1 * o[..., 1]


def block_of(ny, nx, d):
    y0, x0 = (3 + 5 * d) % (ny - BLOCK), (2 + 3 * d) % (nx - BLOCK)
    return slice(y0, y0 + BLOCK), slice(x0, x0 + BLOCK)


def _offset_matrices(ny, nx, nd, r, rows=(0, 1)):
    """identity + a translation of (0.25, 0.15) px (the sign alternates with the distance) + 0.1 % jitter on ``rows``: every sample
    mixes four pixels with weights near (0.64, 0.21, 0.11, 0.04), well away from the pixel centres, where the last bit of a
    coordinate decides which one-sided derivative of the interpolation the matrix gradient sees."""
    aff = np.tile(np.array([[1., 0, 0], [0, 1., 0]]), [nd, 1, 1])
    jit = 0.001 * r.uniform(-1, 1, (nd, 2, 3))
    sg = np.where(np.arange(nd) % 2 == 0, 1., -1.)
    if 0 in rows:
        aff[:, 0] += jit[:, 0]
        aff[:, 0, 2] = sg * 2 * 0.25 / nx
    if 1 in rows:
        aff[:, 1] += jit[:, 1]
        aff[:, 1, 2] = -sg * 2 * 0.15 / ny
    return aff


def zero_block(ny, nx, nd, raw='intensity', matrices='identity'):
    """A BLOCK x BLOCK block of exact zeros in the data of every distance; ``plain_data``: the data before the edit.
    'identity': identity matrices, uploaded -- the samples sit on pixel centres (to an ulp of the coordinate: the inner 6 x 6 samples
    of the block at least are exact zeros in any precision).
    'offset': the matrices of _offset_matrices -- the samples whose four corners lie in the block (at least 5 x 5 per distance) are
    exact zeros, the others at least 0.12 of a pixel's value."""
    c = HM.inputs(ny, nx, nd, raw=raw, affine='none')
    c['has_affine'] = True
    if matrices == 'offset':
        c['affine'] = _offset_matrices(ny, nx, nd, _rng(ny, nx, nd, 3)).astype(F32)
    c['plain_data'] = c['data'].copy()
    for d in range(nd):
        c['data'][(d,) + block_of(ny, nx, d)] = 0
    return c


def negative_data(ny, nx, nd, raw='intensity'):
    """A tenth of the pixels negated under the matrices of _offset_matrices: a sample next to a negated pixel straddles the sign
    change, and none comes nearer to zero than 0.12 of a pixel's value (wx <= 0.3, wy <= 0.2: 0.56 - 0.44)."""
    c = HM.inputs(ny, nx, nd, raw=raw)
    r = _rng(ny, nx, nd, 2)
    c['data'] = np.where(r.uniform(size=c['data'].shape) < NEGATED_SHARE, -c['data'], c['data']).astype(F32)
    c['affine'] = _offset_matrices(ny, nx, nd, r).astype(F32)
    return c


def all_clamped(ny, nx, nd, axes='x'):
    """A translation of +-CLAMP_TRANSLATION (the sign alternates with the distance) along ``axes``, that row of the matrix otherwise
    the identity's: every sample of that axis lies beyond the border, where grid_sampler's mask (HoloArgs mx / my) is 0.  The
    other row is _offset_matrices' with its cross term zero, so that its gradient is well-conditioned and the sample does not
    depend on the clamped coordinate."""
    c = HM.inputs(ny, nx, nd, affine='none')
    c['has_affine'] = True
    free = [q for q, a in enumerate('xy') if a not in axes]
    aff = _offset_matrices(ny, nx, nd, _rng(ny, nx, nd, 4), rows=free)
    sg = np.where(np.arange(nd) % 2 == 0, 1., -1.)
    if 'x' in axes:
        aff[:, 0, 2] = sg * CLAMP_TRANSLATION
        aff[:, 1, 0] = 0
    if 'y' in axes:
        aff[:, 1, 2] = -sg * CLAMP_TRANSLATION
        aff[:, 0, 1] = 0
    c['affine'] = aff.astype(F32)
    return c


def border_data(c):
    """The data of an all_clamped case with every pixel replaced by the border pixel of its row / column / the corner that the
    clamped coordinate reads: nothing else may reach the result."""
    ny, nx = c['ny'], c['nx']
    out = c['data'].copy()
    for d in range(c['nd']):
        tx, ty = c['affine'][d, 0, 2], c['affine'][d, 1, 2]
        if abs(tx) == CLAMP_TRANSLATION:
            out[d] = np.repeat(out[d][:, [nx - 1 if tx > 0 else 0]], nx, 1)
        if abs(ty) == CLAMP_TRANSLATION:
            out[d] = np.repeat(out[d][[ny - 1 if ty > 0 else 0], :], ny, 0)
    return out


def zero_probe(ny, nx, nd, unknown_type='real_imag'):
    c = HM.inputs(ny, nx, nd, unknown_type=unknown_type)
    c['probe'] = np.zeros_like(c['probe'])
    return c


def large_shifts(ny, nx, nd, kind='integer'):
    """The shift stage's inputs (uncorrelated data, amplitude 0.1) with shifts (sy, sx) up to beyond the field.  'integer': 0 and
    +-(n + 3), where the registered hologram is the circular roll of |data|; 'fractional': +-(n + 0.37), (-2.5 n, 0.5) and its
    transpose."""
    c = HM.inputs(ny, nx, nd, shifts=True)
    table = {'integer': [(0, 0), (ny + 3, -(nx + 3)), (-(ny + 3), nx + 3), (ny + 3, 0), (0, -(nx + 3))],
             'fractional': [(ny + 0.37, -(nx + 0.37)), (-2.5 * ny, 0.5), (-(ny + 0.37), nx + 0.37), (0.5, -2.5 * nx), (7.3, -(nx / 2 - 0.25))]}[kind]
    c['shifts'] = np.array(table[:nd], F32)
    return c


def rolled_targets(c):
    """sqrt|data| of every distance rolled by its integer shift (fp64)."""
    sh = np.rint(c['shifts']).astype(int)
    assert np.array_equal(sh, c['shifts'])
    return np.stack([np.roll(np.sqrt(np.abs(c['data'][d].astype(np.float64))), tuple(sh[d]), (0, 1)) for d in range(c['nd'])])


# ------------------------------------------------------------------------------------------------------------ the table
BUILDERS = dict(fresnel_phase=fresnel_phase, unitarity=unitarity, delta_beta_turns=lambda *a, **k: delta_beta(*a, kind='turns', **k),
                delta_beta_absorbing=lambda *a, **k: delta_beta(*a, kind='absorbing', **k),
                delta_beta_amplifying=lambda *a, **k: delta_beta(*a, kind='amplifying', **k),
                zero_block=zero_block, negative_data=negative_data, all_clamped=all_clamped, zero_probe=zero_probe, large_shifts=large_shifts)
_F = tuple(FIELDS)
# class -> [(field, builder keywords)]
CASES = {
    'fresnel_phase': [(f, dict(rung=r, sigma=s)) for f in PHASE_FIELDS for r in ('100', '1000', 'max') for s in (1, -1)]
                     + [(f, dict(rung=r, broadband=True)) for f in PHASE_FIELDS for r in ('100', 'max_broadband')],
    'unitarity': [(f, dict(sigma=s)) for f in PHASE_FIELDS for s in (1, -1)],
    'delta_beta_turns': [(f, dict(sigma=s)) for f in _F for s in (1, -1)],
    'delta_beta_absorbing': [(f, dict()) for f in _F],
    'delta_beta_amplifying': [(f, dict()) for f in _F],
    'zero_block': [(f, dict(raw=w, matrices=m)) for f in _F for w in ('intensity', 'magnitude') for m in ('identity', 'offset')],
    'negative_data': [(f, dict(raw=w)) for f in _F for w in ('intensity', 'magnitude')],
    'all_clamped': [(f, dict(axes=a)) for f in _F for a in ('x', 'y', 'xy')],
    'zero_probe': [(_F[0], dict()), (_F[1], dict(unknown_type='delta_beta'))],
    'large_shifts': [(f, dict(kind=k)) for f in _F for k in ('integer', 'fractional')],
}
UNJUDGED_AGAINST_THE_ORACLE = ('unitarity',)       # no reference is a yardstick beyond sincos_fast's claim
# Cases the oracle pair cannot judge in full: what of ``room`` exceeds one third there (the coverage test recomputes the table).
# At the identity the sampling points sit ON pixel centres, where the last bit of a coordinate decides which one-sided derivative
# of the interpolation the matrix gradient takes (the float32 oracle is 1 ... 8800 norms from the fp64 oracle); with 64 rows the
# float32 coordinates miss the centres by an ulp, so the samples on the rim of the zero block are 1e-7 of a pixel's value, not 0,
# and under intensity data their sqrt is 3e-4: the loss differs by 2.5e-4 of itself, the object gradient by 3.9e-4 of its norm.
UNJUDGED = {
    ('zero_block', '64x16-intensity-identity'): ('loss', 'grad', 'gaff'),
    ('zero_block', '64x16-magnitude-identity'): ('gaff',),
    ('zero_block', '32x32-intensity-identity'): ('gaff',),
    ('zero_block', '32x32-magnitude-identity'): ('gaff',),
}


def ident(v):
    f, kw = v
    return '%dx%d' % f + ''.join('-%s' % (k if x is True else x) for k, x in kw.items())


def params(cls):
    return [(cls, f, kw) for f, kw in CASES[cls]]


def case_id(v):
    return ident(v[1:]) if isinstance(v, tuple) and len(v) == 3 else str(v)


def unjudged(p):
    return UNJUDGED.get((p[0], case_id(p)), ())


def case(cls, field, kw):
    """Inputs and the oracle pair (o64, o32) of one case of the table, in holo_matrix's cache."""
    ny, nx = field
    nd = PHASE_FIELDS[field]
    key = (ny, nx, nd, (('value_class', cls),) + tuple(sorted(kw.items())))
    if key not in HM._CASES:
        c = BUILDERS[cls](ny, nx, nd, **kw)
        c['cls'] = cls
        with np.errstate(all='ignore'):
            c['o64'], c['o32'] = HM.oracle_run(c, 'float64'), HM.oracle_run(c, 'float32')
        HM._CASES[key] = c
    return HM._CASES[key]


# ------------------------------------------------------------------------------------------------------------ judgement
def _rel(a, b):
    n = np.linalg.norm(np.asarray(b).ravel())
    d = np.linalg.norm(np.asarray(a).ravel() - np.asarray(b).ravel())
    return float(d / n) if n > 0 else float(d)


def room(c):
    """The float32 oracle's distance from the fp64 oracle as fractions of the bars (grad: the worse of the object and probe
    gradients; a shifted case has gshift and target in place of gaff); each must stay within one third."""
    o, s = c['o64'], c['o32']
    out = dict(pred=_rel(s['pred'], o['pred']) / BARS['pred'], loss=abs(s['loss'] / o['loss'] - 1) / BARS['loss'],
               grad=max(_rel(s['g_obj'], o['g_obj']), _rel(s['g_probe'], o['g_probe'])) / BARS['grad'],
               gdists=_rel(s['g_dists'], o['g_dists']) / BARS['gdists'])
    if c['shifts'] is None:
        out['gaff'] = _rel(s['g_aff'], o['g_aff']) / BARS['gaff']
    else:
        out['gshift'] = _rel(s['g_shifts'], o['g_shifts']) / BARS['gshift']
        out['target'] = _rel(s['target'], o['target']) / BARS['target']
    return out


def phase_ladder(broadband=False):
    """{rung: {bar: the largest fraction of it the float32 oracle uses up over PHASE_FIELDS and both sigma}}."""
    out = {}
    for rad in LADDER:
        worst = {}
        for (ny, nx), nd in PHASE_FIELDS.items():
            for sigma in (1, -1):
                c = _scale_dists(HM.inputs(ny, nx, nd, sigma=sigma, broadband=broadband), rad)
                with np.errstate(all='ignore'):
                    c['o64'], c['o32'] = HM.oracle_run(c, 'float64'), HM.oracle_run(c, 'float32')
                for k, v in room(c).items():
                    worst[k] = max(worst.get(k, 0.), v)
        out[rad] = worst
    return out


def phase_max_of(ladder):
    """The largest rung at which (and below which) every fraction stays within one third."""
    best = None
    for rad in LADDER:
        if max(ladder[rad].values()) > 1. / 3:
            break
        best = rad
    return best


def energy_defect(pred, c, dtype=np.float64):
    """sum pred_d^2 / sum |probe c(obj)|^2 - 1 per distance (accumulated in fp64)."""
    t = HM.transmission(c['obj'], c['unknown_type'], c['sigma'], dtype)
    e0 = (np.abs(c['probe'].astype(np.complex128) * t) ** 2).sum()
    return (np.asarray(pred, np.float64) ** 2).sum(axis=(1, 2)) / e0 - 1


def sample_stats(c):
    """What the registration's samples look like, from the fp64 oracle's restatement of grid_sampler: shares of negative and
    exactly zero samples, of samples whose four corners differ in sign, of samples masked in x / in y, and min |samp| over the
    samples that are not exactly zero."""
    neg = zero = mixed = cx = cy = 0
    low = np.inf
    n = c['data'].size
    for d in range(c['nd']):
        img, th = c['data'][d].astype(np.float64), c['affine'][d].astype(np.float64)
        s = _sampler(img, th, np.float64)
        samp = s['samp']
        neg += int((samp < 0).sum())
        zero += int((samp == 0).sum())
        sgn = np.sign(np.stack(s['corners']))
        mixed += int(((sgn.max(0) > 0) & (sgn.min(0) < 0)).sum())
        cx += int((s['mx'] == 0).sum())
        cy += int((s['my'] == 0).sum())
        if (samp != 0).any():
            low = min(low, float(np.abs(samp[samp != 0]).min()))
    return dict(negative=neg / n, zero=zero / n, mixed=mixed / n, masked_x=cx / n, masked_y=cy / n, min_abs=low)


# ------------------------------------------------------------------------------------------------------------ the float32 mirror
def _base(n, dt):
    """affine_grid's base coordinates as oracle.affine_sample forms them (the linspace from both ends with a fused multiply-add)."""
    dt_ = np.dtype(dt).type
    wide = np.longdouble if np.dtype(dt) == np.float64 else np.float64
    step = wide(dt_(2) / dt_(n - 1))
    i = np.arange(n)
    lo = (wide(-1) + step * i.astype(wide)).astype(dt)
    hi = (wide(1) - step * (n - 1 - i).astype(wide)).astype(dt)
    return (np.where(i < n // 2, lo, hi) * dt_(n - 1)) / dt_(n)


def _sampler(img, th, dt, swap_masks=False):
    """grid_sampler (bilinear, border, align_corners=False) as K3 evaluates it, in ``dt``: samples, corners, weights, masks."""
    H, W = img.shape
    dt_ = np.dtype(dt).type
    X, Y = np.meshgrid(_base(W, dt), _base(H, dt))
    gx = th[0, 0] * X + th[0, 1] * Y + th[0, 2]
    gy = th[1, 0] * X + th[1, 1] * Y + th[1, 2]
    ix = ((gx + dt_(1)) * dt_(W) - dt_(1)) * dt_(0.5)
    iy = ((gy + dt_(1)) * dt_(H) - dt_(1)) * dt_(0.5)
    mx = ((ix > 0) & (ix < W - 1)).astype(dt)
    my = ((iy > 0) & (iy < H - 1)).astype(dt)
    if swap_masks:
        mx, my = my, mx
    ix, iy = np.clip(ix, 0, W - 1), np.clip(iy, 0, H - 1)
    x0, y0 = np.floor(ix).astype(int), np.floor(iy).astype(int)
    wx, wy = (ix - x0).astype(dt), (iy - y0).astype(dt)
    x1, y1 = np.minimum(x0 + 1, W - 1), np.minimum(y0 + 1, H - 1)
    v00, v01, v10, v11 = img[y0, x0], img[y0, x1], img[y1, x0], img[y1, x1]
    samp = v00 * (1 - wx) * (1 - wy) + v01 * wx * (1 - wy) + v10 * (1 - wx) * wy + v11 * wx * wy
    return dict(samp=samp, corners=(v00, v01, v10, v11), wx=wx, wy=wy, mx=mx, my=my, X=X, Y=Y)


def plain_sincos(x):
    x = np.asarray(x, F32)
    return np.sin(x), np.cos(x)


def mirror(c, sincos=plain_sincos, keep_sign=True, guard=True, swap_masks=False):
    """A float32 NumPy restatement of K1 ... K3 for the mutation checks of the coverage test: psi = probe c(obj), FFT2, holo_h with a
    pluggable ``sincos`` (on arg = (c1 * (dist_cm * 1e7f)) * uv2, every product rounded), IFFT2, |.|, the registration's samples,
    the cotangent and the matrix gradient.  ``keep_sign`` = False drops sign(samp) from the cotangent, ``guard`` = False the
    non-finite guard, ``swap_masks`` exchanges mx and my.  Returns pred [nd, ny, nx] and g_aff [nd, 2, 3] (float32)."""
    ny, nx, nd = c['ny'], c['nx'], c['nd']
    t = HM.transmission(c['obj'], c['unknown_type'], c['sigma'], F32)
    F = sfft.fft2((c['probe'].astype(np.complex64) * t).astype(np.complex64))
    uv2 = uv2_of(ny, nx, F32)
    c1 = F32(-(c['sigma'] * O.PI * LAMBDA_NM))
    gscale = F32(2. / (nd * ny * nx))
    pred, g_aff = [], []
    for d in range(nd):
        arg = ((c1 * (F32(c['dists'][d]) * F32(1e7))) * uv2).astype(F32)
        sn, cs = sincos(arg)
        H = (np.asarray(cs, F32) + 1j * np.asarray(sn, F32)).astype(np.complex64)
        mag = np.abs(sfft.ifft2((F * H).astype(np.complex64))).astype(F32)
        s = _sampler(c['data'][d].astype(F32), c['affine'][d].astype(F32), F32, swap_masks)
        samp = s['samp'].astype(F32)
        a = np.abs(samp)
        tgt = np.sqrt(a) if c['raw'] == 'intensity' else a
        diff = mag - tgt
        sg = np.sign(samp) if keep_sign else np.ones_like(samp)
        with np.errstate(all='ignore'):
            cot = (-gscale * diff * (sg / (F32(2) * np.sqrt(a)) if c['raw'] == 'intensity' else sg)).astype(F32)
        if guard:
            cot = np.where(np.abs(cot) <= F32(3.0e38), cot, F32(0))           # (NaN compares false)
        v00, v01, v10, v11 = s['corners']
        with np.errstate(all='ignore'):
            dix = ((v01 - v00) * (1 - s['wy']) + (v11 - v10) * s['wy']) * s['mx'] * F32(0.5 * nx) * cot
            diy = ((v10 - v00) * (1 - s['wx']) + (v11 - v01) * s['wx']) * s['my'] * F32(0.5 * ny) * cot
            g = [[np.sum(dix * s['X'], dtype=np.float64), np.sum(dix * s['Y'], dtype=np.float64), np.sum(dix, dtype=np.float64)],
                 [np.sum(diy * s['X'], dtype=np.float64), np.sum(diy * s['Y'], dtype=np.float64), np.sum(diy, dtype=np.float64)]]
        pred.append(mag)
        g_aff.append(g)
    return dict(pred=np.stack(pred), g_aff=np.array(g_aff, F32))


# ------------------------------------------------------------------------------------------------------------ source ties
# what of adm_holo.hip each class is there for: (function or kernel whose body must hold it, the text, the classes that reach it)
SOURCE_TIES = {
    'zero prediction guard': ('holo_k3', 'const float g = (mag > 0.f) ? A.gscale * diff / mag : 0.f;', ('zero_probe',)),
    'non-finite guard': ('holo_k3', 'if (!(fabsf(cot) <= 3.0e38f)) cot = 0.f;', ('zero_block',)),
    'sign of the sample': ('holo_k3', 'const float sg = (float)((samp > 0.f) - (samp < 0.f));', ('negative_data',)),
    'clamp mask x': ('holo_k3', 'const float mx = (ix > 0.f && ix < (float)(NX - 1)) ? 1.f : 0.f;', ('all_clamped',)),
    'clamp mask y': ('holo_k3', 'const float my = (iy > 0.f && iy < (float)(ny - 1)) ? 1.f : 0.f;', ('all_clamped',)),
    'mask x applied to dix': ('holo_k3', '* mx * (0.5f * (float)NX) * cot;', ('all_clamped',)),
    'mask y applied to diy': ('holo_k3', '* my * (0.5f * (float)ny) * cot;', ('all_clamped',)),
    'Fresnel argument': ('holo_h', 'const float arg = (c1 * (dist_cm * 1e7f)) * uv2;', ('fresnel_phase', 'unitarity')),
    'Fresnel sincos': ('holo_h', 'sincos_fast(arg, sn, cs);', ('fresnel_phase', 'unitarity')),
    'transmission exp': ('holo_transmission', 'const float e = expf(-k1 * o.y);', ('delta_beta_absorbing', 'delta_beta_amplifying')),
    'transmission sincos': ('holo_transmission', 'sincosf(-sigma * k1 * o.x, &sn, &cs);', ('delta_beta_turns',)),
    'shift phase, forward': ('holo_sli', 'sincosf(-2.f * 3.14159265359f * (fx * sx + fft_freq(k, NY) * sy), &sn, &cs);', ('large_shifts',)),
    'shift phase, gradient': ('holo_slf', 'sincosf(-2.f * 3.14159265359f * (fx * sx + fy * sy), &sn, &cs);', ('large_shifts',)),
}
# how often each transcendental may appear in the file: a new call site fails the coverage test until a class names it
CALL_COUNTS = {'sincos_fast(': 1, 'sincosf(': 3, 'expf(': 1}
