"""The VALUE axis of the CTF kernels (adm_holo_ctf.hip C1 ... C5 and ctf_sums_kernel through adm_ctf_fwd_adj and adm_ctfd_fwd_adj,
adm_ctf_invert.hip I1 ... I3 through adm_ctfinv_run; test infrastructure only, importable without a GPU).  tests/ctf_matrix.py,
tests/ctf_dist_matrix.py and tests/ctfinv_matrix.py cover every instantiation on one narrow set of numbers: delta of a few 1e-2
(I = 1 + O(1e-2), min I >= 0.05), lg_kappa 1.7 (one 30 in the inversion), smooth positive data of order 1, 17.05 keV at 1 um,
distances of 40 ... 90 cm.  The classes here are edits of ``ctf_matrix.inputs`` / ``ctfinv_matrix.inputs`` run through the committed
references (tests/ctf_dist_ref.py, tests/ctf_ref.py, tests/ctfinv_ref.py) in fp64 and in float32; they keep ctf_matrix.BARS,
ctf_dist_matrix.dist_bar and the 3 x rule of ctfinv_matrix.VALUE_ERR32.  tests/test_ctf_value_coverage.py decides on the CPU what the
reference pair alone decides, recomputes every figure below, shows by mutation that the cases bite and ties the table to the
sources; tests/test_gpu_ctf_value_domain.py launches every case.

Fields: (32, 16, 2) and (16, 16, 3), the two smallest of ctf_matrix.FIELDS that put several distances into one C3 block and leave
idle C4 slots, and (16, 32, 2) for the classes that move xi (there the long axis is the row stage).  u^2 + v^2 at Nyquist does not
depend on the field's size, so larger fields add nothing to this axis.

The forward/adjoint model sits at ctf_dist_ref.model_dists(d) (float32-exact, the data are made at d), so dL/dd is judged in every
class; every case goes through both entries: the distances as host doubles (c_d rounded once: tests/ctf_ref.py's float32 run is the
yardstick, ``o32h``) and as a float32 device array with grad_dists (tests/ctf_dist_ref.py's, ``o32``).

The rule is value_matrix.py's: the float32 restatement's own distance from fp64 stays within ONE THIRD of BARS for pred, loss, grad
and gkappa, and within BARS['grad'] element-wise relative to max|dL/dd| for the distance gradient (the GPU is then held to
dist_bar).  A case that leaves no room is moved or dropped, never the bar:

  low_I       min I of the fp64 reference set to 0.05, 0.01, 1e-3, 1e-4 by scaling the object (I - 1 is linear in it).  1 / sqrt(I)
              amplifies float32's 6e-8 of I by 1 / (2 I): the delta gradient uses 0.14 / 1.9 of its bar at 0.01 / 1e-3 on
              (32, 16, 2) and 0.09 / 1.8 at 1e-3 / 1e-4 on (16, 16, 3).  LOW_I_MIN records the lowest admitted rung per field; the
              rungs below it are DROPPED.
  data        scaled down the ladder 0.1 / 1e-2 / 1e-4, the residual tends to the prediction itself, q to a constant, and dL/dd to a
              cancelling sum that carries the rounding of its terms: with targets of 0.1 (intensity x 1e-2, magnitude x 0.1) the
              restatement's dL/dd uses up to 0.41 of its bar, with targets of 1e-2 (magnitude x 1e-2, intensity x 1e-4) 1.7 ... 2.7
              bars.  DATA_SMALL records the smallest admitted scale per raw type; the scales below it are DROPPED.
  kappa       lg_kappa = 50: 1 / kappa is exactly 0 in float32 and dL/dlg_kappa is 1e-50 of anything: its relative value means
              nothing; it must be finite and below 1e-37.  Every other rung keeps |dL/dlg_kappa| >= GKAPPA_FLOOR, thirty times
              float32's smallest normal number, so that the one rounding to float32 is a relative 6e-8.
  crossing    the object x 20 and x 30: I passes through 0 continuously and no reference is a yardstick for a gradient whose
              1 / sqrt(I) is unbounded.  Judged per pixel with tol = 10 max|I32 - I64| (``judge_crossing``); gradients finite.

The figures of every class are in ROOM / INV_ERR32 below and in DESIGN.md section 2 ("the CTF value-domain matrix")."""
import numpy as np
import scipy.fft as sfft

from tests import ctf_dist_matrix as DM
from tests import ctf_dist_ref as DR
from tests import ctf_matrix as CM
from tests import ctf_ref as R
from tests import ctfinv_matrix as IM
from tests import ctfinv_ref as IR
from tests.golden import cases
from tests.holo_matrix import rel, bits  # noqa: F401

F32 = np.float32
BARS = CM.BARS
THIRD = 1. / 3
FIELDS = ((32, 16, 2), (16, 16, 3))
XI_FIELDS = FIELDS + ((16, 32, 2),)
RAWS = ('intensity', 'magnitude')

KAPPA_LADDER = (-0.5, 0., 0.7, 3., 8., 30.)
KAPPA_ZERO = 50.                                   # 1 / kappa == 0.0f
GKAPPA_TINY = 1e-37                                # ... |dL/dlg_kappa| there
GKAPPA_FLOOR = 30 * float(np.finfo(F32).tiny)      # a judged dL/dlg_kappa is a normal float32 with room
CONTRAST = (3., 10.)
LOW_I_LADDER = (0.05, 0.01, 1e-3, 1e-4)
LOW_I_MIN = {(32, 16, 2): 0.01, (16, 16, 3): 1e-3}
CROSSING = (20., 30.)
CROSSING_CAP = 0.01                                # at most this share of the pixels within tol of I = 0
DIST_SCALES = {'x1e-3': 1e-3, 'x1e-2': 1e-2, 'x0.1': 0.1}
PHYSICAL = ((500., 5e-6), (17050., 5e-7), (1e5, 6.5e-4))        # (energy eV, pixel cm)
DATA_KINDS = ('zeros', 'negated', 'x1e4', 'small')
DATA_LARGE = 1e4
DATA_SMALL_LADDER = (0.1, 1e-2, 1e-4)
DATA_SMALL = {'intensity': 1e-2, 'magnitude': 0.1}  # the smallest scale of the ladder the rule admits (dL/dd), per raw type
NEGATED_SHARE = 1. / 3
EXACT_KINDS = ('zero_object_unit_data', 'zero_object', 'beta_1e30', 'beta_inf', 'beta_nan')
BETA = {'beta_1e30': 1e30, 'beta_inf': np.inf, 'beta_nan': np.nan}

# The largest fraction of each bar the float32 restatement uses up per class, over the class's cases and both entries (CPU, written
# once; the coverage test recomputes them: none may exceed its figure here, and no figure here twice what is recomputed + 0.002).
ROOM = {
    'kappa_ladder': dict(pred=0.008, loss=0.008, grad=0.025, gkappa=0.042, gdists=0.125),
    'contrast': dict(pred=0.036, loss=0.005, grad=0.010, gkappa=0.001, gdists=0.150),
    'low_I': dict(pred=0.060, loss=0.005, grad=0.140, gkappa=0.011, gdists=0.430),
    'crossing_zero': dict(pred=0.317, loss=0.054, grad=0.192, gkappa=0.015, gdists=0.141),         # (the gapped clip cases)
    'distances': dict(pred=0.008, loss=0.008, grad=0.021, gkappa=0.005, gdists=0.053),
    'physical_scales': dict(pred=0.008, loss=0.011, grad=0.015, gkappa=0.008, gdists=0.118),
    'data': dict(pred=0.007, loss=0.004, grad=0.014, gkappa=0.003, gdists=0.405),
    'exact': dict(pred=0.007, loss=0.004, grad=0.016, gkappa=0.002, gdists=0.073),
}


# ------------------------------------------------------------------------------------------------------------ forward/adjoint inputs
def base(field, raw='intensity', clip=False):
    """ctf_matrix.inputs + where the model sits ('model_dists', float32-exact) + the physical scales the handle is built with."""
    ny, nx, nd = field
    c = dict(CM.inputs(ny, nx, nd, raw=raw, clip=clip))
    c['obj'], c['data'] = c['obj'].copy(), c['data'].copy()
    c['energy'], c['psize'] = CM.ENERGY_EV, CM.PSIZE_CM
    c['model_dists'] = DR.model_dists(c['dists'])
    return c


def _scale_object(c, s):
    c['obj'][..., 0] = (c['obj'][..., 0].astype(np.float64) * s).astype(F32)
    return c


def kappa_ladder(field, lg_kappa):
    """lg_kappa of the ladder; the object scaled by min(1, 10^(lg_kappa - 1.7)) so that I keeps the table's range when osc grows
    like 2 / kappa."""
    c = _scale_object(base(field), min(1., 10. ** (lg_kappa - CM.LG_KAPPA)))
    c['lg_kappa'] = F32(lg_kappa)
    return c


def contrast(field, scale):
    return _scale_object(base(field), scale)


def fp64_I(c):
    return DR.forward_adjoint(c['obj'][..., 0], c['model_dists'], c['lg_kappa'], c['data'], c['energy'], c['psize'], c['raw'])['I']


def low_I(field, rung):
    """The object scaled so that the fp64 reference's min I is ``rung`` (I - 1 is linear in the object)."""
    c = base(field)
    return _scale_object(c, (1. - rung) / (1. - float(fp64_I(c).min())))


def crossing_zero(field, scale=None, clip=False):
    """The object x ``scale``: I passes through 0, no gap.  ``clip``: ctf_matrix's gapped clip case, for the device-distance entry."""
    return base(field, clip=True) if clip else _scale_object(base(field), scale)


def distances(field, kind):
    """The table's distances x 1e-3 / 1e-2 / 0.1; distance 1 exactly 0; distance 0 negated."""
    c = base(field)
    if kind in DIST_SCALES:
        c['dists'] = c['dists'] * DIST_SCALES[kind]
        c['model_dists'] = DR.model_dists(c['dists'])
    elif kind == 'zero':
        c['model_dists'][1] = 0.
    elif kind == 'negative':
        c['model_dists'][0] = -c['model_dists'][0]
    else:
        raise KeyError(kind)
    return c


def max_xi(c, dists=None):
    d = c['model_dists'] if dists is None else dists
    return float(R.PI * (1240. / c['energy']) * np.abs(d).max() * 1e7 * R.uv2((c['ny'], c['nx']), c['psize']).max())


def physical_scales(field, energy, psize):
    """Another energy and pixel size, the distances rescaled so that the largest xi is the table's: xi, I and the data are the
    table's up to rounding, every host-side scale (c_d, pil, dscale, the u^2 + v^2 upload) moves by decades."""
    c = base(field)
    want = max_xi(c, c['dists'])
    c['energy'], c['psize'] = float(energy), float(psize)
    c['dists'] = c['dists'] * (want / max_xi(c, c['dists']))
    c['model_dists'] = DR.model_dists(c['dists'])
    return c


def _rng(field, k):
    return cases.rng(9700 + 31 * field[0] + 7 * field[1] + field[2] + 1000 * k)


def zero_pattern(field):
    ny, nx, nd = field
    d, y, x = np.mgrid[:nd, :ny, :nx]
    return (y * nx + x + 3 * d) % 7 == 0


def data(field, raw, kind, scale=None):
    """Edits of the measured data: a seventh of the values exactly 0; a third negated ('plain_data': before the edit); x 1e4;
    'small': x DATA_SMALL[raw] (``scale``: another rung of the ladder)."""
    c = base(field, raw=raw)
    c['plain_data'] = c['data'].copy()
    if kind == 'zeros':
        c['data'][zero_pattern(field)] = 0
    elif kind == 'negated':
        neg = _rng(field, 1).uniform(size=c['data'].shape) < NEGATED_SHARE
        c['data'] = np.where(neg, -c['data'], c['data']).astype(F32)
    else:
        c['data'] = (c['data'].astype(np.float64) * (scale or (DATA_LARGE if kind == 'x1e4' else DATA_SMALL[raw]))).astype(F32)
    return c


def exact(field, kind):
    c = base(field)
    if kind.startswith('zero_object'):
        c['obj'][..., 0] = 0
        if kind == 'zero_object_unit_data':
            c['data'][:] = 1
    else:
        c['obj'][..., 1] = F32(BETA[kind])
    return c


def nonfinite_data(field):
    """One NaN and one Inf in the data of distance 1 only ('plain_data': before the edit)."""
    c = base(field)
    c['plain_data'] = c['data'].copy()
    ny, nx, _ = field
    c['data'][1, ny // 3, nx // 2] = np.nan
    c['data'][1, ny - 2, 1] = np.inf
    return c


BUILDERS = dict(plain=base, kappa_ladder=kappa_ladder, contrast=contrast, low_I=low_I, crossing_zero=crossing_zero, distances=distances,
                physical_scales=physical_scales, data=data, exact=exact, nonfinite_data=nonfinite_data)
# class -> [(field, builder keywords)]
CASES = {
    'kappa_ladder': [(f, dict(lg_kappa=k)) for f in FIELDS for k in KAPPA_LADDER + (KAPPA_ZERO,)],
    'contrast': [(f, dict(scale=s)) for f in FIELDS for s in CONTRAST],
    'low_I': [(f, dict(rung=r)) for f in FIELDS for r in LOW_I_LADDER if r >= LOW_I_MIN[f]],
    'crossing_zero': [(f, dict(scale=s)) for f in FIELDS for s in CROSSING] + [(f, dict(clip=True)) for f in FIELDS],
    'distances': [(f, dict(kind=k)) for f in XI_FIELDS for k in tuple(DIST_SCALES) + ('zero', 'negative')],
    'physical_scales': [(f, dict(energy=e, psize=p)) for f in XI_FIELDS for e, p in PHYSICAL],
    'data': [(f, dict(raw=w, kind=k)) for f in FIELDS for w in RAWS for k in DATA_KINDS],
    'exact': [(f, dict(kind=k)) for f in FIELDS for k in EXACT_KINDS],
    'nonfinite_data': [(f, dict()) for f in FIELDS],
}
# class -> (the GPU test that runs it, what of the sources it is there for)
CLASS_TESTS = {
    'kappa_ladder': 'test_kappa_ladder', 'contrast': 'test_contrast', 'low_I': 'test_low_I', 'crossing_zero': 'test_crossing_zero',
    'distances': 'test_distances', 'physical_scales': 'test_physical_scales', 'data': 'test_data', 'exact': 'test_exact',
    'nonfinite_data': 'test_nonfinite_data',
    'inv_kappa_ladder': 'test_inv_kappa_ladder', 'inv_alpha_ladder': 'test_inv_alpha_ladder', 'inv_data': 'test_inv_data',
    'inv_nonfinite_batch_entry': 'test_inv_nonfinite_batch_entry',
}
FWD_KERNELS = ('ctf_c1', 'ctf_c2', 'ctf_c3', 'ctf_c4', 'ctf_c5', 'ctf_sums_kernel')
INV_KERNELS = ('ctfinv_i1', 'ctfinv_i2', 'ctfinv_i3')


def ident(v):
    f, kw = v
    return '%dx%dx%d' % f + ''.join('-%s' % (k if x is True else ('%g' % x if isinstance(x, float) else x)) for k, x in kw.items())


def params(cls):
    return [(cls, f, kw) for f, kw in CASES[cls]]


def case_id(p):
    return ident(p[1:]) if isinstance(p, tuple) and len(p) == 3 else str(p)


def judged(p):
    """The quantities of a case that are held to the reference (and to the one-third rule)."""
    cls, _, kw = p
    if cls == 'nonfinite_data' or (cls == 'crossing_zero' and not kw.get('clip')) or kw.get('kind') == 'zero_object_unit_data':
        return ()
    if kw.get('kind') == 'zero_object':
        return ('pred', 'loss', 'grad')                           # F = 0: dL/dlg_kappa and dL/dd are exactly 0
    if cls == 'kappa_ladder' and kw['lg_kappa'] == KAPPA_ZERO:
        return ('pred', 'loss', 'grad', 'gdists')
    return ('pred', 'loss', 'grad', 'gkappa', 'gdists')


def ref_pair(c):
    """o64, o32 (ctf_dist_ref: the device entry's roundings) and o32h (ctf_ref: the host entry's) of a case, in place."""
    a = (c['obj'][..., 0], c['model_dists'], c['lg_kappa'], c['data'], c['energy'], c['psize'], c['raw'])
    with np.errstate(all='ignore'):
        c['o64'], c['o32'] = DR.forward_adjoint(*a, dtype='float64'), DR.forward_adjoint(*a, dtype='float32')
        c['o32h'] = R.forward_adjoint(*a, dtype='float32')
    return c


_CASES = {}


def case(cls, field, kw):
    """Inputs and the reference runs of one case of the table ('plain': the unedited inputs the bit-for-bit relations compare
    with), built once per process."""
    key = (cls, field, tuple(sorted(kw.items())))
    if key not in _CASES:
        c = BUILDERS[cls](field, **kw)
        c['cls'], c['name'] = cls, '%s %s' % (cls, ident((field, kw)))
        _CASES[key] = ref_pair(c)
    return _CASES[key]


# ------------------------------------------------------------------------------------------------------------ judgement
def _finite(x):
    return float(x) if np.isfinite(x) else np.inf


def errors(out, o64):
    """Distances of a run (the reference's keys) from the fp64 reference: pred, grad (relative, whole array), loss, gkappa
    (relative), gdists (element-wise, relative to max|dL/dd|; only where the run has it).  Non-finite -> inf."""
    with np.errstate(all='ignore'):
        e = dict(pred=_finite(rel(out['pred'], o64['pred'])), loss=_finite(abs(np.float64(out['loss']) / np.float64(o64['loss']) - 1)),
                 grad=_finite(rel(out['grad_delta'], o64['grad_delta'])),
                 gkappa=_finite(abs(np.float64(out['grad_lg_kappa']) / np.float64(o64['grad_lg_kappa']) - 1)))
        if 'grad_dists' in out and 'grad_dists' in o64:
            d = DM.dist_errors(out['grad_dists'], o64['grad_dists'])
            e['gdists'] = _finite(d.max()) if np.isfinite(d).all() else np.inf
    return e


def room(c, keys=None):
    """The float32 restatements' distances from fp64 as fractions of the bars -- the worse of the two entries' restatements; each
    must stay within one third (gdists: within one)."""
    a, b = errors(c['o32'], c['o64']), errors(c['o32h'], c['o64'])
    out = {k: max(a[k], b.get(k, 0.)) / BARS['grad' if k == 'gdists' else k] for k in a}
    return {k: v for k, v in out.items() if keys is None or k in keys}


def leaves_room(c, keys):
    r = room(c, keys)
    return all(v <= (1. if k == 'gdists' else THIRD) for k, v in r.items())


def bars_used(out, c, keys, o32='o32'):
    """How many of the GPU's bars a run uses up, as tests/test_gpu_ctf.py:check_whole and test_gpu_ctf_dist.py:check_dists judge it:
    pred, loss under BARS; grad under min(BARS['grad'], 3 x the restatement); gkappa under max(BARS['gkappa'], 3 x); dL/dd element
    by element under dist_bar.  A run passes when the largest is <= 1."""
    e, e32 = errors(out, c['o64']), errors(c[o32], c['o64'])
    u = dict(pred=e['pred'] / BARS['pred'], loss=e['loss'] / BARS['loss'], grad=e['grad'] / min(BARS['grad'], 3 * e32['grad']),
             gkappa=e['gkappa'] / max(BARS['gkappa'], 3 * e32['gkappa']))
    if 'grad_dists' in out and 'grad_dists' in c[o32]:
        with np.errstate(all='ignore'):
            d = DM.dist_errors(out['grad_dists'], c['o64']['grad_dists']) / DM.dist_bar(c)
        u['gdists'] = float(d.max()) if np.isfinite(d).all() else np.inf
    return {k: v for k, v in u.items() if k in keys}


def crossing_tol(c):
    return 10. * float(np.abs(c['o32']['I'].astype(np.float64) - c['o64']['I']).max())


def judge_crossing(pred, loss, c):
    """The prediction and the loss of a case whose I passes through 0, with tol = 10 max|I32 - I64| of the restatement pair: per
    pixel exactly +0 where I64 <= -tol, within [0, sqrt(2 tol)] where |I64| < tol; where I64 >= tol within BARS['pred'] of
    sqrt(I64), relative to the array; the loss within BARS['loss'] + (pixels within tol) 2 tol / (sum of squared residuals).
    Asserts; returns the figures."""
    I, tol = c['o64']['I'], crossing_tol(c)
    pred = np.asarray(pred)
    neg, pos = I <= -tol, I >= tol
    band = ~(neg | pos)
    assert band.sum() <= CROSSING_CAP * I.size, (c['name'], int(band.sum()))
    assert neg.sum() >= 1 and pos.sum() >= I.size // 2, (c['name'], int(neg.sum()), int(pos.sum()))
    assert not bits(pred[neg]).any(), (c['name'], 'prediction not +0 where I <= -tol', int((bits(pred[neg]) != 0).sum()))
    assert ((pred[band] >= 0) & (pred[band] <= np.sqrt(2 * tol))).all(), (c['name'], 'within tol of I = 0', pred[band])
    want = np.sqrt(I[pos])
    e = float(np.linalg.norm(pred[pos].astype(np.float64) - want) / np.linalg.norm(want))
    assert e < BARS['pred'], (c['name'], 'pred where I >= tol', e)
    el = abs(loss / c['o64']['loss'] - 1)
    bar = BARS['loss'] + band.sum() * 2 * tol / c['o64']['loss_d'].sum()
    assert el < bar, (c['name'], 'loss', el, bar)
    return dict(tol=tol, clipped=int(neg.sum()), within_tol=int(band.sum()), pred=e, loss=float(el), loss_bar=float(bar))


def closed_form_at_zero_distance(c):
    """sqrt(1 + 2 D / kappa): the prediction of a distance that is exactly 0 (xi = 0, osc = 2 / kappa at every frequency)."""
    return np.sqrt(1. + 2. * c['obj'][..., 0].astype(np.float64) / 10. ** float(c['lg_kappa']))


# ------------------------------------------------------------------------------------------------------------ the inversion
# class -> {case: keywords of ctfinv_matrix.inputs + the edit}.  PHASE_FIELD, and (16, 32, 2) for the kappa ladder.
INV_FIELDS = (IM.PHASE_FIELD, (16, 32, 2))
INV_KAPPA_LADDER = (-0.5, 0., 0.7, 3., 8., 50.)
INV_ALPHA_LADDER = (1e-30, 1e-20, 1e-6, 1., 1e3, 1e6)
INV_CONTRAST = 1e4
INV_CASES = {
    'inv_kappa_ladder': {'%dx%dx%d-lg_kappa-%g' % (f + (k,)): dict(field=f, lg_kappa=k) for f in INV_FIELDS for k in INV_KAPPA_LADDER},
    'inv_alpha_ladder': {'alpha-%g' % a: dict(field=IM.PHASE_FIELD, alpha=a) for a in INV_ALPHA_LADDER},
    'inv_data': {'contrast_x1e4': dict(field=IM.PHASE_FIELD, edit='contrast'), 'zeros_and_negated': dict(field=IM.PHASE_FIELD, edit='signs')},
}
INV_NONFINITE = dict(field=IM.PHASE_FIELD, nb=3, max_batch=3)
INV_ADMIT = 1e-4            # a case whose restatement is further from fp64 is not admitted
# The float32 restatement's distance from fp64 per case (relative, whole array; CPU, written once; the coverage test recomputes
# them).  The GPU's bar is 3 x the figure, as ctfinv_matrix.VALUE_ERR32 has it.
INV_ERR32 = {
    ('inv_kappa_ladder', '32x16x2-lg_kappa--0.5'): 6.8e-05, ('inv_kappa_ladder', '16x32x2-lg_kappa--0.5'): 6.7e-05,
    ('inv_kappa_ladder', '32x16x2-lg_kappa-0'): 3.7e-06, ('inv_kappa_ladder', '16x32x2-lg_kappa-0'): 3.6e-06,
    ('inv_kappa_ladder', '32x16x2-lg_kappa-0.7'): 3.5e-06, ('inv_kappa_ladder', '16x32x2-lg_kappa-0.7'): 2.1e-06,
    ('inv_kappa_ladder', '32x16x2-lg_kappa-3'): 8.8e-07, ('inv_kappa_ladder', '16x32x2-lg_kappa-3'): 1.0e-06,
    ('inv_kappa_ladder', '32x16x2-lg_kappa-8'): 1.4e-06, ('inv_kappa_ladder', '16x32x2-lg_kappa-8'): 1.6e-06,
    ('inv_kappa_ladder', '32x16x2-lg_kappa-50'): 2.5e-06, ('inv_kappa_ladder', '16x32x2-lg_kappa-50'): 2.1e-06,
    ('inv_alpha_ladder', 'alpha-1e-30'): 3.1e-06, ('inv_alpha_ladder', 'alpha-1e-20'): 3.1e-06, ('inv_alpha_ladder', 'alpha-1e-06'): 3.1e-06,
    ('inv_alpha_ladder', 'alpha-1'): 4.6e-07, ('inv_alpha_ladder', 'alpha-1000'): 9.6e-07, ('inv_alpha_ladder', 'alpha-1e+06'): 9.7e-07,
    ('inv_data', 'contrast_x1e4'): 3.1e-06,            # the phase reaches 625 rad
    ('inv_data', 'zeros_and_negated'): 4.9e-07,        # ... 20 rad: a stray fabs moves it by O(1)
}


def inv_inputs(field, lg_kappa=IM.LG_KAPPA, alpha=None, edit=None, nb=1, max_batch=1):
    c = IM.inputs(field, nb=nb, max_batch=max_batch, lg_kappa=lg_kappa)
    c['data'] = c['data'].copy()
    if alpha is not None:
        c['alpha_kind'], c['alpha'] = 'constant', F32(alpha)
    if edit == 'contrast':
        c['data'] = (1. + INV_CONTRAST * (c['data'].astype(np.float64) - 1.)).astype(F32)
    elif edit == 'signs':
        ny, nx, nd = field
        c['data'][0][zero_pattern(field)] = 0
        neg = _rng(field, 2).uniform(size=c['data'].shape) < NEGATED_SHARE
        c['data'] = np.where(neg, -c['data'], c['data']).astype(F32)
    return c


def inv_case(cls, name):
    key = ('inv', cls, name)
    if key not in _CASES:
        c = inv_inputs(**INV_CASES[cls][name])
        c['name'] = '%s %s' % (cls, name)
        with np.errstate(all='ignore'):
            c['o64'], c['o32'] = IM.ref_run(c, 'float64'), IM.ref_run(c, 'float32')
        c['bar'] = 3 * INV_ERR32.get((cls, name), np.nan)
        _CASES[key] = c
    return _CASES[key]


def inv_params(cls):
    return [(cls, name) for name in INV_CASES[cls]]


def inv_nonfinite():
    """Three angles, max_batch 3; a NaN and an Inf in the holograms of angle 1 ('plain_data': before the edit).  On PHASE_FIELD I1's
    first block holds the 64 rows of angle 0 and the 64 of angle 1."""
    c = inv_inputs(**INV_NONFINITE)
    c['plain_data'] = c['data'].copy()
    c['data'][1, 0, 5, 3] = np.nan
    c['data'][1, 1, 20, 11] = np.inf
    return c


# ------------------------------------------------------------------------------------------------------------ the float32 mirrors
FWD_MUTANTS = ('no_abs_on_data', 'q_not_zeroed', 'clipped_kept_in_gdists', 'clipped_kept_in_gkappa', 'inv_kappa_dropped',
               'inv_kappa_on_sine', 'inv_kappa_clamped_to_1', 'inv_kappa_flushed_below_1e-7', 'beta_added_to_delta', 'dscale_at_table_energy')
INV_MUTANTS = ('abs_in_inversion', 'denominator_without_2', 'alpha_multiplied')


def mirror(c, mut=None, rounding='device'):
    """tests/ctf_dist_ref.forward_adjoint in float32, line by line (``rounding`` 'host': c_d rounded once like tests/ctf_ref.py),
    with one mistake of FWD_MUTANTS switched on by ``mut``.  Unmutated it gives the restatement's bits."""
    assert mut is None or mut in FWD_MUTANTS, mut
    dt = F32
    energy, psize = c.get('energy', CM.ENERGY_EV), c.get('psize', CM.PSIZE_CM)
    dists = np.asarray(c['model_dists'] if 'model_dists' in c else c['dists'], np.float64).reshape(-1)
    D = np.asarray(c['obj'][..., 0], dtype=dt)
    if mut == 'beta_added_to_delta':
        D = (D + np.asarray(c['obj'][..., 1], dtype=dt)).astype(dt)
    nd, n = len(dists), D.size
    q2 = R.uv2(D.shape, psize, dt)
    if rounding == 'device':
        xi = np.stack([cd * q2 for cd in DR.c_of(dists, energy, dt)]).astype(dt)
    else:
        xi = np.stack([dt(R.PI * (1240. / energy) * (float(d) * 1e7)) * q2 for d in dists])
    sn, cs = np.sin(xi), np.cos(xi)
    lgk = float(c['lg_kappa'])
    ik = dt(1. / 10. ** lgk)
    kscale = 2. * R.LN10 / 10. ** lgk                              # the kappa gradient's scale, a double
    if mut == 'inv_kappa_clamped_to_1' and ik > 1:
        ik, kscale = dt(1), 2. * R.LN10
    if mut == 'inv_kappa_flushed_below_1e-7' and ik < 1e-7:
        ik, kscale = dt(0), 0.
    if mut == 'inv_kappa_dropped':
        o, dxi = dt(2) * sn, dt(2) * cs
    elif mut == 'inv_kappa_on_sine':
        o, dxi = dt(2) * (ik * sn + cs), dt(2) * (ik * cs - sn)
    else:
        o, dxi = dt(2) * (sn + ik * cs), dt(2) * (cs - ik * sn)
    F = sfft.fft2(D)
    I = (dt(1) + sfft.ifft2(o * F).real).astype(dt)
    pos = I > 0
    with np.errstate(all='ignore'):
        pred = np.sqrt(np.where(pos, I, dt(0))).astype(dt)
        raw = np.asarray(c['data'], dtype=dt)
        a = raw if mut == 'no_abs_on_data' else np.abs(raw)
        diff = pred - (np.sqrt(a) if c['raw'] == 'intensity' else a)
        loss_d = (diff.astype(np.float64) ** 2).sum(axis=(1, 2))
        kept = (diff / (pred * dt(nd * n))).astype(dt)
        q = np.where(pos, kept, dt(0)).astype(dt)
        Q, Qkept = sfft.fft2(kept if mut == 'q_not_zeroed' else q), sfft.fft2(kept)
        out = dict(I=I, pred=pred, loss=float(loss_d.sum() / (nd * n)), loss_d=loss_d)
        out['grad_delta'] = sfft.ifft2((o * Q).sum(axis=0)).real.astype(dt)
        Qk = Qkept if mut == 'clipped_kept_in_gkappa' else Q
        out['grad_lg_kappa'] = float(-kscale / n * (np.conj(Qk).astype(np.complex128) * cs * F).real.sum())
        Qd = Qkept if mut == 'clipped_kept_in_gdists' else Q
        g_osc = ((Qd.real * F.real + Qd.imag * F.imag) / dt(n)).astype(dt)
        g_c = ((g_osc * dxi).astype(dt) * q2).sum(axis=(1, 2), dtype=dt)
        e = CM.ENERGY_EV if mut == 'dscale_at_table_energy' else energy
        out['grad_dists'] = np.asarray(g_c * dt(R.PI * (1240. / e)) * dt(1e7), dtype=np.float64)
    return out


def inv_mirror(c, mut=None):
    """tests/ctfinv_ref.retrieve in float32, line by line, with one mistake of INV_MUTANTS switched on by ``mut``."""
    assert mut is None or mut in INV_MUTANTS, mut
    dt = F32
    alpha = np.asarray(IR.ALPHA if c['alpha'] is None else c['alpha'], dtype=dt)
    out = []
    for I in np.asarray(c['data'], dtype=dt):
        if mut == 'abs_in_inversion':
            I = np.abs(I)
        w = IR.weights(I.shape[1:], c['dists'], c['lg_kappa'], IM.ENERGY_EV, IM.PSIZE_CM, dt)
        F = sfft.fft2(I - dt(1), norm='ortho')
        num = (w * F).sum(axis=0)
        s = ((w ** 2) if mut == 'denominator_without_2' else (dt(2) * w ** 2)).sum(axis=0)
        den = s * alpha if mut == 'alpha_multiplied' else s + alpha
        with np.errstate(all='ignore'):
            out.append(sfft.ifft2(num / den, norm='ortho').real.astype(dt))
    return np.stack(out)


# mutant -> the cases of this matrix that must reject it by at least REJECT bars: (class, field or inversion case name, keywords)
REJECT = 10.
MUTANT_CASES = {
    'no_abs_on_data': [('data', f, dict(raw=w, kind='negated')) for f in FIELDS for w in RAWS],
    'q_not_zeroed': [('crossing_zero', f, dict(clip=True)) for f in FIELDS],
    'clipped_kept_in_gdists': [('crossing_zero', f, dict(clip=True)) for f in FIELDS],
    'clipped_kept_in_gkappa': [('crossing_zero', f, dict(clip=True)) for f in FIELDS],
    'inv_kappa_dropped': [('kappa_ladder', f, dict(lg_kappa=k)) for f in FIELDS for k in (-0.5, 0., 0.7, 3.)],
    'inv_kappa_on_sine': [('kappa_ladder', f, dict(lg_kappa=k)) for f in FIELDS for k in (-0.5, 0.7, 3.)],
    'inv_kappa_clamped_to_1': [('kappa_ladder', f, dict(lg_kappa=-0.5)) for f in FIELDS],
    'inv_kappa_flushed_below_1e-7': [('kappa_ladder', f, dict(lg_kappa=k)) for f in FIELDS for k in (8., 30.)],
    'beta_added_to_delta': [('exact', f, dict(kind=k)) for f in FIELDS for k in BETA],
    'dscale_at_table_energy': [('physical_scales', f, dict(energy=e, psize=p)) for f in XI_FIELDS for e, p in PHYSICAL if e != CM.ENERGY_EV],
    'abs_in_inversion': [('inv_data', 'zeros_and_negated')],
    'denominator_without_2': [('inv_alpha_ladder', 'alpha-%g' % a) for a in INV_ALPHA_LADDER[:4]],
    'alpha_multiplied': [('inv_alpha_ladder', 'alpha-%g' % a) for a in INV_ALPHA_LADDER if a != 1.],
}
# What the existing tables already see (the coverage test recomputes it): the old case that rejects the mutant, or None where every
# case of ctf_matrix, ctf_dist_matrix and ctfinv_matrix accepts it -- the gap this matrix closes.
CAUGHT_BEFORE = {
    'no_abs_on_data': None, 'abs_in_inversion': None, 'clipped_kept_in_gdists': None, 'dscale_at_table_energy': None,
    'inv_kappa_clamped_to_1': None, 'inv_kappa_flushed_below_1e-7': None,
    'q_not_zeroed': 'ctf_matrix clip', 'clipped_kept_in_gkappa': 'ctf_matrix clip',
    'inv_kappa_dropped': 'ctf_matrix 16x16x1', 'inv_kappa_on_sine': 'ctf_matrix 16x16x1', 'beta_added_to_delta': 'ctf_matrix 16x16x1',
    'denominator_without_2': 'ctfinv_matrix 16x16x1', 'alpha_multiplied': 'ctfinv_matrix 16x16x1',
}


def old_forward_cases():
    """(name, case, rounding, judged keys) of every forward/adjoint case the existing tables compare with a reference."""
    out = [('ctf_matrix %dx%dx%d' % f, CM.case(*f), 'host') for f in CM.FIELDS]
    out.append(('ctf_matrix magnitude', CM.case(*CM.VARIANT_FIELD, raw='magnitude'), 'host'))
    out += [('ctf_matrix %g rad' % p, CM.case(*CM.PHASE_FIELD, phase=p), 'host') for p in CM.PHASE_RUNGS]
    out.append(('ctf_matrix clip', CM.case(*CM.VARIANT_FIELD, clip=True), 'host'))
    out += [('ctf_dist_matrix %dx%dx%d' % f, DM.case(*f), 'device') for f in DM.FIELDS]
    out.append(('ctf_dist_matrix %g rad' % DM.PHASE_RUNG, DM.case(*DM.PHASE_FIELD, phase=DM.PHASE_RUNG), 'device'))
    return out


def old_inversion_cases():
    return [('ctfinv_matrix %s' % n, IM.case(n)) for n in list(IM.CASES) + list(IM.VALUE_CASES)]


def rejected_before(mut):
    """The first case of the existing tables that rejects the mutant (judged as their GPU modules judge, whole arrays), or None."""
    for name, c in (old_inversion_cases() if mut is None or mut in INV_MUTANTS else []):
        e = rel(inv_mirror(c, mut), np.asarray(c['o64']).reshape(c['nb'], c['ny'], c['nx']))
        if not e <= c['bar']:
            return name
    for name, c, rounding in (old_forward_cases() if mut is None or mut in FWD_MUTANTS else []):
        out = mirror(c, mut, rounding)
        keys = ('pred', 'loss', 'grad', 'gkappa') + (('gdists',) if rounding == 'device' else ())
        if not all(np.isfinite(out[k]).all() for k in ('pred', 'grad_delta', 'grad_lg_kappa')) or max(bars_used(out, c, keys).values()) > 1:
            return name
    return None


def rejection(mut, p):
    """How many bars the mutant is from passing the case ``p`` of this matrix (inf: a non-finite output)."""
    if len(p) == 2:
        c = inv_case(*p)
        return _finite(rel(inv_mirror(c, mut), c['o64'])) / c['bar']
    c = case(*p)
    keys = judged(p)
    return max(max(bars_used(mirror(c, mut, r), c, keys if r == 'device' else tuple(k for k in keys if k != 'gdists'), o32).values())
               for r, o32 in (('device', 'o32'), ('host', 'o32h')))


# ------------------------------------------------------------------------------------------------------------ source ties
# what of the sources each class is there for: (file, the text that must be in it, the classes that reach it)
SOURCE_TIES = {
    'abs of the measured value': ('adm_holo_ctf.hip', 'const float as = fabsf(meas[j]);', ('data',)),
    'the prediction clip': ('adm_holo_ctf.hip', 'const float pr = (I > 0.f) ? sqrtf(I) : 0.f;', ('low_I', 'crossing_zero')),
    'q zeroed where I <= 0': ('adm_holo_ctf.hip', '(ok && I > 0.f) ? A.qscale * diff / pr : 0.f', ('crossing_zero', 'nonfinite_data')),
    '1 / kappa in double': ('adm_holo_ctf.hip', 'return exp(-2.302585092994045684 * (double)lg_kappa[0]);', ('kappa_ladder',)),
    'osc': ('adm_holo_ctf.hip', 'return 2.f * (sn + inv_kappa * cs);', ('kappa_ladder', 'contrast', 'distances')),
    'the kappa gradient scale': ('adm_holo_ctf.hip', '-2.0 * 2.302585092994045684 * inv_kappa_f64(A.lg_kappa) * (double)A.inv_n * s', ('kappa_ladder',)),
    'dL/dd term': ('adm_holo_ctf.hip', 'dacc += (double)((cs - ik * sn) * uv2) * (double)(q.x * f.x + q.y * f.y);', ('distances', 'kappa_ladder')),
    'the model reads delta alone': ('adm_holo_ctf.hip', 'A.obj[(size_t)y * NX + x].x : 0.f', ('exact',)),
    'c_d on the device': ('adm_holo_ctf.hip', 'mul_rounded(A.pil, mul_rounded(A.dists_dev[d], 1e7f))', ('physical_scales', 'distances')),
    'c_d on the host': ('adm_holo_ctf.hip', 'A.c[i] = (float)(3.14159265359 * lambda_nm * (dists_cm[i] * 1e7));', ('physical_scales', 'distances')),
    'pil': ('adm_holo_ctf.hip', 'A.pil = (float)(3.14159265359 * lambda_nm);', ('physical_scales',)),
    'dscale': ('adm_holo_ctf.hip', 'A.dscale = 2.0 * 3.14159265359 * lambda_nm * 1e7 / (double)n;', ('physical_scales',)),
    'qscale': ('adm_holo_ctf.hip', 'A.qscale = (float)(1.0 / ((double)n * d.n_dists));', ('contrast', 'data')),
    'the frequency mesh': ('adm_line_host.h', 'const float u = (float)(((double)ky / ny) / voxel_nm_y);', ('physical_scales',)),
    'the device-distance entry': ('adm_ctf_dist.hip', 'ctf::group_run(h, "adm_ctfd_fwd_adj", obj, nullptr, dists_cm_dev,', tuple(CASES)),
    'the data as given': ('adm_ctf_invert.hip', 'ok ? A.data[row + x] - 1.f : 0.f', ('inv_data', 'inv_nonfinite_batch_entry')),
    'w': ('adm_ctf_invert.hip', 'const float w = sn + ik * cs;', ('inv_kappa_ladder',)),
    'the denominator': ('adm_ctf_invert.hip', 'den[j] = fmaf(2.f * w, w, den[j]);', ('inv_alpha_ladder', 'inv_kappa_ladder')),
    'alpha added': ('adm_ctf_invert.hip', 'const float q = den[j] + al[j];', ('inv_alpha_ladder',)),
    "the inversion's 1 / kappa": ('adm_ctf_invert.hip', '*slot = (float)exp(-2.302585092994045684 * (double)lg_kappa[0]);', ('inv_kappa_ladder',)),
}


if __name__ == '__main__':
    worst = {}
    for cls in CASES:
        for p in params(cls):
            c, keys = case(*p), judged(p)
            if not keys:
                continue
            r = room(c, keys)
            print('%-60s %s  min I %.4g  gkappa %.3g' % (c['name'], '  '.join('%s %.3f' % kv for kv in r.items()), c['o64']['I'].min(),
                                                      c['o64']['grad_lg_kappa']))
            for k, v in r.items():
                worst.setdefault(cls, {})[k] = max(worst.get(cls, {}).get(k, 0.), v)
    for cls, w in worst.items():
        print("    '%s': dict(%s)," % (cls, ', '.join('%s=%.3f' % (k, np.ceil(v * 1000) / 1000) for k, v in w.items())))
    for cls in INV_CASES:
        for _, name in inv_params(cls):
            c = inv_case(cls, name)
            print("    ('%s', '%s'): %.2g,   # max |phase| %.3g" % (cls, name, rel(c['o32'], c['o64']) * 1.05, np.abs(c['o64']).max()))
