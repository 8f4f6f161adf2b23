"""The OPTION axis of the three small-parameter gradients of the streamed multislice plan (test infrastructure only; importable
without a GPU):

  dL/dz  slice positions of sparse multislice         st_col_conv_sparse_kernel<>, st_dd_reduce_kernel     tests/sparse_ref.py
  dL/ds  per-angle exit-wave offsets                  es_col_conv_kernel<>, st_shift_reduce_kernel         tests/prj_offset_ref.py
  dL/dd  detector distances of a refined fan-out      md_fanout_kernel<true>, md_fanin_kernel<true>,       tests/multidist3d_dist_ref.py
                                                      st_dd_reduce_kernel

All three are formed from the cotangent st_det_kernel hands back, which depends on the loss (loss_term / loss_term_nz, LSQ or
Poisson with poisson_mult), the data convention, the detector mask (det_weight: dropped, not weighted) and the mode count (M == 1:
the guarded loss_term, M > 1: loss_term_nz).  The launch geometries are other matrices' business (st_matrix, count_matrix,
fan_matrix); here every shape is the smallest with more than one column group and a clipped last one, 24 x 20 (groups 8, 8, 4).

* ``OPTIONS``: the settings; ``ROWS``: every option x path x mode count exactly once, each with the detector and seed it runs at;
  ``FAR_ROWS``: a far-field magnitude does not see the exit-wave offsets; ``Z_ROWS``: the values of the sparse path's own
  parameter; ``ZERO_ROWS``: predictions of (numerically) zero under M = 2.
* ``build(name)``: the inputs of a row, computed once per process and left unchanged; ``ref(name, dtype)``: the extended
  restatement on them; ``yardstick(name)``: fp64, fp32 and the fp32 run's distances.
* the bars, each with its reason, are at the end.
tests/test_smallgrad_conditions.py holds the table to the pinned oracle, to finite differences and to its own rules on the CPU;
tests/test_gpu_smallgrad_options.py runs it on the engine.
"""
import functools

import numpy as np

from oracle import adorym_oracle as O
from tests import ms_matrix as MM
from tests import value_matrix as VM
from tests import fan_matrix as FM
from tests import sparse_ref as SR
from tests import prj_offset_ref as PR
from tests import multidist3d_ref as MR
from tests import multidist3d_dist_ref as DR
from tests import test_gpu_sparse_multislice as SP
from tests import test_gpu_prj_offset as PO

ENERGY_EV, PSIZE_CM = SP.ENERGY_EV, SP.PSIZE_CM
FIELD = FM.FIELD                        # 24 x 20
FRESNEL_CM = 2e-3                       # the sparse rows' Fresnel detector
# the exit-wave offsets are drawn within +-SHIFT_AMP px and the fan-out's distances are FAN_DISTS_CM (5 - 12 um, not aliased on
# this field): at the sibling modules' +-2 px and 1 - 3.5 um the float32 restatement's error on dL/ds and dL/dd is 2e-7 .. 5e-7,
# the rounding of a float32 output, and the rows would miss MIN_YARDSTICK (below)
SHIFT_AMP = 24.
FAN_DISTS_CM = (5e-4, 8e-4, 1.2e-3)
PATHS = ('sparse', 'exit_shift', 'fanout')
SMALL = {'sparse': 'gz', 'exit_shift': 'gs', 'fanout': 'gdists'}
rel = MM.rel

# ---------------------------------------------------------------------------------------------------------------- options
#   name: what differs from (LSQ, magnitude data, no mask, normalize_fft=False, delta_beta)
OPTIONS = {
    'lsq_intensity': dict(raw_data_type='intensity'),
    'poisson_magnitude': dict(loss='poisson', poisson_multiplier=50.),
    'poisson_intensity': dict(loss='poisson', poisson_multiplier=50., raw_data_type='intensity'),
    'beamstop': dict(beamstop=True),
    'beamstop_poisson': dict(beamstop=True, loss='poisson', poisson_multiplier=50.),
    'ortho': dict(normalize_fft=True),
    'real_imag_poisson': dict(unknown_type='real_imag', loss='poisson', poisson_multiplier=50.),
}
PLAIN = dict(loss='lsq', poisson_multiplier=1., raw_data_type='magnitude', beamstop=False, normalize_fft=False, unknown_type='delta_beta')
PATH_OPTIONS = {'sparse': tuple(OPTIONS), 'exit_shift': tuple(OPTIONS),
                'fanout': tuple(o for o in OPTIONS if o != 'real_imag_poisson')}       # (the fan-out engine is delta_beta only)
MODE_COUNTS = (1, 2)


def settings(option):
    out = dict(PLAIN)
    out.update(OPTIONS.get(option, {}))
    return out


def _row(path, option, M, det=None, seed=0, kind='reference', **kw):
    return '%s-%s-M%d' % (path, option, M), dict(path=path, option=option, M=M, det=det, seed=seed, kind=kind, kw=kw)


# kind 'reference': judged against the extended restatement; 'identity': the option cannot act on the path (normalize_fft in front
# of a Fresnel or exit-wave detector) and every output is bit-identical to the run without it.
# det: 'inf' (far field), a distance in cm (Fresnel), 0 (exit wave).  The seeds are chosen, from the restatement alone, so that
# every row's fp32 yardstick on the small gradient is at least MIN_YARDSTICK (test_smallgrad_conditions.py asserts it).
ROWS = dict([
    # ---- sparse multislice: probe 24 x 20, S = 3, B = 3
    _row('sparse', 'lsq_intensity', 1, det=FRESNEL_CM, seed=1),
    _row('sparse', 'lsq_intensity', 2, det='inf', seed=1),
    _row('sparse', 'poisson_magnitude', 1, det='inf'),
    _row('sparse', 'poisson_magnitude', 2, det=0),
    _row('sparse', 'poisson_intensity', 1, det=0),
    _row('sparse', 'poisson_intensity', 2, det='inf', seed=1),
    _row('sparse', 'beamstop', 1, det='inf'),
    _row('sparse', 'beamstop', 2, det=FRESNEL_CM, seed=1),
    _row('sparse', 'beamstop_poisson', 1, det=FRESNEL_CM),
    _row('sparse', 'beamstop_poisson', 2, det='inf'),
    _row('sparse', 'ortho', 1, det='inf'),                       # det_scale: normalize_fft acts on a far-field detector
    _row('sparse', 'ortho', 2, det='inf', seed=1),
    _row('sparse', 'real_imag_poisson', 1, det=0),
    _row('sparse', 'real_imag_poisson', 2, det='inf'),
    # ---- exit-wave offsets: 24 x 20, S = 2, B = 5 on the shared index [0, 1, 2, 1, 0]
    _row('exit_shift', 'lsq_intensity', 1, det=PO.FREE_PROP_CM),
    _row('exit_shift', 'lsq_intensity', 2, det=0),
    _row('exit_shift', 'poisson_magnitude', 1, det=0),
    _row('exit_shift', 'poisson_magnitude', 2, det=PO.FREE_PROP_CM),
    _row('exit_shift', 'poisson_intensity', 1, det=PO.FREE_PROP_CM),
    _row('exit_shift', 'poisson_intensity', 2, det=0, seed=1),
    _row('exit_shift', 'beamstop', 1, det=0),
    _row('exit_shift', 'beamstop', 2, det=PO.FREE_PROP_CM),
    _row('exit_shift', 'beamstop_poisson', 1, det=PO.FREE_PROP_CM),
    _row('exit_shift', 'beamstop_poisson', 2, det=0),
    _row('exit_shift', 'ortho', 1, det=PO.FREE_PROP_CM, kind='identity'),
    _row('exit_shift', 'ortho', 2, det=0, kind='identity'),
    _row('exit_shift', 'real_imag_poisson', 1, det=0, seed=2),
    _row('exit_shift', 'real_imag_poisson', 2, det=PO.FREE_PROP_CM),
    # ---- refined fan-out: fan_matrix.FIELD, S = 2, B = 3, D = 3
    _row('fanout', 'lsq_intensity', 1),
    _row('fanout', 'lsq_intensity', 2),
    _row('fanout', 'poisson_magnitude', 1),
    _row('fanout', 'poisson_magnitude', 2),
    _row('fanout', 'poisson_intensity', 1),
    _row('fanout', 'poisson_intensity', 2),
    _row('fanout', 'beamstop', 1),
    _row('fanout', 'beamstop', 2),
    _row('fanout', 'beamstop_poisson', 1),
    _row('fanout', 'beamstop_poisson', 2),
    _row('fanout', 'ortho', 1, kind='identity'),
    _row('fanout', 'ortho', 2, kind='identity'),
])
# the float32 restatement's own error on the small gradient of these rows, in the table's order (CPU; test_fp32_yardsticks asserts
# >= MIN_YARDSTICK and prints them):
#   sparse      1.8e-5 1.6e-5 | 8.5e-5 3.8e-6 | 6.1e-6 1.3e-5 | 5.7e-6 1.1e-5 | 2.9e-5 3.2e-6 | 1.9e-6 2.4e-6 | 1.5e-5 6.5e-6
#   exit shift  3.8e-6 1.6e-6 | 6.9e-6 2.4e-6 | 1.5e-5 2.5e-6 | 3.0e-6 2.1e-6 | 1.2e-5 1.6e-6 | (identity)     | 2.8e-6 1.6e-6
#   fan-out     4.5e-6 5.0e-6 | 7.9e-6 4.3e-6 | 7.9e-6 4.2e-6 | 4.0e-6 3.5e-6 | 4.7e-6 2.0e-6 | (identity)
# At seed 0 lsq_intensity in front of a far-field detector has 5.0e-7 (M = 2) and beamstop M = 2 behind the Fresnel detector 8.5e-7:
# those rows run at seed 1.  Prediction, loss, object and probe gradient: at most 0.30 of GENERIC's bars (the prediction of
# sparse-poisson_intensity-M1, 1.5e-6 of 5e-6).
# Finite differences (fp64, FD_STEP): plain rows 5.1e-7 / 1.7e-8 / 9.7e-9; option rows 2.4e-10 .. 1.3e-4, the worst
# sparse-poisson_intensity-M1 (an exit-wave detector) and sparse-poisson_magnitude-M1 (far field, 8.2e-5); the mutants lie
# 3.4e-2 (the mask ignored on the fan-out) .. 26 away.
# the plain LSQ row of every path: golden-tied, the finite-difference step is chosen on it (no GPU test of its own: the three
# sibling modules run it)
PLAIN_ROWS = dict([_row('sparse', 'plain', 1, det='inf', seed=1), _row('exit_shift', 'plain', 1, det=PO.FREE_PROP_CM), _row('fanout', 'plain', 1)])
# a far-field magnitude does not see the offsets: one row per loss, the gradient buffer comes back bit-unchanged
FAR_ROWS = dict([_row('exit_shift', 'far_lsq', 1, det='inf'), _row('exit_shift', 'far_poisson', 2, det='inf', option_of='poisson_magnitude')])

# ---------------------------------------------------------------------------------------------------------------- slice positions
# the sparse path's own parameter, S = 4, far field, M = 1, under LSQ and poisson_magnitude.  z in units of 2^-12 cm (2.44 um), so
# that z + 1 cm is exact in float32 and the moved run sees the same gaps bit for bit.
Z_UNIT = 2. ** -12
Z_BASE = (0, 2, 7, 11)
# LADDER: the gaps of Z_BASE times 10, 100, ...  The top rung is the largest at which the float32 restatement's own dL/dz error
# stays at or below LADDER_BAR (decided on the CPU; test_smallgrad_conditions.py asserts both that and that the next rung is
# above it).
LADDER_BAR = 1e-3
LADDER = {'plain': (10, 100, 1000), 'poisson_magnitude': (10,)}
# measured (float32 restatement, dL/dz):  LSQ      x10 2.8e-5, x100 2.8e-4, x1000 8.5e-4 (the top: gaps to 17 mm), x10000 2.7e-2
#                                         Poisson  x10 2.6e-5 (the top: gaps to 0.17 mm), x100 5.2e-3
# base 3.5e-6 / 5.9e-6, zero gap 9.2e-6 / 4.2e-6, negative gap 4.1e-6 / 1.1e-4.  On the ladder the restatement's prediction
# leaves GENERIC's bar as well (3.4e-6 at x10, 4.0e-4 at x1000): those rows are judged by the 3x rule against that yardstick.
Z_VALUES = {
    'base': [u * Z_UNIT for u in Z_BASE],
    'zero_gap': [u * Z_UNIT for u in (0, 2, 2, 7)],              # two slices at the same z
    'negative_gap': [u * Z_UNIT for u in (0, 7, 2, 11)],         # two slices swapped
    'moved_1cm': [1. + u * Z_UNIT for u in Z_BASE],              # bit-identical to 'base'
}
Z_VALUES.update({'gaps_x%d' % k: [u * k * Z_UNIT for u in Z_BASE] for k in (10, 100, 1000, 10000)})
Z_LOSSES = ('plain', 'poisson_magnitude')
Z_ROWS = dict(('sparse-z-%s-%s' % (v, o), dict(path='sparse', option=o, M=1, det='inf', seed=0, kind='reference', kw=dict(S=4, z=v)))
              for v in Z_VALUES for o in Z_LOSSES if not v.startswith('gaps_x') or int(v[6:]) in LADDER[o])
# one rung above the top (CPU only: it shows that the top rung is the top)
OVER_ROWS = dict(('sparse-z-gaps_x%d-%s' % (10 * LADDER[o][-1], o),
                  dict(path='sparse', option=o, M=1, det='inf', seed=0, kind='reference', kw=dict(S=4, z='gaps_x%d' % (10 * LADDER[o][-1]))))
                 for o in Z_LOSSES)

# ---------------------------------------------------------------------------------------------------------------- zero predictions
# M = 2, an exit-wave detector, both modes' probes exactly 0 outside a disc, nothing that moves the field sideways (slices at one
# depth; offsets of zero): behind the forward / inverse transform pair the prediction outside the disc is zero up to the
# transforms' rounding (1e-17 of the field in fp64, 1e-8 in fp32, and exactly 0 where the rounding cancels), and loss_term_nz
# divides by it.  'masked': those pixels are under the mask and every output is the restatement's; 'bare': no mask, recorded only.
ZERO_ROWS = dict([_row('sparse', 'zero_pred', 2, det=0, zero=True), _row('exit_shift', 'zero_pred', 2, det=0, zero=True, S=1)])

ALL_ROWS = dict(ROWS)
for _t in (PLAIN_ROWS, FAR_ROWS, Z_ROWS, OVER_ROWS, ZERO_ROWS):
    ALL_ROWS.update(_t)


# ---------------------------------------------------------------------------------------------------------------- builders
def disc(P=FIELD):
    Py, Px = P
    yy, xx = np.meshgrid(np.arange(Py) - Py / 2, np.arange(Px) - Px / 2, indexing='ij')
    return yy ** 2 + xx ** 2 < (min(Py, Px) / 3) ** 2


def _data(mag, st):
    """The magnitudes a builder made, as the data of the row's convention (float32) and as the engine's target: the magnitude
    under LSQ, the intensity under the Poisson loss (make_case of test_gpu_multidist3d.py)."""
    mag = np.asarray(mag, np.float64)
    meas = (mag ** 2 if st['raw_data_type'] == 'intensity' else mag).astype(np.float32)
    if st['loss'] == 'lsq':
        target = O.target_magnitude(meas, st['raw_data_type'])
    else:
        target = meas.astype(np.float64) ** 2 if st['raw_data_type'] == 'magnitude' else meas
    return meas, np.asarray(target, np.float32)


@functools.lru_cache(maxsize=None)
def build(name):
    """The inputs of a row: the case of the path's own module (make_case of test_gpu_sparse_multislice.py /
    test_gpu_prj_offset.py, fan_matrix.make_case) with the option's data, target and mask.  Computed once, left unchanged."""
    row = ALL_ROWS[name]
    st = settings(row['kw'].get('option_of', row['option']))
    path, M, kw = row['path'], row['M'], row['kw']
    if path == 'sparse':
        z = Z_VALUES[kw['z']] if 'z' in kw else None
        case = SP.make_case(FIELD, S=kw.get('S', 3), B=3, M=M, unknown_type=st['unknown_type'], free_prop=row['det'], seed=row['seed'], z=z)
        if kw.get('zero'):
            case['z'] = np.zeros_like(case['z'])
    elif path == 'exit_shift':
        case = PO.make_case(FIELD, S=kw.get('S', 2), B=5, M=M, shared=True, unknown_type=st['unknown_type'], free_prop=row['det'],
                            seed=row['seed'], shifts_fn=lambda n: np.random.default_rng([row['seed'], n]).uniform(-SHIFT_AMP, SHIFT_AMP, (n, 2)))
        if kw.get('zero'):
            case['shifts'] = np.zeros_like(case['shifts'])
    else:
        case = FM.make_case(B=3, D=3, M=M, dists=DR.round32(FAN_DISTS_CM), seed=row['seed'])
        case['dists'] = [float(d) for d in case['dists']]
        case['unknown_type'] = 'delta_beta'
    if kw.get('zero'):
        case['probes'] = (case['probes'] * disc()).astype(np.complex64)
    case['meas'], case['target'] = _data(case['meas'], st)
    if kw.get('z') == 'moved_1cm':          # (make_case scales z to make the data: the moved row takes the unmoved row's)
        base = build(name.replace('moved_1cm', 'base'))
        case['meas'], case['target'] = base['meas'], base['target']
    case['beamstop'] = VM.value_beamstop(FIELD) if st['beamstop'] else None
    case['loss'], case['poisson_multiplier'], case['raw_data_type'] = st['loss'], st['poisson_multiplier'], st['raw_data_type']
    case['normalize_fft'] = st['normalize_fft']
    case['row'], case['name'] = row, name
    return case


def with_mask(case, beamstop):
    out = dict(case)
    out['beamstop'] = beamstop
    return out


def zero_mask():
    """ZERO_ROWS' mask: every pixel outside the probes' disc dropped."""
    return np.where(disc(), 1., 0.)


def dirtied(case, roll):
    """``case`` with NaN, +inf, -1, 0 and 3e38 in the data and the target under its mask (value_matrix.dirty; ``roll`` moves the
    mix along)."""
    out = dict(case)
    drop = np.asarray(case['beamstop']) < 1e-5
    n = int(drop.sum())
    for k in ('meas', 'target'):
        a = np.array(case[k], np.float32)
        for b in range(len(a)):
            a[b][drop] = np.resize(np.roll(VM.DIRT, b + roll), n)
        out[k] = a
    return out


# ---------------------------------------------------------------------------------------------------------------- the restatements
def loss_kw(case, **over):
    kw = dict(raw_data_type=case['raw_data_type'], loss_function_type=case['loss'], poisson_multiplier=case['poisson_multiplier'],
              beamstop=case['beamstop'])
    kw.update(over)
    return kw


def physics(case, normalize_fft=None):
    nf = case['normalize_fft'] if normalize_fft is None else normalize_fft
    path = case['row']['path']
    if path == 'fanout':
        return O.Physics(FIELD, ENERGY_EV, PSIZE_CM, free_prop_cm=case['dists'][0], sign_convention=case['sign_convention'], normalize_fft=nf)
    return O.Physics(FIELD, ENERGY_EV, PSIZE_CM, free_prop_cm=case['free_prop'], sign_convention=case['sign_convention'],
                     unknown_type=case['unknown_type'], normalize_fft=nf)


def small_of(case):
    """The path's small parameter as the restatement takes it (fp64)."""
    path = case['row']['path']
    return np.asarray(case[{'sparse': 'z', 'exit_shift': 'shifts', 'fanout': 'dists'}[path]], np.float64)


def ref(case, dtype='float64', small=None, normalize_fft=None, **over):
    """The extended restatement on ``case``: loss, pred, grad (object), gprobe and 'small' (dL/dz [S], dL/ds [n, 2], dL/dd [D]).
    ``small``: the parameter in place of the case's; ``over``: loss arguments in place of the case's (the mutants)."""
    path = case['row']['path']
    phys = physics(case, normalize_fft)
    x = small_of(case) if small is None else np.asarray(small, np.float64)
    obj, probes = case['obj'].astype(np.float64), case['probes'].astype(np.complex128)
    kw = loss_kw(case, **over)
    if path == 'sparse':
        l, p, g, gp, gx = SR.forward_adjoint_object(obj, None, probes, case['pos'], case['meas'], phys, x, dtype, **kw)
    elif path == 'exit_shift':
        l, p, g, gp, gx = PR.forward_adjoint_object(obj, None, probes, case['pos'], case['meas'], phys, x, case['index'], dtype, **kw)
    else:
        l, p, g, gp = MR.forward_adjoint_object(obj, None, probes, case['pos'], case['meas'], phys, x, dtype, **kw)
        l2, p2, gx, _ = DR.forward_dist_grad_object(obj, None, probes, case['pos'], case['meas'], phys, x, dtype, **kw)
        if np.dtype(dtype) == np.float64 and np.array_equal(x, DR.round32(x)):
            assert rel(p2, p) < 1e-12 and abs(l2 / l - 1) < 1e-12         # one model, stated twice
    return dict(loss=l, pred=p, grad=g, gprobe=gp, small=np.asarray(gx, np.float64))


def loss_at(case, small):
    """The fp64 restatement's loss with the small parameter at ``small`` (the finite differences).  The fan-out's own restatement
    rounds its distances to float32, so the multi-distance restatement underneath, which does not, serves there."""
    path = case['row']['path']
    phys = physics(case)
    obj, probes = case['obj'].astype(np.float64), case['probes'].astype(np.complex128)
    tiles, _ = O.extract_tiles(obj, case['pos'], FIELD, case['unknown_type'])
    kw = loss_kw(case)
    if path == 'sparse':
        return SR.forward_adjoint_tiles(tiles, probes, case['meas'], phys, small, want_grad=False, **kw)[0]
    if path == 'exit_shift':
        return PR.forward_adjoint_tiles(tiles, probes, case['meas'], phys, small, case['index'], **kw)[0]
    return MR.forward_adjoint_tiles(tiles, probes, case['meas'], phys, small, **kw)[0]


def central_differences(case, h):
    x0 = small_of(case)
    out = np.zeros(x0.shape)
    for i in np.ndindex(x0.shape):
        xp, xm = x0.copy(), x0.copy()
        xp[i] += h
        xm[i] -= h
        out[i] = (loss_at(case, xp) - loss_at(case, xm)) / (2 * h)
    return out


def mutants(case):
    """The mistakes a row guards against, as loss arguments of ``ref``: the mask ignored, the LSQ cotangent under the Poisson loss,
    intensity data read as magnitudes, the far-field scale of normalize_fft left out."""
    st = settings(case['row']['kw'].get('option_of', case['row']['option']))
    out = {}
    if st['beamstop']:
        out['mask_ignored'] = dict(beamstop=None)
    if st['loss'] == 'poisson':
        out['lsq_cotangent'] = dict(loss_function_type='lsq')
    if st['raw_data_type'] == 'intensity' and st['loss'] == 'lsq':
        out['data_as_magnitude'] = dict(raw_data_type='magnitude')
    if st['normalize_fft'] and case['row']['kind'] == 'reference':
        out['scale_left_out'] = dict(normalize_fft=False)
    return out


@functools.lru_cache(maxsize=None)
def yardstick(name):
    """The restatement in fp64 and in fp32 on a row, and the fp32 run's distances: pred, loss, grad, gprobe, small, then gprobe
    per mode (the layout of the fixtures' err32)."""
    case = build(name)
    r64, r32 = ref(case, 'float64'), ref(case, 'float32')
    e32 = [rel(r32['pred'], r64['pred']), abs(r32['loss'] / r64['loss'] - 1), rel(r32['grad'], r64['grad']), rel(r32['gprobe'], r64['gprobe']),
           rel(r32['small'], r64['small'])] + [rel(r32['gprobe'][m], r64['gprobe'][m]) for m in range(len(r64['gprobe']))]
    return r64, r32, e32


# ---------------------------------------------------------------------------------------------------------------- the engine
def engine_kw(case):
    """The engine keywords an option adds (run_sparse and run_shifted take them as **engine_kw; the fan-out's _engine reads loss,
    multiplier and mask from the case and takes the rest)."""
    kw = dict(normalize_fft=case['normalize_fft'])
    if case['row']['path'] != 'fanout':
        kw.update(loss_function_type=case['loss'], poisson_multiplier=case['poisson_multiplier'], beamstop=case['beamstop'])
    return kw


def engine_case(case):
    """``case`` as the path's runner reads it: run_sparse and run_shifted hand case['meas'] to set_batch, which takes the target."""
    out = dict(case)
    if case['row']['path'] != 'fanout':
        out['meas'] = case['target']
    return out


# ---------------------------------------------------------------------------------------------------------------- bars
# finite differences (fp64, central, of the restatement's own loss; step per path, chosen on the plain LSQ row)
FD_STEP = {'sparse': 1e-7, 'exit_shift': 1e-5, 'fanout': 1e-8}        # cm, pixels, cm
FD_PLAIN = 1e-4         # the plain row, which the goldens tie to the reference: of the gradient's norm
FD_OPTION = 1e-3        # every option row at the same step
FD_MUTANT = 10 * FD_OPTION          # a mutant's derivative is at least this far from the finite differences
# the neutral parameters: two float64 restatements of the same formulas
NEUTRAL = 1e-12
# the fp32 restatement on every row: a third of GENERIC's bars for what has them, so that the 3x rule's band stays inside them ...
YARD_FRACTION = 1. / 3
# ... and at least this on the small gradient: it comes back as float32, whose own resolution is 6e-8 .. 1.2e-7; below 1e-6 a row
# would measure the rounding of the output, not the kernel (the rule of test_gpu_sparse_multislice.py).  Held by ROWS and Z_ROWS.
# ZERO_ROWS cannot be: their parameters are pinned (slices at one depth, offsets of zero -- anything else moves the field out of
# the disc), and the offsets' row has 2.4e-7; it is judged by gs_bar, whose floor is the resolution of the float32 buffer.
MIN_YARDSTICK = 1e-6
