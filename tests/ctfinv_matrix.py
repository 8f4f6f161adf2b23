"""Tables, mirrors and references of the CTF inversion matrix (tests/test_gpu_ctfinv.py, tests/test_gpu_ctfinv_driver.py; importable
without a GPU).

adm_ctf_invert.hip compiles its three line kernels for the eight line lengths of ADM_LINE_SIZES; the length that instantiates
a kernel is the field's nx (rows: I1, I3) or its ny (lines kx: I2).  ``geometry`` restates the launch arithmetic (LineGeo,
blocks_for, I1's jobs (b, d, y), I2's grid (kx blocks, b), I3's jobs (b, y), the rounds of CTFInversion.retrieve), ``KERNELS`` and
``ENTRY_POINTS`` name every kernel family and entry point with the tests that run it, ``CASES`` the launches that put every length
in both roles and reach every class of ``ALL_CLASSES``.  tests/test_ctfinv_coverage.py ties all of it to the kernel source.

The reference is tests/ctfinv_ref.py in fp64 (held to golden F31 by tests/test_ctfinv_ref_vs_golden.py), the yardstick of the 3x
rule the same restatement in float32.  The holograms are ctf_matrix.inputs' (float32: the reference and the kernels see the same
numbers).  The line geometry, the band judgement and the bit helpers are those of tests/holo_matrix.py."""
import numpy as np

from tests import ctf_matrix as CM
from tests import ctfinv_ref as IR
from tests.golden import cases
from tests.holo_matrix import (line_geo, pow2_in_range, _blocks, rel, band_errors, check_bands, spectrum2, sentinel, bits,  # noqa: F401
                               SIZES, MAX_DISTS)
from tests.ctf_matrix import ENERGY_EV, PSIZE_CM, LG_KAPPA, FIELDS, PHASE_FIELD, PHASE_RUNGS  # noqa: F401

# The bars.  None is tuned against a GPU: each is 3 x the largest distance of the committed float32 restatement from fp64, computed
# on the CPU over the table (python -m tests.ctfinv_matrix prints the figures) and written here once.
ERR32 = 7.5e-6              # phase, relative, whole array: the largest of CASES is 7.1e-6, at (64, 512, 2)
BAR = 3 * ERR32
# The value rungs scale xi, and fl32(c_d (u^2 + v^2)) -- the product the reference's float32 tensors and the kernel both form --
# is off by up to xi 2^-24 rad: the inversion divides by w_d, so the float32 restatement's own error grows with the rung (4.7e-6,
# 1.8e-5, 8.5e-5 at 100, 1000, 3000 rad).  Each rung is held to 3 x the restatement's error AT that rung; the pure-phase case
# (2.4e-6) to the table's bar.
VALUE_ERR32 = {'phase_100_rad': ERR32, 'phase_1000_rad': 1.8e-5, 'phase_3000_rad': 8.5e-5, 'pure_phase': ERR32}
# retrieve(affine=identity) against retrieve(): the reference's own identity resample in float32 moves its phase by up to 3.15e-6
# (golden F31, '<case>/identity'[1], at 64 x 32 x 3; in fp64 by 1e-15)
IDENTITY_ERR32 = 3.15e-6
IDENTITY_BAR = 3 * IDENTITY_ERR32
# the driver run (DRV below): ctfinv_ref.drive in float32 against fp64 -- lg_kappa after every update (absolute) and the final
# delta (relative): 6.4e-6 and 1.6e-6; the losses of at least LOSS_FLOOR (relative; from the second on they are 1e-8, sums of squared
# residuals of 1e-4 that carry float32's 6e-8 of a prediction near 1): 1.4e-4.  Losses below LOSS_FLOOR are rounding and not judged.
DRV = dict(field=(16, 16, 3), n_epochs=10, learning_rate=1e-3, ctf_lg_kappa_learning_rate=2e-2)
DRV_ERR32 = dict(trace=6.5e-6, delta=1.7e-6, loss=1.45e-4)
LOSS_FLOOR = 1e-9
DRV_BARS = {k: 3 * v for k, v in DRV_ERR32.items()}
PURE_PHASE_LG_KAPPA = 30.


# ------------------------------------------------------------------------------------------------------------ launch geometry
def geometry(ny, nx, nd, nb=1):
    """One adm_ctfinv_run of nb angles."""
    gx, gy = line_geo(nx), line_geo(ny)
    i1 = _blocks(nb * nd * ny, gx['LPB'])
    return dict(gx=gx, gy=gy,
                i1_blocks=i1,                                                                   # I1: jobs b * nd * ny + d * ny + y
                i1_spans_dists=[lo // ny != (hi - 1) // ny for lo, hi in i1],
                i1_spans_batch=[lo // (nd * ny) != (hi - 1) // (nd * ny) for lo, hi in i1],
                col_blocks=_blocks(nx, gy['LPB']), i2_grid=(len(_blocks(nx, gy['LPB'])), nb),     # I2: lines kx, one b per blockIdx.y
                i3_blocks=_blocks(nb * ny, gx['LPB']))                                          # I3: jobs b * ny + y


def rounds(n_batch, max_batch):
    """The launches of CTFInversion.retrieve: (first angle, angles) per round."""
    return [(b0, min(max_batch, n_batch - b0)) for b0 in range(0, n_batch, max_batch)]


ALL_CLASSES = ('partial_block', 'i1_block_spans_distances', 'i1_block_spans_batch', 'nd_1', 'nd_odd', 'nd_64', 'twiddles_global',
               'tpr_gt_64', 'tpr_le_64', 'tall', 'wide', 'batch_1', 'batch_3', 'one_round', 'several_rounds', 'ragged_last_round',
               'spare_batch_capacity', 'out_stride_1', 'out_stride_2', 'alpha_default', 'alpha_constant', 'alpha_table')


def classes(ny, nx, nd, nb=1, max_batch=1, out_stride=1, alpha=None):
    c = set()
    rs = rounds(nb, max_batch)
    for _, n in rs:
        g = geometry(ny, nx, nd, n)
        for blocks, lpb in ((g['i1_blocks'], g['gx']['LPB']), (g['i3_blocks'], g['gx']['LPB']), (g['col_blocks'], g['gy']['LPB'])):
            if any(hi - lo < lpb for lo, hi in blocks):
                c.add('partial_block')
        if any(g['i1_spans_dists']):
            c.add('i1_block_spans_distances')
        if any(g['i1_spans_batch']):
            c.add('i1_block_spans_batch')
    c.add('one_round' if len(rs) == 1 else 'several_rounds')
    if len(rs) > 1 and rs[-1][1] < max_batch:
        c.add('ragged_last_round')
    if nb < max_batch:
        c.add('spare_batch_capacity')
    if nb in (1, 3):
        c.add('batch_%d' % nb)
    if nd == 1:
        c.add('nd_1')
    if nd % 2 == 1 and nd > 1:
        c.add('nd_odd')
    if nd == MAX_DISTS:
        c.add('nd_64')
    g = geometry(ny, nx, nd)
    for geo in (g['gx'], g['gy']):
        c.add('tpr_gt_64' if geo['TPR'] > 64 else 'tpr_le_64')
        if not geo['tw_lds']:
            c.add('twiddles_global')
    if ny > nx:
        c.add('tall')
    if nx > ny:
        c.add('wide')
    c.add('out_stride_%d' % out_stride)
    c.add('alpha_default' if alpha is None else 'alpha_' + alpha)
    return c


# ------------------------------------------------------------------------------------------------------------ tables
# name -> keywords of ``case``.  Every field of ctf_matrix.FIELDS alone (B = 1, max_batch = 1, the default alpha), then what the
# batch, the output stride and the regulariser add, on the smallest fields that reach it.
CASES = {'%dx%dx%d' % f: dict(field=f) for f in FIELDS}
CASES.update({
    '16x16x3_B3': dict(field=(16, 16, 3), nb=3, max_batch=3),               # 144 I1 jobs in blocks of 128: a block over two batch entries
    '16x16x3_B3_rounds_of_2': dict(field=(16, 16, 3), nb=3, max_batch=2),   # two rounds, the last ragged
    '16x16x3_B1_capacity_2': dict(field=(16, 16, 3), nb=1, max_batch=2),
    '64x32x3_B3_rounds_of_2': dict(field=(64, 32, 3), nb=3, max_batch=2),   # several blocks per batch entry in every kernel
    '32x16x2_into_object': dict(field=(32, 16, 2), out_stride=2),
    '16x32x2_into_object': dict(field=(16, 32, 2), out_stride=2),
    '32x16x2_alpha_constant': dict(field=(32, 16, 2), alpha='constant'),
    '32x16x2_alpha_table': dict(field=(32, 16, 2), alpha='table'),
    '16x32x2_alpha_table': dict(field=(16, 32, 2), alpha='table'),
    '64x32x3_alpha_table_B3': dict(field=(64, 32, 3), alpha='table', nb=3, max_batch=3),
})
# the value axis, on PHASE_FIELD: xi scaled to the rungs of ctf_matrix (sincos_fast's argument), and the pure-phase kappa
VALUE_CASES = {'phase_%g_rad' % p: dict(field=PHASE_FIELD, phase=p) for p in PHASE_RUNGS}
VALUE_CASES['pure_phase'] = dict(field=PHASE_FIELD, lg_kappa=PURE_PHASE_LG_KAPPA)

_ALL = ('test_cases', 'test_value_classes')
KERNELS = {
    'ctfinv_i1<N>': ('nx', _ALL),
    'ctfinv_i2<N>': ('ny', _ALL),
    'ctfinv_i3<N>': ('nx', _ALL),
}
ENTRY_POINTS = {
    'adm_ctfinv_create': ('test_cases', 'test_create_refusals'),
    'adm_ctfinv_destroy': ('test_cases', 'test_one_handle_many_launches'),
    'adm_ctfinv_run': _ALL + ('test_run_refusals', 'test_two_calls_give_identical_bits'),
}


def reached():
    """{(family, N)} the table launches."""
    out = set()
    for k, (axis, _) in KERNELS.items():
        for kw in CASES.values():
            ny, nx, _nd = kw['field']
            out.add((k, {'nx': nx, 'ny': ny}[axis]))
    return out


# ------------------------------------------------------------------------------------------------------------ inputs
def alpha_of(kind, ny, nx):
    """None: the reference's 1e-10.  'constant': 1e-3.  'table': a value per bin [ky, kx] that differs in every bin and is not
    symmetric in (ky, kx), of the size of the denominator at low frequencies (2 / kappa^2 = 8e-4): a transposed table is wrong by
    up to a factor of two in alpha, far above the bar."""
    if kind is None:
        return None
    if kind == 'constant':
        return np.float32(1e-3)
    return (1e-3 * (1. + np.arange(ny * nx).reshape(ny, nx) / float(ny * nx))).astype(np.float32)


def inputs(field, nb=1, max_batch=1, out_stride=1, alpha=None, phase=None, lg_kappa=LG_KAPPA):
    """data [nb, nd, ny, nx] float32: the holograms of ctf_matrix.inputs for nb objects (seeds apart), dists, lg_kappa, alpha."""
    ny, nx, nd = field
    base = 2600 + 31 * ny + 7 * nx + nd
    cs = [CM.inputs(ny, nx, nd, seed=base + 211 * b, phase=phase) for b in range(nb)]
    return dict(ny=ny, nx=nx, nd=nd, nb=nb, max_batch=max_batch, out_stride=out_stride, alpha_kind=alpha, alpha=alpha_of(alpha, ny, nx),
                data=np.stack([c['data'] for c in cs]), dists=cs[0]['dists'], lg_kappa=np.float32(lg_kappa))


def ref_run(c, dtype='float64'):
    return IR.retrieve(c['data'], c['dists'], c['lg_kappa'], ENERGY_EV, PSIZE_CM, alpha=c['alpha'], dtype=dtype)


_CASES = {}


def case(name):
    """Inputs and the reference pair (o64, o32) of a row of CASES or VALUE_CASES, built once per process."""
    if name not in _CASES:
        c = inputs(**(CASES[name] if name in CASES else VALUE_CASES[name]))
        c['name'], c['bar'] = name, 3 * VALUE_ERR32.get(name, ERR32)
        c['o64'], c['o32'] = ref_run(c, 'float64'), ref_run(c, 'float32')
        _CASES[name] = c
    return _CASES[name]


# ------------------------------------------------------------------------------------------------------------ judgement
def band_defs(c):
    """name -> (bands, axis) of what the GPU module judges band by band, per angle: the rows of every I3 block of the phase map and
    the kx lines of its spectrum per I2 block.  (An I3 block of a small field holds several angles' rows: the bands are then cut
    from the angles stacked along y, jobs b * ny + y.)"""
    g = geometry(c['ny'], c['nx'], c['nd'], c['nb'])
    return {'phase rows': (g['i3_blocks'], 0), 'spectrum kx blocks': (g['col_blocks'], 1)}


def band_views(c, phase):
    """The arrays band_defs' bands cut, of phase maps [nb, ny, nx]."""
    p = np.asarray(phase, np.float64).reshape(c['nb'], c['ny'], c['nx'])
    return {'phase rows': p.reshape(c['nb'] * c['ny'], c['nx']), 'spectrum kx blocks': spectrum2(p)}


def conditions(c):
    """What the reference pair alone decides, without a GPU: the float32 restatement within a third of the bar, and no band
    without signal.  Asserts; returns the figures as a line of text."""
    e = rel(c['o32'], c['o64'])
    assert e <= c['bar'] / 3, (c['name'], e)
    assert np.isfinite(c['o64']).all() and np.abs(c['o64']).max() > 1e-3, c['name']
    o, s = band_views(c, c['o64']), band_views(c, c['o32'])
    worst = {}
    for name, (bands, axis) in band_defs(c).items():
        e_, _, judged = band_errors(s[name], o[name], s[name], bands, axis)
        assert judged.all(), (c['name'], name, 'bands without signal', int((~judged).sum()), len(judged))
        worst[name] = float(e_.max())
    return 'fp32 restatement %.1e (bar %.1e);  its worst band: %s' % (e, c['bar'],'  '.join('%s %.1e' % kv for kv in worst.items()))


# ------------------------------------------------------------------------------------------------------------ the driver run
def drv_inputs():
    ny, nx, nd = DRV['field']
    return CM.inputs(ny, nx, nd)


_DRV = {}


def drv_ref(dtype='float64'):
    if dtype not in _DRV:
        c = drv_inputs()
        kw = {k: v for k, v in DRV.items() if k != 'field'}
        _DRV[dtype] = IR.drive(c['data'], c['obj'][..., 0], c['obj'][..., 1], c['dists'], LG_KAPPA, ENERGY_EV, PSIZE_CM, dtype=dtype, **kw)
    return _DRV[dtype]


def drv_errors(trace, delta, losses):
    """The distances of a run from drive() in fp64: lg_kappa after every update (absolute), the final delta (relative), the losses
    of at least LOSS_FLOOR (relative)."""
    a = drv_ref('float64')
    la, l = np.array(a['losses']), np.asarray(losses, np.float64)
    assert l.shape == la.shape and (la >= LOSS_FLOOR).sum() >= 2
    return dict(trace=float(np.abs(np.array(a['lg_kappa_trace']) - np.asarray(trace, np.float64)).max()),
                delta=rel(np.asarray(delta, np.float64).reshape(a['obj'].shape[:2]), a['obj'][..., 0]),
                loss=float(np.abs(l / la - 1)[la >= LOSS_FLOOR].max()))


def drv_conditions():
    a, b = drv_ref('float64'), drv_ref('float32')
    e = drv_errors(b['lg_kappa_trace'], b['obj'][..., 0], b['losses'])
    for k, v in e.items():
        assert v <= DRV_BARS[k] / 3, (k, v)
    # the run does something: kappa moves by far more than the bar, the loss falls by four orders after the first inversion
    assert abs(a['lg_kappa_trace'][-1] - LG_KAPPA) > 1e3 * DRV_BARS['trace'] and a['losses'][1] < 1e-3 * a['losses'][0]
    return 'fp32 restatement: lg_kappa trace %.1e  final delta %.1e;  lg_kappa %.4f -> %.4f' % (e['trace'], e['delta'], LG_KAPPA, a['lg_kappa_trace'][-1])


if __name__ == '__main__':
    for n in list(CASES) + list(VALUE_CASES):
        print(n, conditions(case(n)))
    print('driver', drv_conditions())
