"""Tables, mirrors and references of the CTF matrix (tests/test_gpu_ctf.py; importable without a GPU).

adm_holo_ctf.hip compiles every line kernel for the eight line lengths of ADM_LINE_SIZES; the length that instantiates a kernel is
the field's nx (rows: C1, C3, C5) or its ny (lines kx: C2, C4).  ``geometry`` restates the launch arithmetic (LineGeo, blocks_for,
C3's jobs, C4's rounds, the outputs of ctf_sum_one), ``KERNELS`` and ``ENTRY_POINTS`` name every kernel family and entry point
with the tests that run it, ``FIELDS`` the fields that put every length in both roles and reach every class of ``ALL_CLASSES``.
tests/test_ctf_coverage.py ties all of it to the kernel source.

The reference is tests/ctf_ref.py in fp64 (held to golden F26 by tests/test_ctf_ref_vs_golden.py), the yardstick of the 3x rule
the same restatement in float32.  Every input is rounded to float32 first: the reference and the kernels see the same numbers.
The line geometry, the band judgement and the bit helpers are those of tests/holo_matrix.py (the kernels share that skeleton)."""
import numpy as np

from tests import ctf_ref as R
from tests.golden import cases
from tests.holo_matrix import (line_geo, pow2_in_range, _blocks, rel, band_errors, check_bands, spectrum2, sentinel, bits,  # noqa: F401
                               SIZES, MAX_DISTS, MAX_UNJUDGED)

ENERGY_EV, PSIZE_CM = 17050., 1e-4          # golden cases' C5MINI: xi reaches 46 rad at 40 cm and 103 rad at 90 cm
LG_KAPPA, LG_KAPPA_TRUTH = 1.7, 1.5
MIN_I = 0.05                                # every case compared with a reference keeps min I_d >= MIN_I
CLIP_I = -0.05                              # ... the clipped case: I_d <= CLIP_I or I_d >= MIN_I, nothing in between

# whole-array bars: the holography path's (tests/holo_matrix.py BARS); gkappa: max(bar, 3 x fp32 reference)
BARS = dict(loss=5e-5, pred=5e-6, grad=2e-4, gkappa=2e-3)


# ------------------------------------------------------------------------------------------------------------ launch geometry
def geometry(ny, nx, nd):
    gx, gy = line_geo(nx), line_geo(ny)
    jobs = _blocks(nd * ny, gx['LPB'])
    row_blocks = _blocks(ny, gx['LPB'])
    return dict(gx=gx, gy=gy,
                row_blocks=row_blocks,                                  # C1 / C5: rows y
                c3_blocks=jobs,                                         # C3: jobs d * ny + y
                c3_spans=[lo // ny != (hi - 1) // ny for lo, hi in jobs],
                col_blocks=_blocks(nx, gy['LPB']),                      # C2: lines kx
                c4_rounds=-(-nd // gy['LPB']), c4_ragged=nd % gy['LPB'] != 0,     # C4: one block per kx, LPB(ny) distances per round
                n_sums=nd + 1,                                          # ctf_sum_one outputs (nd losses, the kappa gradient) ...
                sums_per_block=-(-(nd + 1) // len(row_blocks)))         # ... spread over C5's blocks


ALL_CLASSES = ('partial_block', 'c3_block_spans_distances', 'c4_one_round', 'c4_several_rounds', 'c4_ragged_last_round',
               'c4_one_slot', 'c4_idle_slots', 'nd_1', 'nd_odd', 'nd_64', 'twiddles_global', 'tpr_gt_64', 'tpr_le_64',
               'tall', 'wide', 'several_sums_per_block')


def classes(ny, nx, nd):
    g = geometry(ny, nx, nd)
    c = set()
    for blocks, lpb in ((g['row_blocks'], g['gx']['LPB']), (g['c3_blocks'], g['gx']['LPB']), (g['col_blocks'], g['gy']['LPB'])):
        if any(hi - lo < lpb for lo, hi in blocks):
            c.add('partial_block')
    if any(g['c3_spans']):
        c.add('c3_block_spans_distances')
    c.add('c4_one_round' if g['c4_rounds'] == 1 else 'c4_several_rounds')
    if g['c4_rounds'] > 1 and g['c4_ragged']:
        c.add('c4_ragged_last_round')
    if g['gy']['LPB'] == 1:
        c.add('c4_one_slot')
    if g['gy']['LPB'] > nd:
        c.add('c4_idle_slots')
    if nd == 1:
        c.add('nd_1')
    if nd % 2 == 1 and nd > 1:
        c.add('nd_odd')
    if nd == MAX_DISTS:
        c.add('nd_64')
    for geo in (g['gx'], g['gy']):
        c.add('tpr_gt_64' if geo['TPR'] > 64 else 'tpr_le_64')
        if not geo['tw_lds']:
            c.add('twiddles_global')
    if ny > nx:
        c.add('tall')
    if nx > ny:
        c.add('wide')
    if g['sums_per_block'] > 1:
        c.add('several_sums_per_block')
    return c


# ------------------------------------------------------------------------------------------------------------ tables
# (ny, nx): n_dists.  At most 32 768 pixels per field; every length in both roles.
GOLDEN_FIELDS = {(16, 16, 1): 'intensity', (16, 16, 3): 'intensity', (32, 16, 2): 'intensity', (16, 32, 2): 'intensity',
                 (64, 32, 3): 'intensity', (16, 16, 2): 'magnitude'}
FIELDS = (
    (16, 16, 1),                          # 16 lines in a block of 128
    (16, 16, 3),                          # 48 C3 jobs in one block: three distances side by side
    (32, 16, 2), (16, 32, 2),
    (64, 32, 3),                          # 192 jobs in blocks of 64
    (64, 512, 2), (512, 64, 3),           # LPB(512) = 4
    (2048, 16, 3), (16, 2048, 2),         # lines of four waves, twiddles from global memory, one C4 slot
    (1024, 16, 3), (32, 1024, 5),         # LPB(1024) = 2: C4 in two rounds, the second ragged (ny = 1024); the largest LDS twiddle copy
    (256, 128, 2), (128, 256, 4),
    (256, 16, 64),                        # the most distances: C4 in 8 rounds, 65 sums over 2 C5 blocks
)
VARIANT_FIELD = (128, 256, 4)
# the value axis of ctf_sincos (sincos_fast, as holo_h): the rungs of tests/holo_value_matrix.py, whose top rung (PHASE_MAX) is the largest
# of its ladder at which the float32 restatement keeps within a third of every bar -- here too (at 1e4 rad it does not: pred 2.1e-6,
# grad 1.3e-4).  At the table's own distances xi reaches 103 rad.
PHASE_FIELD = (32, 16, 2)
PHASE_RUNGS = (100., 1000., 3000.)


_GRAD = ('test_fields_gradient_launch', 'test_variants', 'test_clip')
_FWD = ('test_fields_forward_only', 'test_variants')
KERNELS = {
    'ctf_c1<N>': ('nx', _GRAD + _FWD),
    'ctf_c2<N>': ('ny', _GRAD + _FWD),
    'ctf_c3<N, true>': ('nx', _GRAD),
    'ctf_c3<N, false>': ('nx', _FWD),
    'ctf_c4<N>': ('ny', _GRAD),
    'ctf_c5<N>': ('nx', _GRAD),
    'ctf_sums_kernel': (None, _FWD),
}
ENTRY_POINTS = {
    'adm_ctf_create': ('test_fields_gradient_launch', 'test_create_refusals'),
    'adm_ctf_destroy': ('test_fields_gradient_launch', 'test_one_handle_many_launches'),
    'adm_ctf_fwd_adj': _GRAD + _FWD,
}


def reached():
    """{(family, N)} the table launches."""
    out = set()
    for k, (axis, _) in KERNELS.items():
        for ny, nx, _nd in FIELDS:
            out.add((k, {'nx': nx, 'ny': ny, None: 0}[axis]))
    return out


# name -> launch keywords
VARIANTS = {
    'overwrite': dict(overwrite=True),
    'accumulate': dict(seed='seeded'),
    'overwrite_sentinel': dict(seed='sentinel', overwrite=True),
    'accumulate_sentinel_beta': dict(seed='sentinel'),
    'forward_only': dict(want_grad=False, seed='sentinel'),
    'forward_only_null_gradients': dict(want_grad=False, want_obj=False, want_kappa=False),      # grad_obj = grad_lg_kappa = NULL
    'no_pred': dict(want_pred=False),
    'no_grad_lg_kappa': dict(want_kappa=False),
    'no_loss': dict(want_loss=False),
    'magnitude': dict(raw='magnitude'),
}


# ------------------------------------------------------------------------------------------------------------ inputs
def window(ny, nx):
    """The vignette the model needs (adorym/propagate.py:592-595): a raised cosine over the outer eighth of either side."""
    def w1(n):
        e = max(n // 8, 1)
        w = np.ones(n)
        ramp = 0.5 - 0.5 * np.cos(np.pi * (np.arange(e) + 0.5) / e)
        w[:e], w[n - e:] = ramp, ramp[::-1]
        return w
    return w1(ny)[:, None] * w1(nx)[None, :]


def delta_map(ny, nx, seed, scale=1.):
    """A windowed random map of a few 1e-2: a smooth part and half of it in white noise.  The prediction is 1 + O(1e-2), so a float32
    run carries an absolute error of 3e-8 into EVERY line of its two-dimensional spectrum: the noise keeps enough signal on the
    lines far from the smooth part for the float32 reference to stay within 3.3e-6 on each (with a tenth in noise: 7.5e-6, a band
    bar of 2.75e-5, under which osc x 1.00005 in one kx block of C2 -- 2.5e-5 on its line and the mirrored one -- passes)."""
    r = cases.rng(seed)
    return scale * window(ny, nx) * (3e-2 * (cases.smooth_field((ny, nx), seed + 1) - 0.5) + 1.5e-2 * r.standard_normal((ny, nx)))


def dists_for(nd):
    return 40. + 50. * np.arange(nd) / max(nd - 1, 1)                  # cm; (40, 65, 90) at nd = 3


def max_xi(ny, nx, dists):
    """The largest argument ctf_sincos sees: PI lambda d_nm (u^2 + v^2) at Nyquist of both axes and the largest distance."""
    return float(R.PI * (1240. / ENERGY_EV) * np.max(dists) * 1e7 * R.uv2((ny, nx), PSIZE_CM).max())


def inputs(ny, nx, nd, raw='intensity', clip=False, seed=None, phase=None):
    """Host inputs of one case: obj [ny, nx, 2] float32 (beta non-zero: the model must ignore it), data [nd, ny, nx] float32 -- the
    fp64 model of a second object at lg_kappa = 1.5 -- dists [nd] float64, lg_kappa float32.  ``clip``: a tone of a quarter of the
    sampling frequency along both axes, un-windowed (one bin of the spectrum: A_d scales it by osc_d), strong enough to take a
    quarter of the pixels of at least one distance below zero.  ``phase``: the distances scaled so that the largest argument of
    ctf_sincos (``max_xi``) is so many radians."""
    s = 2600 + 31 * ny + 7 * nx + nd if seed is None else seed
    r = cases.rng(s)
    dists = dists_for(nd)
    if phase is not None:
        dists = dists * (phase / max_xi(ny, nx, dists))
    delta = delta_map(ny, nx, s)
    truth = delta_map(ny, nx, s + 50, scale=1.2)
    if clip:
        sn, cs = R.xi_sincos((ny, nx), dists, ENERGY_EV, PSIZE_CM)
        o = R.osc(sn, cs, LG_KAPPA)[:, ny // 4, nx // 4]               # osc_d at the tone's bin
        yy, xx = np.mgrid[:ny, :nx]
        tone = np.cos(0.5 * np.pi * (yy + xx))                         # values 1, 0, -1, 0
        # |amp osc_d| stays out of [0.8, 1.25] for every distance (I_d = 1 +- amp osc_d + O(0.1) on the tone's pixels), above it for one
        amp = next(a for a in np.arange(0.7, 6., 0.05) if all(abs(a * v) < 0.8 or abs(a * v) > 1.25 for v in o) and any(abs(a * v) > 1.25 for v in o))
        delta = delta + amp * tone
    beta = 1e-3 * cases.smooth_field((ny, nx), s + 2)
    obj = np.stack([delta, beta], -1).astype(np.float32)
    I = R.forward_adjoint(truth.astype(np.float32), dists, LG_KAPPA_TRUTH, np.ones((nd, ny, nx)), ENERGY_EV, PSIZE_CM, want_grad=False)['I']
    data = (I if raw == 'intensity' else np.sqrt(I)).astype(np.float32)
    return dict(ny=ny, nx=nx, nd=nd, raw=raw, clip=clip, obj=obj, data=data, dists=dists, lg_kappa=np.float32(LG_KAPPA))


def ref_run(c, dtype='float64'):
    return R.forward_adjoint(c['obj'][:, :, 0], c['dists'], c['lg_kappa'], c['data'], ENERGY_EV, PSIZE_CM, c['raw'], dtype)


_CASES = {}


def case(ny, nx, nd, **kw):
    """Inputs and the reference pair (o64, o32), built once per process."""
    key = (ny, nx, nd, tuple(sorted(kw.items())))
    if key not in _CASES:
        c = inputs(ny, nx, nd, **kw)
        c['o64'], c['o32'] = ref_run(c, 'float64'), ref_run(c, 'float32')
        _CASES[key] = c
    return _CASES[key]


# ------------------------------------------------------------------------------------------------------------ judgement
def band_defs(c):
    """name -> (bands, axis, bar) of everything the GPU module judges band by band: the rows of every C3 block of the prediction
    (jobs d * ny + y), the rows of every C5 block of the delta gradient, and the kx lines of FFT2 of both (C2 / C4 work on lines kx)."""
    g = geometry(c['ny'], c['nx'], c['nd'])
    lines = [(k, k + 1) for k in range(c['nx'])]
    return {'pred rows': (g['c3_blocks'], 0, 'pred'), 'grad rows': (g['row_blocks'], 0, 'grad'),
            'pred kx lines': (lines, 1, 'pred'), 'grad kx lines': (lines, 1, 'grad')}


def band_views(c, pred, grad):
    """The arrays band_defs' bands cut, of a prediction [nd, ny, nx] and a delta gradient [ny, nx] (either may be None)."""
    out = {}
    if pred is not None:
        out['pred rows'] = np.asarray(pred).reshape(c['nd'] * c['ny'], c['nx'])
        out['pred kx lines'] = spectrum2(np.asarray(pred, np.float64) - 1.)      # (pred = 1 + small: without the 1, which is bin 0 alone)
    if grad is not None:
        out['grad rows'] = np.asarray(grad)
        out['grad kx lines'] = spectrum2(np.asarray(grad, np.float64))
    return out


def band_sets(c):
    o, s = band_views(c, c['o64']['pred'], c['o64']['grad_delta']), band_views(c, c['o32']['pred'], c['o32']['grad_delta'])
    return [(name, o[name], s[name], bands, axis) for name, (bands, axis, _) in band_defs(c).items()]


def conditions(c):
    """What the reference pair alone decides, without a GPU: min I_d, the ill-conditioning guard (the fp32 restatement within a
    third of every bar) and the bands without signal (none).  Asserts; returns the figures as a line of text."""
    o, s = c['o64'], c['o32']
    I = o['I']
    if c['clip']:
        assert ((I <= CLIP_I) | (I >= MIN_I)).all() and (I <= CLIP_I).sum() >= I[0].size // 8, (c['ny'], c['nx'], float(np.abs(I).min()))
        assert np.array_equal(s['I'] > 0, I > 0)
    else:
        assert I.min() >= MIN_I, (c['ny'], c['nx'], c['nd'], float(I.min()))
    e = dict(pred=rel(s['pred'], o['pred']), grad=rel(s['grad_delta'], o['grad_delta']), loss=abs(s['loss'] / o['loss'] - 1),
             gkappa=abs(s['grad_lg_kappa'] / o['grad_lg_kappa'] - 1))
    for k, v in e.items():
        assert v < BARS[k] / 3, (c['ny'], c['nx'], c['nd'], k, v)
    for name, x64, x32, bands, axis in ([] if c['clip'] else band_sets(c)):       # (the clipped case's tone is one bin: no band judgement)
        _, _, judged = band_errors(x32, x64, x32, bands, axis)
        assert judged.all(), (c['ny'], c['nx'], c['nd'], name, 'bands without signal', int((~judged).sum()), len(judged))
    return 'min I %.3f;  fp32 restatement: pred %.1e  grad %.1e  loss %.1e  gkappa %.1e' % (I.min(), e['pred'], e['grad'], e['loss'], e['gkappa'])
