"""Tables, mirrors and references of the holography matrix (tests/test_gpu_holo_matrix.py; importable without a GPU).

adm_holo.hip compiles every line kernel for the eight line lengths of ADM_LINE_SIZES; which length a kernel is instantiated by
is the field's nx (rows: K1, K3, K5, SR, SRI) or its ny (lines kx: K2, K4, SLF, SLI).  ``line_geo`` / ``geometry`` restate the
launch arithmetic (LineGeo, blocks_for, K3's jobs, K4's rounds), ``KERNELS`` names every instantiation family and the tests that
run it, ``FIELDS`` is the smallest set of fields that puts every length in both roles and reaches every class of ``ALL_CLASSES``,
``VARIANTS`` the argument values.  tests/test_holo_matrix_coverage.py ties all of it to the kernel source.

The reference is oracle.adorym_oracle.holo_forward_adjoint in fp64, the yardstick of the 3x rule the same function in float32.
The oracle has no delta/beta object: ``oracle_run`` forms c = exp(-k1 beta) exp(-i sigma k1 delta) in the run's precision, hands it
over as a real_imag object and applies the chain rule to the gradient it gets back.  Every input is rounded to float32 first, so
the oracle and the kernels see the same numbers."""
import numpy as np

from oracle import adorym_oracle as O
from tests.golden import cases

ENERGY_EV, PSIZE_CM = 17050., 1e-4
SIZES = (16, 32, 64, 128, 256, 512, 1024, 2048)
MIN_SIDE, MAX_SIDE, MAX_DISTS = 16, 2048, 64
THREADS = 256

# whole-array bars: the ones the holography tests of test_gpu_edge_cases.py use (gdists / gaff: max(bar, 3 x fp32 oracle))
BARS = dict(loss=5e-5, pred=5e-6, grad=2e-4, gdists=2e-3, gaff=2e-3, target=1e-5, spectrum=2e-6, gshift=2e-4)
SIGNAL = 1e-6            # a band is judged when its energy is at least 1e-6 of the strongest band's (norm: 1e-3)
MAX_UNJUDGED = 0.05
MIN_TARGET = 0.05        # the smallest |T| of a shifted case: the relative error of dL/dT at a pixel is that of T, 3e-7 / MIN_TARGET


# ------------------------------------------------------------------------------------------------------------ launch geometry
def line_geo(n):
    """LineGeo<N> and TwLds<N>::USE."""
    tpr = n // 8
    lpb = THREADS // tpr
    lp = n + (32 // (lpb if lpb < 32 else 32) if lpb > 1 else 0)
    return dict(TPR=tpr, LPB=lpb, LP=lp, tw_lds=n <= 1024)


def pow2_in_range(n):
    return MIN_SIDE <= n <= MAX_SIDE and (n & (n - 1)) == 0


def _blocks(lines, lpb):
    return [(lo, min(lo + lpb, lines)) for lo in range(0, lines, lpb)]


def geometry(ny, nx, nd):
    gx, gy = line_geo(nx), line_geo(ny)
    jobs = _blocks(nd * ny, gx['LPB'])
    rounds = -(-nd // gy['LPB'])
    return dict(gx=gx, gy=gy,
                row_blocks=_blocks(ny, gx['LPB']),                      # K1 / K5 / SR / SRI: rows y
                k3_blocks=jobs,                                         # K3: jobs d * ny + y
                k3_spans=[lo // ny != (hi - 1) // ny for lo, hi in jobs],
                col_blocks=_blocks(nx, gy['LPB']),                      # K2 / SLF / SLI: lines kx
                k4_rounds=rounds, k4_ragged=nd % gy['LPB'] != 0,        # K4: one block per kx, LPB(ny) distances per round
                n_sums=nd * 8)                                          # holo_sum_one outputs, spread over K5's blocks


ALL_CLASSES = ('partial_block', 'k3_block_spans_distances', 'k4_one_round', 'k4_several_rounds', 'k4_ragged_last_round',
               'nd_1', 'nd_64', 'twiddles_global', 'tpr_gt_64', 'tpr_le_64')


def classes(ny, nx, nd):
    g = geometry(ny, nx, nd)
    c = set()
    for blocks, lpb in ((g['row_blocks'], g['gx']['LPB']), (g['k3_blocks'], g['gx']['LPB']), (g['col_blocks'], g['gy']['LPB'])):
        if any(hi - lo < lpb for lo, hi in blocks):
            c.add('partial_block')
    if any(g['k3_spans']):
        c.add('k3_block_spans_distances')
    c.add('k4_one_round' if g['k4_rounds'] == 1 else 'k4_several_rounds')
    if g['k4_rounds'] > 1 and g['k4_ragged']:
        c.add('k4_ragged_last_round')
    if nd == 1:
        c.add('nd_1')
    if nd == MAX_DISTS:
        c.add('nd_64')
    for geo in (g['gx'], g['gy']):
        c.add('tpr_gt_64' if geo['TPR'] > 64 else 'tpr_le_64')
        if not geo['tw_lds']:
            c.add('twiddles_global')
    return c


# ------------------------------------------------------------------------------------------------------------ tables
# (ny, nx): n_dists.  The first eight hold 32 768 pixels and put every length in both roles.
FIELDS = {
    (16, 2048): 3, (2048, 16): 3, (32, 1024): 3, (1024, 32): 3,
    (64, 512): 5, (512, 64): 5,          # LPB(512) = 4: K4 in two rounds, the second ragged
    (128, 256): 3, (256, 128): 3,
    (16, 16): 1,                         # 16 lines in a block of 128
    (64, 16): 3,                         # 192 K3 jobs = one and a half blocks; block 0 holds d = 0 and d = 1
    (32, 32): 5,                         # 160 jobs in blocks of 64: ragged last block over two distances
    (256, 16): 64,                       # the most distances: K4 in 8 rounds, 512 sums over 16 K5 blocks
}
BIG8 = tuple(f for f in FIELDS if f[0] * f[1] == 32768)
NEW_KERNELS = tuple(f for f in FIELDS if 2048 in f)          # instantiations no test had launched: run in functions of their own
SHIFT_FIELDS = BIG8 + ((16, 16),)
SPECTRUM_FIELDS = tuple(f for f in FIELDS if f[1] <= 64)     # K4's block is one kx line of nx

# instantiation family -> (axis whose length instantiates it, fields that run it, test functions of test_gpu_holo_matrix.py)
_GRAD = ('test_fields_gradient_launch', 'test_new_kernels_gradient_launch', 'test_variants', 'test_new_kernels_variants')
_FWD = ('test_fields_forward_only', 'test_new_kernels_forward_only')
_SHIFT = ('test_shift_stage', 'test_new_kernels_shift_stage')
KERNELS = {
    'holo_k1<N>': ('nx', 'FIELDS', _GRAD + _FWD),
    'holo_k2<N>': ('ny', 'FIELDS', _GRAD + _FWD),
    'holo_k3<N, true>': ('nx', 'FIELDS', _GRAD),
    'holo_k3<N, false>': ('nx', 'FIELDS', _FWD),
    'holo_k4<N>': ('ny', 'FIELDS', _GRAD + ('test_k4_lines_in_the_spectrum', 'test_new_kernels_lines_in_the_spectrum')),
    'holo_k5<N, false>': ('nx', 'FIELDS', _GRAD),
    'holo_k5<N, true>': ('nx', 'BIG8', ('test_fused_adam_equals_the_separate_update_bitwise', 'test_new_kernels_fused_adam')),
    'holo_sums_kernel': (None, 'FIELDS', _FWD),
    'holo_sr<N>': ('nx', 'SHIFT_FIELDS', _SHIFT),
    'holo_slf<N, 0>': ('ny', 'SHIFT_FIELDS', _SHIFT),
    'holo_slf<N, 1>': ('ny', 'SHIFT_FIELDS', _SHIFT),
    'holo_shift_sum_kernel': (None, 'SHIFT_FIELDS', _SHIFT),
    'holo_sli<N>': ('ny', 'SHIFT_FIELDS', _SHIFT),
    'holo_sri<N>': ('nx', 'SHIFT_FIELDS', _SHIFT),
}


def reached():
    """{(family, N)} the tables launch."""
    sets = dict(FIELDS=tuple(FIELDS), BIG8=BIG8, SHIFT_FIELDS=SHIFT_FIELDS)
    out = set()
    for k, (axis, fields, _) in KERNELS.items():
        for ny, nx in sets[fields]:
            out.add((k, {'nx': nx, 'ny': ny, None: 0}[axis]))
    return out


# name -> (case keywords, launch keywords, touches K2 / K4: also run at (2048, 16))
VARIANTS = {
    'delta_beta': (dict(unknown_type='delta_beta'), {}, True),
    'sigma_minus': (dict(sigma=-1), {}, True),
    'magnitude': (dict(raw='magnitude'), {}, False),
    'delta_beta_sigma_minus': (dict(unknown_type='delta_beta', sigma=-1), {}, True),
    'plane_probe': (dict(probe='plane'), {}, False),
    'no_affine': (dict(affine='none'), dict(want=('probe', 'dists')), False),
    'grad_affine_without_affine': (dict(affine='none'), {}, False),
    'clamped_translation': (dict(affine='clamp'), {}, False),
    'grad_dists_only': ({}, dict(want=('probe', 'dists')), True),
    'grad_affine_only': ({}, dict(want=('probe', 'affine')), False),
    'no_small_gradients': ({}, dict(want=('probe',)), True),
    'no_grad_probe': ({}, dict(want=('dists', 'affine')), False),
    'no_pred': ({}, dict(want_pred=False), False),
    'forward_only': ({}, dict(want_grad=False), True),
    'accumulate': ({}, dict(seed='seeded'), True),
    'accumulate_delta_beta': (dict(unknown_type='delta_beta'), dict(seed='seeded'), False),
    'overwrite_sentinel': ({}, dict(seed='sentinel', overwrite=True), True),
}
VARIANT_FIELD, VARIANT_FIELD_K4 = (128, 256), (2048, 16)
VARIANT_CASES = [(n, VARIANT_FIELD) for n in VARIANTS] + [(n, VARIANT_FIELD_K4) for n, v in VARIANTS.items() if v[2]]


# ------------------------------------------------------------------------------------------------------------ inputs
def k1_of(energy_ev=ENERGY_EV, psize_cm=PSIZE_CM):
    """HolographyEngine's k1 as the kernels get it (adm_holo_desc::k1 is a float)."""
    return np.float32(2. * np.pi * (psize_cm * 1e7) / (1240. / energy_ev))


def inputs(ny, nx, nd, unknown_type='real_imag', sigma=1, raw='intensity', probe='structured', affine='random', shifts=False,
           broadband=False, seed=None):
    """Host inputs of one case, float32 (what is uploaded; the oracle gets the same numbers).  Smooth object, probe and data as
    in the holography tests of test_gpu_edge_cases.py; with ``shifts`` the data are uncorrelated noise, which keeps the
    cancellation in the shift gradient that the kernel's double accumulation is there for.  ``broadband``: object and data of
    uncorrelated noise (test_shifted_holograms_vs_oracle_at_other_sizes' inputs), for the checks that judge the two-dimensional
    spectrum line by line: the smooth fields leave 5 - 20 % of the kx lines of a 16 ... 64 wide gradient without signal."""
    s = 7000 + 31 * ny + 7 * nx + nd if seed is None else seed
    r = cases.rng(s)
    f = lambda k: cases.smooth_field((ny, nx, 1), s + k)
    if broadband:
        o = (1 + 0.1 * r.standard_normal((ny, nx, 1))) * np.exp(0.2j * r.standard_normal((ny, nx, 1)))
        obj = np.stack([o.real, o.imag], -1)
    elif unknown_type == 'real_imag':
        mag, ph = 1 - 0.2 * f(1), 0.5 * f(2)
        obj = np.stack([mag * np.cos(ph), mag * np.sin(ph)], -1)
    else:
        obj = np.stack([4e-6 * (f(1) - 0.5), 4e-7 * f(2)], -1)          # k1 = 8.6e4: phase within 0.2 rad, absorption to 3 %
    if probe == 'plane':
        pr = np.ones((ny, nx), complex)
    else:
        pr = (1 + 0.2 * f(3)[:, :, 0]) * np.exp(0.3j * f(4)[:, :, 0])
    ident = np.tile(np.array([[1., 0, 0], [0, 1., 0]]), [nd, 1, 1])
    jitter = 0.01 * r.uniform(-1, 1, (nd, 2, 3))
    if affine == 'none' or shifts:
        aff = ident
    elif affine == 'clamp':
        aff = ident + jitter
        aff[:, 0, 2] += 0.2                 # a tenth of the width / 0.075 of the height past the border
        aff[:, 1, 2] -= 0.15
    else:
        aff = ident + jitter
    if shifts or broadband:
        # (shifts: 0.1, not the 0.2 of test_shifted_holograms_vs_oracle_at_other_sizes -- with 0.2 the Fourier-shifted holograms T come
        # within 6e-5 of zero at single pixels of 32 768, where d sqrt|T| / dT = 1 / (2 sqrt|T|) diverges and one pixel carries 1e-3 of a
        # shift gradient in either float32 run; oracle_conditions asserts min |T| >= MIN_TARGET)
        data = (1 + (0.1 if shifts else 0.2) * r.standard_normal((nd, ny, nx))) ** 2
        sh = r.uniform(-1.5, 1.5, (nd, 2)).astype(np.float32) if shifts else None
    else:
        data = (1 + 0.1 * cases.smooth_field((nd, ny, nx), s + 5)) ** 2
        sh = None
    dists = 3. + 6. * np.arange(nd) / max(nd - 1, 1)
    return dict(ny=ny, nx=nx, nd=nd, unknown_type=unknown_type, sigma=sigma, raw=raw, has_affine=affine != 'none' and not shifts,
                obj=obj.astype(np.float32), probe=pr.astype(np.complex64), dists=dists.astype(np.float32),
                affine=aff.astype(np.float32), data=data.astype(np.float32), shifts=sh)


def transmission(obj, unknown_type, sigma, dtype):
    """c(obj) [ny, nx] complex in ``dtype`` from the object [ny, nx, 1, 2]."""
    dt = np.dtype(dtype)
    a, b = obj[:, :, 0, 0].astype(dt), obj[:, :, 0, 1].astype(dt)
    if unknown_type == 'real_imag':
        return a + 1j * b
    k1 = dt.type(k1_of())
    e, ph = np.exp(-k1 * b), dt.type(sigma) * k1 * a
    return (e * np.cos(ph) - 1j * (e * np.sin(ph))).astype(np.complex128 if dt == np.float64 else np.complex64)


def oracle_run(c, dtype='float64'):
    """holo_forward_adjoint on the inputs ``c`` in ``dtype``; delta/beta objects through c(obj) and the chain rule."""
    dt = np.dtype(dtype)
    cdt = np.complex128 if dt == np.float64 else np.complex64
    t = transmission(c['obj'], c['unknown_type'], c['sigma'], dt)
    ri = np.stack([t.real, t.imag], -1)[:, :, None, :].astype(dt)
    res = O.holo_forward_adjoint(ri, c['probe'].astype(cdt), c['dists'].astype(dt), c['affine'].astype(dt), c['data'].astype(dt),
                                 ENERGY_EV, PSIZE_CM, raw_data_type=c['raw'], sign_convention=c['sigma'], dtype=dtype,
                                 shifts=None if c['shifts'] is None else c['shifts'].astype(dt))
    g = np.asarray(res[3], dt)
    if c['unknown_type'] != 'real_imag':
        k1, sg = dt.type(k1_of()), dt.type(c['sigma'])
        gre, gim = g[:, :, 0, 0], g[:, :, 0, 1]
        g = np.stack([sg * k1 * (gre * t.imag - gim * t.real), -k1 * (gre * t.real + gim * t.imag)], -1)[:, :, None, :].astype(dt)
    out = dict(loss=float(res[0]), pred=res[1], target=res[2], g_obj=g, g_probe=res[4], g_dists=res[5], g_aff=res[6])
    if c['shifts'] is not None:
        out['g_shifts'] = res[7]
    return out


def wrapped_loss(c, obj):
    """The fp64 loss as a function of the object array (the finite-difference check of the delta/beta chain rule)."""
    return oracle_run(dict(c, obj=obj), 'float64')['loss']


_CASES = {}


def case(ny, nx, nd, **kw):
    """Inputs and the oracle pair (o64, o32), built once per process."""
    key = (ny, nx, nd, tuple(sorted(kw.items())))
    if key not in _CASES:
        c = inputs(ny, nx, nd, **kw)
        c['o64'], c['o32'] = oracle_run(c, 'float64'), oracle_run(c, 'float32')
        _CASES[key] = c
    return _CASES[key]


def clamped_samples(c):
    """How many sampling points of the registration fall at or beyond the border (grid_sampler's mask is 0), per axis."""
    nx_, ny_ = 0, 0
    for th in c['affine'].astype(np.float64):
        base = lambda n: (np.linspace(-1, 1, n) * (n - 1)) / n
        X, Y = np.meshgrid(base(c['nx']), base(c['ny']))
        ix = ((th[0, 0] * X + th[0, 1] * Y + th[0, 2] + 1) * c['nx'] - 1) / 2
        iy = ((th[1, 0] * X + th[1, 1] * Y + th[1, 2] + 1) * c['ny'] - 1) / 2
        nx_ += int((~((ix > 0) & (ix < c['nx'] - 1))).sum())
        ny_ += int((~((iy > 0) & (iy < c['ny'] - 1))).sum())
    return nx_, ny_


# ------------------------------------------------------------------------------------------------------------ judgement
def rel(a, b):
    return float(np.linalg.norm(np.asarray(a).ravel() - np.asarray(b).ravel()) / np.linalg.norm(np.asarray(b).ravel()))


def complex_of(a):
    """[..., 2] -> complex."""
    a = np.asarray(a)
    return a[..., 0] + 1j * a[..., 1]


def band_errors(x, x64, x32, bands, axis):
    """tests/test_gpu_streamed_matrix.band_errors for one axis and a given list of bands (lo, hi): the relative distance of ``x``
    and of the oracle's fp32 run from the fp64 oracle per band, and which bands carry enough signal to be judged.  Arrays are
    [..., ny, nx] (summed over what is in front); axis 0: bands of rows, axis 1: bands of columns."""
    ny, nx = np.shape(x64)[-2:]
    sq = lambda d: (np.abs(d) ** 2).reshape(-1, ny, nx).sum(0)
    x64 = np.asarray(x64)
    d, d32, n64 = sq(np.asarray(x) - x64), sq(np.asarray(x32) - x64), sq(x64)
    sums = lambda a: np.add.reduceat(a.sum(1 - axis), [lo for lo, _ in bands])
    n = sums(n64)
    judged = n >= SIGNAL * n.max()
    with np.errstate(divide='ignore', invalid='ignore'):
        e, e32 = np.sqrt(sums(d) / n), np.sqrt(sums(d32) / n)
    return e, e32, judged


def check_bands(x, x64, x32, bands, axis, floor, what, quiet=False):
    """The 3x rule on every band: its error at most 3 x the fp32 oracle's on the same band + the whole-array floor; at most 5 %
    of the bands left out for lack of signal.  Returns (band, bands, error, fp32 oracle's error) of the worst margin."""
    e, e32, judged = band_errors(x, x64, x32, bands, axis)
    assert (~judged).sum() <= MAX_UNJUDGED * len(judged), (what, 'bands without signal', int((~judged).sum()), len(judged))
    margin = np.where(judged, e - (3 * e32 + floor), -np.inf)
    k = int(np.argmax(margin))
    worst = (k, len(e), float(e[k]), float(e32[k]))
    if not quiet:
        print('%s bands: worst %d of %d: %.2e (fp32 oracle %.2e, bar %.2e)' % ((what,) + worst + (3 * e32[k] + floor,)))
    assert margin[k] <= 0, (what, 'band %d of %d' % (k, len(e)), float(e[k]), float(e32[k]), floor)
    return worst


def oracle_conditions(c, spectral=False):
    """What the oracle pair alone decides, without a GPU: the ill-conditioning guard (the fp32 oracle within a third of the bar
    for the prediction and the object and probe gradients) and the 5 % cap on bands without signal, for every band the GPU module
    judges.  Asserts both; returns the figures as a line of text."""
    o, s = c['o64'], c['o32']
    g = geometry(c['ny'], c['nx'], c['nd'])
    e = {k: rel(s[k], o[k]) for k in ('pred', 'g_obj', 'g_probe')}
    for k, v in e.items():
        assert v < BARS['pred' if k == 'pred' else 'grad'] / 3, (c['ny'], c['nx'], k, v)
    cx = lambda a: complex_of(np.asarray(a)[:, :, 0])
    flat = lambda a: np.asarray(a).reshape(c['nd'] * c['ny'], c['nx'])
    sets = [('pred[%d]' % d, o['pred'][d], s['pred'][d], g['row_blocks'], 0) for d in range(c['nd'])]
    sets += [('pred K3', flat(o['pred']), flat(s['pred']), g['k3_blocks'], 0), ('g_obj', cx(o['g_obj']), cx(s['g_obj']), g['row_blocks'], 0),
             ('g_probe', o['g_probe'], s['g_probe'], g['row_blocks'], 0)]
    if c['shifts'] is not None:
        assert (o['target'] ** 2).min() >= MIN_TARGET, (c['ny'], c['nx'], 'a registered hologram touches zero', float((o['target'] ** 2).min()))
        sets += [('target[%d]' % d, o['target'][d], s['target'][d], g['row_blocks'], 0) for d in range(c['nd'])]
    if spectral:
        sets += [('K4 lines', spectrum2(o['g_obj']), spectrum2(s['g_obj']), [(k, k + 1) for k in range(c['nx'])], 1)]
        sets += [('K2 blocks[%d]' % d, spectrum2(o['pred'][d]), spectrum2(s['pred'][d]), g['col_blocks'], 1) for d in range(c['nd'])]
    left, worst, weakest = 0, {}, 1.
    for name, x64, x32, bands, axis in sets:
        be, be32, judged = band_errors(x32, x64, x32, bands, axis)
        assert (~judged).sum() <= MAX_UNJUDGED * len(judged), (c['ny'], c['nx'], name, 'bands without signal', int((~judged).sum()), len(judged))
        left += int((~judged).sum())
        key = name.split('[')[0]
        worst[key] = max(worst.get(key, 0.), float(be32[judged].max()))
    return 'fp32 oracle: pred %.1e  g_obj %.1e  g_probe %.1e;  bands without signal %d;  worst band of the fp32 oracle %s' % (
        e['pred'], e['g_obj'], e['g_probe'], left, '  '.join('%s %.1e' % kv for kv in worst.items()))


def spectrum2(g):
    """FFT2 in fp64 of a gradient [ny, nx, 1, 2] (or a complex / real field [..., ny, nx])."""
    g = np.asarray(g)
    if g.ndim == 4 and g.shape[-1] == 2:
        g = g[:, :, 0, 0].astype(np.float64) + 1j * g[:, :, 0, 1].astype(np.float64)
    return np.fft.fft2(g.astype(np.complex128 if np.iscomplexobj(g) else np.float64))


def data_spectrum_pair(c):
    """FFT2(|data|) [d][ky][kx] in fp64 and in float32 (scipy's transform works in the precision of its input)."""
    import scipy.fft as sfft
    a = np.abs(c['data'])
    return np.fft.fft2(a.astype(np.float64)), sfft.fft2(a.astype(np.complex64))


def sentinel(shape, seed):
    """A finite pattern no result equals: magnitudes over 2^+-12, mixed signs."""
    r = cases.rng(seed)
    return (np.ldexp(r.uniform(0.5, 1, shape), r.integers(-12, 13, shape)) * r.choice([-1., 1.], shape)).astype(np.float32)


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)
