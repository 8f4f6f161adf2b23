"""The direct CTF inversion's kernels (adm_ctf_invert.hip: three line-kernel templates at the eight line lengths of
ADM_LINE_SIZES, three ABI entry points) through adorym_amd.CTFInversion and the C ABI against tests/ctfinv_ref.py in fp64
(pytest -m gpu).  tests/ctfinv_matrix.py holds the cases, the mirror of the launch geometry and the references;
tests/test_ctfinv_coverage.py ties those tables to the kernel source, tests/test_ctfinv_ref_vs_golden.py the reference to golden
F31 and every case here to its conditions.

Judged twice.  Whole phase maps by M.BAR = 3 x the largest distance of the float32 restatement from fp64 over the table (a value
rung by 3 x the restatement's distance at that rung).  Then band by band (holo_matrix.check_bands: 3 x the float32 restatement on
the same band + the whole-array bar): the rows of every I3 block and the kx lines of the spectrum per I2 block.

Every case builds one engine, uploads, retrieves once and reads back; the reference pair is built once per module (M.case)."""
import ctypes as C

import numpy as np
import pytest

from tests import ctfinv_matrix as M

pytestmark = pytest.mark.gpu


@pytest.fixture(scope='module')
def A():
    import adorym_amd
    return adorym_amd


@pytest.fixture(scope='module')
def ctx(A):
    c = A.Context(0)
    yield c
    c.close()


def engine(A, ctx, c, **kw):
    kw.setdefault('max_batch', c['max_batch'])
    kw.setdefault('alpha', c['alpha'])
    return A.CTFInversion(ctx, (c['ny'], c['nx']), c['nd'], M.ENERGY_EV, M.PSIZE_CM, **kw)


def run(A, ctx, c, eng=None, data=None):
    """One CTFInversion.retrieve of the case ``c``: phase [nb, ny, nx]; with out_stride 2 the object it was written into and the
    object as it was before, too."""
    eng = eng or engine(A, ctx, c)
    data = ctx.array(c['data'] if data is None else data)
    lgk = ctx.array(np.array([c['lg_kappa']], np.float32))
    if c['out_stride'] == 2:
        before = M.sentinel((c['ny'], c['nx'], 2), 71)
        obj = ctx.array(before)
        eng.retrieve(data, c['dists'], lgk, out=obj, into_object=True)
        after = obj.get()
        return dict(phase=after[None, :, :, 0], obj=after, before=before)
    out = ctx.array(M.sentinel((c['nb'], c['ny'], c['nx']), 73))
    assert eng.retrieve(data, c['dists'], lgk, out=out) is out
    return dict(phase=out.get())


def judge(res, c, what):
    o, s = np.asarray(c['o64']).reshape(res['phase'].shape), np.asarray(c['o32']).reshape(res['phase'].shape)
    assert np.isfinite(res['phase']).all(), what
    e, e32 = M.rel(res['phase'], o), M.rel(s, o)
    print('%s: phase %.2e (fp32 restatement %.2e, bar %.2e)' % (what, e, e32, c['bar']))
    assert e <= c['bar'], (what, e, e32, c['bar'])
    for b in range(c['nb']):          # (an angle swapped with another or left unwritten hides in no sum)
        eb = M.rel(res['phase'][b], o[b])
        assert eb <= c['bar'], (what, 'angle %d' % b, eb)
    mine, oo, ss = M.band_views(c, res['phase']), M.band_views(c, o), M.band_views(c, s)
    worst = {}
    for name, (bands, axis) in M.band_defs(c).items():
        worst[name] = M.check_bands(mine[name], oo[name], ss[name], bands, axis, c['bar'], '%s %s' % (what, name), quiet=True)
    print('%s worst bands (band, of, error, fp32 restatement): %s' % (what, {k: '%d/%d %.2e (%.2e)' % v for k, v in worst.items()}))


def same_bits(a, b, what):
    a, b = M.bits(a), M.bits(b)
    assert a.shape == b.shape, what
    bad = int((a != b).sum())
    assert bad == 0, (what, '%d of %d elements differ' % (bad, a.size))


# ------------------------------------------------------------------------------------------------------------ the table
@pytest.mark.parametrize('name', list(M.CASES))
def test_cases(A, ctx, name):
    """I1, I2, I3 at every field of ctf_matrix.FIELDS, and what batch, rounds, output stride and the regulariser add.  With
    out_stride 2 the beta channel keeps its sentinel bit for bit."""
    c = M.case(name)
    res = run(A, ctx, c)
    judge(res, c, name)
    if c['out_stride'] == 2:
        same_bits(res['obj'][..., 1], res['before'][..., 1], name + ': the beta channel')


@pytest.mark.parametrize('name', list(M.VALUE_CASES))
def test_value_classes(A, ctx, name):
    """xi scaled to 100, 1000 and 3000 rad (sincos_fast's argument), and lg_kappa = 30: w at DC is 1e-30, the denominator there
    is alpha alone, every value is finite and the map has no mean beyond the rounding of its pixels."""
    c = M.case(name)
    res = run(A, ctx, c)
    judge(res, c, name)
    if name == 'pure_phase':
        p = res['phase'].astype(np.float64)
        n = c['ny'] * c['nx']
        # DC of the spectrum is 1e-20 FFT2(I - 1)(0): nothing; what is left is the transforms' rounding, eps log2(n) of the largest value
        assert abs(p.mean()) <= np.finfo(np.float32).eps * np.log2(n) * np.abs(p).max(), p.mean()


def test_constant_data(A, ctx):
    """All-ones holograms (I - 1 = 0) give exactly 0 everywhere; zero holograms (I - 1 = -1: the DC bin alone) the constant the
    restatement gives, -D / kappa / (2 D / kappa^2 + alpha)."""
    c = dict(M.case('phase_100_rad'))
    eng = engine(A, ctx, c)
    ones = run(A, ctx, c, eng, np.ones_like(c['data']))['phase']
    assert not (ones != 0).any()
    zero = run(A, ctx, c, eng, np.zeros_like(c['data']))['phase']
    c0 = dict(c, data=np.zeros_like(c['data']))
    want = M.ref_run(c0)
    assert np.isfinite(zero).all() and np.ptp(want) < 1e-9 * abs(want.mean()) and want.mean() < -10
    e = M.rel(zero, want)
    print('zero data: %.2e (bar %.2e), value %.6f' % (e, M.BAR, want.mean()))
    assert e <= M.BAR


# ------------------------------------------------------------------------------------------------------------ relations
@pytest.mark.regression
def test_two_calls_give_identical_bits(A, ctx):
    for name in ('128x256x4', '2048x16x3', '256x16x64', '16x16x3_B3'):
        c = M.case(name)
        eng = engine(A, ctx, c)
        same_bits(run(A, ctx, c, eng)['phase'], run(A, ctx, c, eng)['phase'], name)
        same_bits(run(A, ctx, c)['phase'], run(A, ctx, c)['phase'], name + ' (fresh handles)')


@pytest.mark.regression
def test_one_handle_many_launches(A, ctx):
    """One engine through launches of different data, batch counts, strides and kappa equals fresh engines; a batch equals its
    angles one by one, whatever the rounds."""
    c3, c1 = M.case('16x16x3_B3'), M.case('16x16x3')
    eng = engine(A, ctx, c3)
    into = dict(c1, out_stride=2)
    hot = dict(c1, lg_kappa=np.float32(1.5))
    for cc in (c3, c1, into, hot, c3):
        same_bits(run(A, ctx, cc, eng)['phase'], run(A, ctx, cc)['phase'], (cc['name'], cc['out_stride'], float(cc['lg_kappa'])))
    whole = run(A, ctx, c3, eng)['phase']
    ragged = run(A, ctx, M.case('16x16x3_B3_rounds_of_2'))['phase']
    same_bits(whole, ragged, 'rounds of 3 and of 2 + 1')
    for b in range(3):
        one = run(A, ctx, dict(c1, data=c3['data'][b:b + 1]), eng)['phase']
        same_bits(whole[b], one[0], 'angle %d alone' % b)
    del eng


def _create(ctx, ny=16, nx=16, nd=1, mb=1, alpha=None, energy=M.ENERGY_EV):
    from adorym_amd._lib import CtfInvDesc
    h = C.c_void_p()
    desc = CtfInvDesc(ny=ny, nx=nx, n_dists=nd, max_batch=mb, energy_ev=energy, psize_cm=M.PSIZE_CM)
    a = None if alpha is None else np.ascontiguousarray(alpha, np.float32)
    rc = ctx.lib.adm_ctfinv_create(ctx.handle, C.byref(desc), None if a is None else a.ctypes.data, C.byref(h))
    return rc, h


def test_create_refusals(ctx):
    from adorym_amd._lib import ADM_ERR_UNSUPPORTED, ADM_ERR_INVALID, ADM_OK
    for ny, nx in ((24, 16), (16, 24), (4096, 16), (16, 4096), (8, 16), (16, 8)):
        rc, h = _create(ctx, ny, nx)
        assert rc == ADM_ERR_UNSUPPORTED and not h.value, (ny, nx, rc)
        assert b'adm_ctfinv_create' in ctx.lib.adm_last_error()
    good = np.full((16, 16), 1e-3, np.float32)
    bad_alpha = []
    for v in (0., -1e-3, np.nan, np.inf):
        a = good.copy()
        a[5, 11] = v
        bad_alpha.append(dict(alpha=a))
    for kw in [dict(nd=0), dict(nd=65), dict(mb=0), dict(mb=-1), dict(energy=0.)] + bad_alpha:
        rc, h = _create(ctx, **kw)
        assert rc == ADM_ERR_INVALID and not h.value, (kw, rc)
        assert b'adm_ctfinv_create' in ctx.lib.adm_last_error()
    rc, _ = _create(ctx)
    assert rc == ADM_OK
    assert ctx.lib.adm_ctfinv_create(ctx.handle, None, None, None) == ADM_ERR_INVALID
    rc, h = _create(ctx, alpha=good)
    assert rc == ADM_OK and ctx.lib.adm_ctfinv_destroy(h) == ADM_OK and ctx.lib.adm_ctfinv_destroy(None) == ADM_OK


def test_run_refusals(ctx):
    """n_batch outside [1, max_batch], out_stride not 1 or 2, a NULL pointer: ADM_ERR_INVALID, and nothing is written."""
    from adorym_amd._lib import ADM_ERR_INVALID, ADM_OK
    rc, h = _create(ctx, 16, 16, 2, mb=2)
    assert rc == ADM_OK
    data, lgk = ctx.array(np.ones((2, 2, 16, 16), np.float32)), ctx.array(np.array([1.7], np.float32))
    before = M.sentinel((2, 16, 16, 2), 75)
    out = ctx.array(before)
    d = np.array([40., 90.])
    dp = d.ctypes.data_as(C.POINTER(C.c_double))
    calls = [(data.ptr, 0, dp, lgk.ptr, out.ptr, 1), (data.ptr, 3, dp, lgk.ptr, out.ptr, 1), (data.ptr, -1, dp, lgk.ptr, out.ptr, 1),
             (data.ptr, 1, dp, lgk.ptr, out.ptr, 0), (data.ptr, 1, dp, lgk.ptr, out.ptr, 3),
             (None, 1, dp, lgk.ptr, out.ptr, 1), (data.ptr, 1, None, lgk.ptr, out.ptr, 1), (data.ptr, 1, dp, None, out.ptr, 1),
             (data.ptr, 1, dp, lgk.ptr, None, 1)]
    for args in calls:
        assert ctx.lib.adm_ctfinv_run(h, *args) == ADM_ERR_INVALID, args[1:]
        assert b'adm_ctfinv_run' in ctx.lib.adm_last_error()
    assert ctx.lib.adm_ctfinv_run(None, data.ptr, 1, dp, lgk.ptr, out.ptr, 1) == ADM_ERR_INVALID
    same_bits(out.get(), before, 'a refused call wrote')
    assert ctx.lib.adm_ctfinv_run(h, data.ptr, 2, dp, lgk.ptr, out.ptr, 1) == ADM_OK
    got = out.get().reshape(-1)
    assert not (got[:2 * 256] != 0).any()                                  # (all-ones data)
    same_bits(got[2 * 256:], before.reshape(-1)[2 * 256:], 'beyond [n_batch][ny][nx]')
    assert ctx.lib.adm_ctfinv_destroy(h) == ADM_OK


def test_engine_checks(A, ctx):
    """CTFInversion.retrieve refuses by name what does not fit, before anything is queued."""
    c = M.case('16x16x3_B3')
    eng = engine(A, ctx, c)
    data, lgk = ctx.array(c['data']), ctx.array(np.array([1.7], np.float32))
    with pytest.raises(TypeError, match='data must be a DeviceArray'):
        eng.retrieve(c['data'], c['dists'], lgk)
    with pytest.raises(ValueError, match='data must be float32'):
        eng.retrieve(ctx.array(c['data'][:, :2]), c['dists'], lgk)
    with pytest.raises(ValueError, match='distances given'):
        eng.retrieve(data, c['dists'][:2], lgk)
    with pytest.raises(ValueError, match='lg_kappa must be float32'):
        eng.retrieve(data, c['dists'], ctx.array(np.zeros(2, np.float32)))
    with pytest.raises(ValueError, match='out must be float32'):
        eng.retrieve(data, c['dists'], lgk, out=ctx.zeros((2, 16, 16)))
    with pytest.raises(ValueError, match='into_object takes one angle'):
        eng.retrieve(data, c['dists'], lgk, out=ctx.zeros((16, 16, 2)), into_object=True)
    with pytest.raises(ValueError, match='affine registration takes one angle'):
        eng.retrieve(data, c['dists'], lgk, affine=ctx.zeros((3, 2, 3)))
    with pytest.raises(ValueError, match='alpha must be a scalar or'):
        A.CTFInversion(ctx, (16, 16), 3, M.ENERGY_EV, M.PSIZE_CM, alpha=np.ones((16, 32)))
    with pytest.raises(ValueError, match='alpha must be finite and > 0'):
        A.CTFInversion(ctx, (16, 16), 3, M.ENERGY_EV, M.PSIZE_CM, alpha=0.)
    # [D, ny, nx] data is one angle; without ``out`` the engine's own array comes back
    one = eng.retrieve(ctx.array(c['data'][1]), c['dists'], lgk)
    assert one.shape == (1, 16, 16)
    same_bits(one.get()[0], eng.retrieve(data, c['dists'], lgk).get()[1], 'one angle as [D, ny, nx]')


# ------------------------------------------------------------------------------------------------------------ registration, wrapper
def test_identity_affine(A, ctx):
    """retrieve(affine=identity) against retrieve(): the holograms pass through HologramRegistration (bilinear samples of |data|
    at the pixels' own centres); the bar is 3 x what the reference's own identity resample does to its float32 phase (golden F31)."""
    for name in ('64x32x3', '16x32x2'):
        c = M.case(name)
        eng = engine(A, ctx, c)
        data, lgk = ctx.array(c['data']), ctx.array(np.array([c['lg_kappa']], np.float32))
        plain = eng.retrieve(data, c['dists'], lgk).get()
        ident = ctx.array(np.tile(np.array([[1., 0., 0.], [0., 1., 0.]], np.float32), (c['nd'], 1, 1)))
        reg = eng.retrieve(data, c['dists'], lgk, affine=ident).get()
        e = M.rel(reg, plain)
        print('%s: identity registration moves the phase by %.2e (bar %.2e)' % (name, e, M.IDENTITY_BAR))
        assert e <= M.IDENTITY_BAR
        shift = ctx.array(np.tile(np.array([[1., 0., 0.25], [0., 1., 0.]], np.float32), (c['nd'], 1, 1)))
        assert M.rel(eng.retrieve(data, c['dists'], lgk, affine=shift).get(), plain) > 100 * M.IDENTITY_BAR      # (the matrices are read)


def test_conventional_wrapper(A, ctx):
    """adorym_amd.conventional.multidistance_ctf_wrapped, the reference's signature, numpy in and out."""
    c = M.case('32x16x2')
    kappa = 10. ** float(c['lg_kappa'])
    got = A.conventional.multidistance_ctf_wrapped(c['data'][0], c['dists'], M.ENERGY_EV, M.PSIZE_CM, kappa=kappa, device=ctx)
    assert got.shape == (32, 16) and got.dtype == np.float32
    e = M.rel(got, c['o64'][0])
    assert e <= c['bar'], e
    with pytest.raises(NotImplementedError, match='safe_zone_width'):
        A.conventional.multidistance_ctf_wrapped(c['data'][0], c['dists'], M.ENERGY_EV, M.PSIZE_CM, kappa=kappa, safe_zone_width=2, device=ctx)
