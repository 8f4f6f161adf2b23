"""adm_project_z and adm_project_z_adj through the C ABI (pytest -m gpu).

Forward: every written element against the host's float64 sum S of the same float32 inputs,
|got - S| <= 2^-24 |S| + Z 2^-53 sum_z |v| (tests/projection_ref.py:z_sum_and_bar: a theorem for a double accumulator in any order
plus one rounding; tests/test_projection_ref_vs_golden.py shows on the CPU that it catches a dropped or doubled slice); rows
outside the range and the y pads keep a sentinel bit for bit; two launches give the same bits.  Adjoint: every slice of the rows is
the source, everything else keeps the sentinel.

Geometries: the run of rows starts on a 16-byte boundary in every slice or not (Xp odd / even, Yp * Xp odd / even, y_lo odd /
even: the kernels' two access widths), its length is even or odd (the wide form's one-pixel tail), and it spans one workgroup or
several; Z = 1 ... 257 covers fewer slices than waves, the unrolled rounds of loads with and without a remainder, and both
numbers of waves along z.
"""
import numpy as np
import pytest

from tests import projection_ref as PJ

pytestmark = pytest.mark.gpu

SENTINEL = np.uint32(0x7fc12345)          # (a NaN payload: no sum produces it)
#        name: (Y, X, pads, ranges)
GEOMS = {
    'xp_odd_slice_even': (5, 37, ((2, 3), (1, 3)), ((0, 5), (1, 4))),        # Xp 41, Yp 10: wide with a tail / narrow (odd start)
    'xp_odd_slice_odd': (5, 37, ((1, 3), (1, 3)), ((0, 5), (2, 3))),         # Xp 41, Yp 9: slices alternate alignment -> narrow
    'xp_even': (33, 130, ((1, 2), (3, 1)), ((0, 33), (7, 30))),              # Xp 134: wide, several workgroups
}
DEPTHS = (1, 2, 7, 64, 257)


@pytest.fixture(scope='module')
def A():
    import adorym_amd
    return adorym_amd


@pytest.fixture(scope='module')
def ctx(A):
    c = A.Context(0)
    yield c
    c.close()


def make_plan(A, ctx, Y, X, Z, pads):
    return A.Plan(ctx, (Y, X, Z), (8, 8), pads, 1.0, np.ones((8, 8), np.complex128))


def sentinel(shape):
    return np.full(shape, SENTINEL, np.uint32).view(np.float32)


def bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


@pytest.mark.parametrize('Z', DEPTHS)
@pytest.mark.parametrize('geom', sorted(GEOMS))
def test_projection_pair(A, ctx, geom, Z):
    from adorym_amd._lib import check
    Y, X, pads, ranges = GEOMS[geom]
    plan = make_plan(A, ctx, Y, X, Z, pads)
    _, Yp, Xp, _ = plan.rot_shape
    r = np.random.default_rng(2500 + 10 * sorted(GEOMS).index(geom) + DEPTHS.index(Z))
    vol = PJ.mixed_values(r, plan.rot_shape)
    S, bar = PJ.z_sum_and_bar(vol)
    gproj = PJ.mixed_values(r, (1, Yp, Xp, 2))
    d_vol, d_gproj = ctx.array(vol), ctx.array(gproj)
    lib, h, y0 = ctx.lib, plan.handle, pads[0][0]
    for lo, hi in ranges:
        rows = np.zeros(Yp, bool)
        rows[y0 + lo:y0 + hi] = True
        # ---- forward, twice
        got = []
        for _ in range(2):
            d_proj = ctx.array(sentinel((1, Yp, Xp, 2)))
            check(lib.adm_project_z(h, d_vol.ptr, lo, hi, d_proj.ptr))
            got.append(d_proj.get()[0])
        assert np.array_equal(bits(got[0]), bits(got[1])), 'two launches differ'
        assert np.all(bits(got[0][~rows]) == SENTINEL), 'a row outside [%d, %d) or a y pad was written' % (lo, hi)
        err = np.abs(got[0][rows].astype(np.float64) - S[rows])
        worst = np.unravel_index(np.argmax(err - bar[rows]), err.shape)
        print(geom, Z, (lo, hi), 'max |got - S| / bar = %.3f' % (err / bar[rows]).max())
        assert np.all(err <= bar[rows]), (geom, Z, lo, hi, worst, got[0][rows][worst], S[rows][worst], bar[rows][worst])
        # ---- adjoint
        d_grot = ctx.array(sentinel(plan.rot_shape))
        check(lib.adm_project_z_adj(h, d_gproj.ptr, lo, hi, d_grot.ptr))
        grot = d_grot.get()
        assert np.all(bits(grot[:, ~rows]) == SENTINEL), 'the broadcast wrote outside the rows [%d, %d)' % (lo, hi)
        for z in range(Z):
            assert np.array_equal(grot[z][rows], gproj[0][rows]), 'slice %d' % z
    plan.close()


def test_empty_range_writes_nothing(A, ctx):
    from adorym_amd._lib import check
    plan = make_plan(A, ctx, 5, 37, 7, ((2, 3), (1, 3)))
    d_vol = ctx.array(PJ.mixed_values(np.random.default_rng(1), plan.rot_shape))
    d_proj = ctx.array(sentinel((1,) + plan.rot_shape[1:]))
    d_grot = ctx.array(sentinel(plan.rot_shape))
    check(ctx.lib.adm_project_z(plan.handle, d_vol.ptr, 3, 3, d_proj.ptr))
    check(ctx.lib.adm_project_z_adj(plan.handle, d_proj.ptr, 3, 3, d_grot.ptr))
    assert np.all(bits(d_proj.get()) == SENTINEL) and np.all(bits(d_grot.get()) == SENTINEL)
    plan.close()


def test_bad_arguments_are_refused(A, ctx):
    from adorym_amd._lib import check
    plan = make_plan(A, ctx, 5, 37, 7, ((2, 3), (1, 3)))
    d_vol = ctx.zeros(plan.rot_shape)
    d_proj = ctx.zeros((1,) + plan.rot_shape[1:])
    for fn, a, b in ((ctx.lib.adm_project_z, d_vol, d_proj), (ctx.lib.adm_project_z_adj, d_proj, d_vol)):
        for lo, hi in ((-1, 2), (0, 6), (3, 2)):
            with pytest.raises(ValueError, match='bad y range'):
                check(fn(plan.handle, a.ptr, lo, hi, b.ptr))
        for args in ((None, a.ptr, 0, 5, b.ptr), (plan.handle, None, 0, 5, b.ptr), (plan.handle, a.ptr, 0, 5, None)):
            with pytest.raises(ValueError, match='null argument'):
                check(fn(*args))
    plan.close()
