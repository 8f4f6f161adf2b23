"""adm_rotate_project_fwd and adm_rotate_project_adj through the C ABI (pytest -m gpu): every row of tests/rotproj_matrix.py under
bar 1 (element-wise, derived), bar 2 (the 3x rule against the fp64 oracle), adjointness from the GPU's own two results and
bitwise canaries, with the unfused pair of kernels printed beside them.  tests/test_rotate_project_coverage.py proves on the CPU
that the rows reach the launch branches their comments name.
"""
import numpy as np
import pytest

from tests import rot_matrix as RM
from tests import rotproj_matrix as PM

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


def make_plan(ctx, size):
    """A bare plan on rot_matrix.positions: pads (3, 1) x (2, 4)."""
    from adorym_amd.device import Plan
    plan = Plan(ctx, size, (RM.P, RM.P), RM.pads_of(size), 1.0, np.ones((RM.P, RM.P), complex))
    Yp, Xp, py0, px0 = RM.frame(size)
    assert plan.rot_shape == (size[2], Yp, Xp, 2) and py0 > 0 and px0 > 0
    return plan


def device_coords(ctx, c):
    return None if c.coords is None else ctx.array(np.ascontiguousarray(c.coords).view(np.uint16))


def run_forward(ctx, plan, c, d_coords, lo, hi):
    """-> ([Y, X, 2] of the fused kernel, the same from adm_rotate_fwd + adm_project_z); canaries checked here (bar 4)."""
    from adorym_amd._lib import check
    Y, X, Z = c.size
    Yp, Xp, py0, px0 = RM.frame(c.size)
    d_obj = ctx.array(c.obj)
    cp = d_coords.ptr if d_coords is not None else None
    outs = []
    for _ in range(2):
        d_proj = ctx.array(np.full((Yp, Xp, 2), RM.SENTINEL, np.float32))
        check(ctx.lib.adm_rotate_project_fwd(plan.handle, d_obj.ptr, cp, d_proj.ptr, lo, hi))
        outs.append(d_proj.get())
    buf = outs[0]
    assert RM.same_bits(outs[0], outs[1]), 'the fused forward gave different bits on its second call'
    rows = np.zeros((Yp, Xp, 2), bool)
    rows[py0 + lo:py0 + hi] = True
    inner = np.zeros_like(rows)
    inner[py0 + lo:py0 + hi, px0:px0 + X] = True
    assert RM.same_bits(buf[~rows], np.full((~rows).sum(), RM.SENTINEL, np.float32)), 'proj written outside the rows of the range'
    assert not buf[rows & ~inner].view(np.uint32).any(), 'the x pads of the rows are not +0'
    # the unfused pair on the same plan
    d_rot = ctx.array(np.zeros(plan.rot_shape, np.float32))
    d_two = ctx.array(np.zeros((Yp, Xp, 2), np.float32))
    check(ctx.lib.adm_rotate_fwd(plan.handle, d_obj.ptr, cp, d_rot.ptr, lo, hi))
    check(ctx.lib.adm_project_z(plan.handle, d_rot.ptr, lo, hi, d_two.ptr))
    return buf[py0:py0 + Y, px0:px0 + X], d_two.get()[py0:py0 + Y, px0:px0 + X]


def run_adjoint(ctx, plan, c, tables, lo, hi, g0):
    """-> (grad_obj of the fused kernel, the same from adm_project_z_adj + adm_rotate_adj_csr)."""
    from adorym_amd._lib import check
    Y, X, Z = c.size
    Yp, Xp, py0, px0 = RM.frame(c.size)
    gp = np.full((Yp, Xp, 2), RM.POISON, np.float32)
    gp[py0 + lo:py0 + hi, px0:px0 + X] = c.cot[lo:hi]
    d_gp = ctx.array(gp)
    tp = [t.ptr for t in tables] if tables is not None else [None] * 3
    outs = []
    for lanes_x in (0, 1):
        d_g = ctx.array(g0)
        check(ctx.lib.adm_rotate_project_adj(plan.handle, d_gp.ptr, tp[0], tp[1], tp[2], d_g.ptr, lo, hi, lanes_x))
        outs.append(d_g.get())
    got = outs[0]
    assert RM.same_bits(outs[0], outs[1]), 'the fused adjoint gave different bits on its second call'
    assert RM.same_bits(got[:lo], g0[:lo]) and RM.same_bits(got[hi:], g0[hi:]), 'grad_obj touched outside the y range'
    # the unfused pair: the pads of grad_proj are zero here, as the broadcast copies them into the volume
    gp0 = np.zeros_like(gp)
    gp0[py0 + lo:py0 + hi, px0:px0 + X] = c.cot[lo:hi]
    d_gp0, d_vol, d_two = ctx.array(gp0), ctx.array(np.zeros(plan.rot_shape, np.float32)), ctx.array(g0)
    check(ctx.lib.adm_project_z_adj(plan.handle, d_gp0.ptr, lo, hi, d_vol.ptr))
    if tables is not None:
        check(ctx.lib.adm_rotate_adj_csr(plan.handle, d_vol.ptr, tp[0], tp[1], tp[2], d_two.ptr, lo, hi, 0))
    else:
        check(ctx.lib.adm_rotate_adj(plan.handle, d_vol.ptr, None, d_two.ptr, lo, hi))
    return got, d_two.get()


@pytest.mark.parametrize('name', list(PM.CASES))
def test_fused_pair_vs_references(A, ctx, name):
    """Both directions of one row: bars 1 and 2 per range, bar 3 on the whole range (gradient into zeros), bar 4 inside the
    runners; a partial range goes into a non-zero gradient."""
    c = PM.case_refs(name)
    Y, X, Z = c.size
    plan = make_plan(ctx, c.size)
    d_coords = device_coords(ctx, c)
    tables = None
    if c.theta is not None:
        tables = [ctx.array(t) for t in RM.host_tables(c.size, c.theta, staged=False)]
    for lo, hi in c.ranges:
        what = '%s forward [%d, %d)' % (name, lo, hi)
        fwd, two = run_forward(ctx, plan, c, d_coords, lo, hi)
        worst = PM.check_fwd_bar1(fwd[lo:hi], c.fwd_S[lo:hi], c.fwd_bound[lo:hi], what)
        e, e32 = RM.check_bar2(fwd[lo:hi], c.fwd_64[lo:hi], c.fwd_32[lo:hi], what)
        same = np.mean(fwd[lo:hi].view(np.uint32) == two[lo:hi].view(np.uint32))
        print('%s: bar 1 reached %.2f; rel(gpu, f64) %.2e, rel(f32 oracle, f64) %.2e; %.4f of the elements equal the unfused pair\'s bits'
              % (what, worst, e, e32, same))
        whole = (lo, hi) == (0, Y)
        g0 = np.zeros_like(c.g0) if whole else c.g0
        what = '%s adjoint [%d, %d)' % (name, lo, hi)
        got, two = run_adjoint(ctx, plan, c, tables, lo, hi, g0)
        S, bound, f64, f32 = c.adjoint(g0)
        worst = RM.check_bar1(got[lo:hi], S[lo:hi], bound[lo:hi], what)
        e, e32 = RM.check_bar2(got[lo:hi], f64[lo:hi], f32[lo:hi], what)
        same = np.mean(got[lo:hi].view(np.uint32) == two[lo:hi].view(np.uint32))
        print('%s: bar 1 reached %.2f; rel(gpu, f64) %.2e, rel(f32 oracle, f64) %.2e; %.4f of the elements equal the unfused pair\'s bits'
              % (what, worst, e, e32, same))
        if whole:
            # <P R x, y> = <x, R^T P^T y>
            x64, y64 = c.obj.astype(np.float64), c.cot.astype(np.float64)
            lhs, rhs = np.sum(fwd.astype(np.float64) * y64), np.sum(x64 * got.astype(np.float64))
            tol = np.sum(np.abs(y64) * c.fwd_bound) + np.sum(np.abs(x64) * bound)
            assert abs(lhs - rhs) <= tol, '%s: <PRx, y> = %.17g, <x, (PR)^T y> = %.17g, difference %.3e > %.3e' % (name, lhs, rhs, abs(lhs - rhs), tol)
    plan.close()


def test_bad_arguments_are_refused(A, ctx):
    """Null pointers, tables that do not come together and bad ranges: ADM_ERR_INVALID (ValueError), nothing launched; an empty range
    is a no-op."""
    from adorym_amd._lib import check
    size = (3, 16, 7)
    plan = make_plan(ctx, size)
    Yp, Xp, _, _ = RM.frame(size)
    d_obj = ctx.array(np.zeros(size + (2,), np.float32))
    d_proj = ctx.array(np.full((Yp, Xp, 2), RM.SENTINEL, np.float32))
    lib, h = ctx.lib, plan.handle
    check(lib.adm_rotate_project_fwd(h, d_obj.ptr, None, d_proj.ptr, 2, 2))
    check(lib.adm_rotate_project_adj(h, d_proj.ptr, None, None, None, d_obj.ptr, 2, 2, 0))
    for lo, hi in ((-1, 2), (0, 4), (2, 1)):
        with pytest.raises(ValueError, match='bad y range'):
            check(lib.adm_rotate_project_fwd(h, d_obj.ptr, None, d_proj.ptr, lo, hi))
        with pytest.raises(ValueError, match='bad y range'):
            check(lib.adm_rotate_project_adj(h, d_proj.ptr, None, None, None, d_obj.ptr, lo, hi, 0))
    for args in ((None, d_obj.ptr, None, d_proj.ptr), (h, None, None, d_proj.ptr), (h, d_obj.ptr, None, None)):
        with pytest.raises(ValueError, match='null argument'):
            check(lib.adm_rotate_project_fwd(*(args + (0, 3))))
    for args in ((None, d_proj.ptr, None, None, None, d_obj.ptr), (h, None, None, None, None, d_obj.ptr), (h, d_proj.ptr, None, None, None, None)):
        with pytest.raises(ValueError, match='null argument'):
            check(lib.adm_rotate_project_adj(*(args + (0, 3, 0))))
    with pytest.raises(ValueError, match='come together'):
        check(lib.adm_rotate_project_adj(h, d_proj.ptr, d_obj.ptr, None, None, d_obj.ptr, 0, 3, 0))
    assert RM.same_bits(d_proj.get(), np.full((Yp, Xp, 2), RM.SENTINEL, np.float32))
    plan.close()
