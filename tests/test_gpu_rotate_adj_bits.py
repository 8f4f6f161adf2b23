"""The LDS-staged rotation adjoint gives the bits of the plain CSR gather (pytest -m gpu).

adm_rotate_adj_staged adds, for every object voxel, the entries of its CSR row in CSR order, from zero, each with one fused
multiply-add, and then adds the sum to the gradient: the additions adm_rotate_adj_csr makes with lanes_along_x = 0.  However the
staged kernels batch their loads, the two must agree bit for bit -- on every rotated row of tests/rot_matrix.py's CASES (no-box,
interior, two-plane and one-plane rim patches; y ranges of length 1, 2 and 3 modulo 4), into a zero gradient and into a non-zero
one.  The stacked form (STACK_CASES: one block walking the angles, and the angles side by side + their sum) must give the bits of
R sequential staged launches on a plan of the real object.
"""
import numpy as np
import pytest

from tests import rot_matrix as RM
from tests.test_gpu_rotation_matrix import make_plan

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


def _grot(cot, size, lo, hi):
    """The padded rotated-frame cotangent; 1e30 in the pads and in the planes outside [lo, hi)."""
    g = RM.to_frame(cot, size, RM.POISON)
    g[~RM.frame_mask(size, lo, hi)] = RM.POISON
    return g


def _fields(name, size):
    """Float32 cotangent and initial gradient (no float64 reference is needed here, so not RM.case_refs)."""
    _, cot, g0 = RM.fields(name, size)
    return cot, g0


@pytest.mark.parametrize('name', RM.ROTATED)
def test_staged_equals_csr_gather_bit_for_bit(A, ctx, name):
    from adorym_amd._lib import check
    size, theta, partial, _, classes = RM.CASES[name]
    cot, g0 = _fields(name, size)
    plan = make_plan(ctx, size)
    tab = A.RotationTable(ctx, size, np.float32(theta))
    p, s, ls, w, b = tab.csr(plan)
    lib, h = ctx.lib, plan.handle
    Y = size[0]
    for (lo, hi), start in (((0, Y), np.zeros_like(g0)), (partial, g0), ((0, Y), g0), (partial, np.zeros_like(g0))):
        d_grot = ctx.array(_grot(cot, size, lo, hi))
        d_ref, d_got = ctx.array(start), ctx.array(start)
        check(lib.adm_rotate_adj_csr(h, d_grot.ptr, p.ptr, s.ptr, w.ptr, d_ref.ptr, lo, hi, 0))
        check(lib.adm_rotate_adj_staged(h, d_grot.ptr, p.ptr, s.ptr, ls.ptr, w.ptr, b.ptr, d_got.ptr, lo, hi))
        ref, got = d_ref.get(), d_got.get()
        assert np.isfinite(ref).all(), '%s [%d, %d): the CSR gather read a pad or a plane outside the range' % (name, lo, hi)
        assert not RM.same_bits(ref[lo:hi], start[lo:hi])           # (the reference did add something)
        diff = np.ascontiguousarray(ref).view(np.uint32) != np.ascontiguousarray(got).view(np.uint32)
        if diff.any():
            y, x, z, c = [int(v[0]) for v in np.nonzero(diff)]
            raise AssertionError('%s [%d, %d) into %s: %d elements differ from adm_rotate_adj_csr; first (y, x, z, c) = (%d, %d, %d, %d), '
                                 'patch (%d, %d): staged %r, csr %r' % (name, lo, hi, 'zeros' if not start.any() else 'a non-zero gradient',
                                                                         diff.sum(), y, x, z, c, x // 16, z // 16, got[y, x, z, c],
                                                                         ref[y, x, z, c]))
    plan.close()


@pytest.mark.parametrize('name', list(RM.STACK_CASES))
def test_stacked_equals_sequential_staged_launches_bit_for_bit(A, ctx, name):
    from adorym_amd._lib import check
    from adorym_amd.device import DeviceArray
    Yb, scratch, npl = RM.STACK_CASES[name]
    (X, Z), R = RM.STACK_XZ, len(RM.STACK_THETAS)
    real, stacked = (Yb, X, Z), (R * Yb, X, Z)
    assert RM.stack_npl(X, Z, Yb, R, scratch) == npl
    cot, _ = _fields('stackcot%d' % Yb, stacked)
    _, g0 = _fields('stack%d' % Yb, real)
    lib = ctx.lib
    # R sequential launches on a plan of the real object, angle r fed block r of the stacked cotangent
    plan1 = make_plan(ctx, real)
    tabs1 = [A.RotationTable(ctx, real, np.float32(th)) for th in RM.STACK_THETAS]
    refs = {}
    for zero in (True, False):
        d_ref = ctx.array(np.zeros_like(g0) if zero else g0)
        for r, t in enumerate(tabs1):
            p, s, ls, w, b = t.csr(plan1)
            d_blk = ctx.array(_grot(cot[r * Yb:(r + 1) * Yb], real, 0, Yb))
            check(lib.adm_rotate_adj_staged(plan1.handle, d_blk.ptr, p.ptr, s.ptr, ls.ptr, w.ptr, b.ptr, d_ref.ptr, 0, Yb))
        refs[zero] = d_ref.get()
        assert np.isfinite(refs[zero]).all()
    plan1.close()
    # the stacked launch
    plan = make_plan(ctx, stacked)
    tabs = [A.RotationTable(ctx, real, np.float32(th)) for th in RM.STACK_THETAS]
    parts = [t.csr(plan) for t in tabs]
    d_adj = ctx.array(np.array([[a.ptr for a in p] for p in parts], dtype=np.uint64))          # AdjTables: ptr, src, lsrc, w, boxes
    d_grot = ctx.array(RM.to_frame(cot, stacked, RM.POISON))
    d_scr = DeviceArray(ctx, (R * g0.size,), np.float32) if scratch else None
    for zero in (True, False):
        d_g = ctx.array(np.zeros_like(g0) if zero else g0)
        check(lib.adm_rotate_adj_staged_stack(plan.handle, d_grot.ptr, d_adj.ptr, R, d_g.ptr, d_scr.ptr if scratch else None,
                                              d_scr.nbytes if scratch else 0))
        got = d_g.get()
        diff = np.ascontiguousarray(refs[zero]).view(np.uint32) != np.ascontiguousarray(got).view(np.uint32)
        if diff.any():
            y, x, z, c = [int(v[0]) for v in np.nonzero(diff)]
            raise AssertionError('%s into %s: %d elements differ from %d sequential staged launches; first (y, x, z, c) = (%d, %d, %d, %d), '
                                 'patch (%d, %d): stacked %r, sequential %r' % (name, 'zeros' if zero else 'a non-zero gradient', diff.sum(), R,
                                                                                y, x, z, c, x // 16, z // 16, got[y, x, z, c],
                                                                                refs[zero][y, x, z, c]))
    plan.close()
