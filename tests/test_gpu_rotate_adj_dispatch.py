"""How adm_rotate_adj_staged hands out its blocks leaves the bits alone (pytest -m gpu).

The staged adjoint walks a 1-D grid: the border ring of the 16 x 16 patch grid first, two blocks per ring patch and group of
four planes (a rim patch's halves take planes [0, 2) and [2, 4) of the group; any other ring patch does all four in its first
block), then the inside.  Whatever the order and the split, every voxel's sum is the one adm_rotate_adj_csr forms with
lanes_along_x = 0 -- the CSR row in order, from zero, one fused multiply-add per entry, then added to the gradient -- so the two
agree bit for bit.  Fields, pads and poison as in tests/test_gpu_rotate_adj_bits.py.

  plane splits   an (80, 48) plane at pi/4 (one-plane rim passes, `rim1`) and a (37, 53) plane at 0.3 rad (two-plane rim
                 passes, `rim2`), every range [lo, hi) with lo in 0..3 and hi - lo in 1..7: the last group of a range holds 1 - 4
                 planes, so a rim block's second half sees 0, 1 and 2 of them.  Y = 10, not 9: lo = 3 with seven planes ends at 10.
  all border     patch grids of 1 x 1, 1 x 3 and 2 x 2: no inside at all; a patch visited twice or never shows as other bits.
  5 x 4 grid     a ring of 14 around an inside of 3 x 2: neither count divides the other, at pi/4.
  determinism    two launches on the same inputs give the same bits.
No case for interior boxes around a one-iteration staging limit: that lever (RB = 3 up to 768 elements) was not built.
"""
import numpy as np
import pytest

from tests import rot_matrix as RM
from tests.test_gpu_rotation_matrix import make_plan

pytestmark = pytest.mark.gpu

SPLITS = {'rim1': ((10, 80, 48), np.pi / 4), 'rim2': ((10, 37, 53), 0.3)}
RANGES = [(lo, lo + n) for lo in range(4) for n in range(1, 8)]
BORDER_SIZES = {(5, 16, 16): (1, 1), (5, 12, 40): (1, 3), (5, 32, 32): (2, 2)}       # size: (nx, nz) of its patch grid


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


class Case(object):
    """Plan, tables and fields of one (size, angle); launch() runs both adjoints over [lo, hi) from `start`."""

    def __init__(self, A, ctx, name, size, theta):
        self.ctx, self.name, self.size = ctx, name, size
        _, self.cot, self.g0 = RM.fields(name, size)
        self.plan = make_plan(ctx, size)
        self.tab = A.RotationTable(ctx, size, np.float32(theta))
        self.tables = self.tab.csr(self.plan)

    def staged(self, d_grot, start, lo, hi):
        from adorym_amd._lib import check
        p, s, ls, w, b = self.tables
        d = self.ctx.array(start)
        check(self.ctx.lib.adm_rotate_adj_staged(self.plan.handle, d_grot.ptr, p.ptr, s.ptr, ls.ptr, w.ptr, b.ptr, d.ptr, lo, hi))
        return d.get()

    def csr(self, d_grot, start, lo, hi):
        from adorym_amd._lib import check
        p, s, ls, w, b = self.tables
        d = self.ctx.array(start)
        check(self.ctx.lib.adm_rotate_adj_csr(self.plan.handle, d_grot.ptr, p.ptr, s.ptr, w.ptr, d.ptr, lo, hi, 0))
        return d.get()

    def compare(self, lo, hi):
        d_grot = self.ctx.array(_grot(self.cot, self.size, lo, hi))
        for start in (np.zeros_like(self.g0), self.g0):
            ref, got = self.csr(d_grot, start, lo, hi), self.staged(d_grot, start, lo, hi)
            assert np.isfinite(ref).all(), '%s [%d, %d): the CSR gather read a pad or a plane outside the range' % (self.name, lo, hi)
            assert not RM.same_bits(ref[lo:hi], start[lo:hi])           # (the reference did add something)
            diff = np.ascontiguousarray(ref).view(np.uint32) != np.ascontiguousarray(got).view(np.uint32)
            if diff.any():
                y, x, z, c = [int(v[0]) for v in np.nonzero(diff)]
                raise AssertionError('%s [%d, %d) into %s: %d elements differ from adm_rotate_adj_csr; first (y, x, z, c) = (%d, %d, %d, %d), '
                                     'patch (%d, %d): staged %r, csr %r' % (self.name, lo, hi, 'a non-zero gradient' if start.any() else 'zeros',
                                                                             diff.sum(), y, x, z, c, x // 16, z // 16, got[y, x, z, c],
                                                                             ref[y, x, z, c]))

    def close(self):
        self.plan.close()


@pytest.mark.parametrize('cls', list(SPLITS))
def test_plane_splits_of_rim_blocks(A, ctx, cls):
    size, theta = SPLITS[cls]
    classes, _, _ = RM.patch_classes(size, theta)
    assert cls in classes, (cls, sorted(set(classes)))
    nx, nz = (size[1] + 15) // 16, (size[2] + 15) // 16
    assert nx > 2 and nz > 2                                            # a patch grid with an inside
    ring = [k for k in range(nx * nz) if k % nx in (0, nx - 1) or k // nx in (0, nz - 1)]
    assert all(c == 'interior' for k, c in enumerate(classes) if k not in ring), 'a rim patch off the border ring'
    case = Case(A, ctx, 'split_' + cls, size, theta)
    assert max(hi for _, hi in RANGES) == size[0]
    for lo, hi in RANGES:
        case.compare(lo, hi)
    case.close()


@pytest.mark.parametrize('theta', [0.3, np.pi / 4], ids=['t0.3', 'pi4'])
@pytest.mark.parametrize('size', list(BORDER_SIZES), ids=lambda s: 'x%dz%d' % s[1:])
def test_patch_grids_that_are_all_border(A, ctx, size, theta):
    assert ((size[1] + 15) // 16, (size[2] + 15) // 16) == BORDER_SIZES[size]
    case = Case(A, ctx, 'border_x%dz%d' % size[1:], size, theta)
    case.compare(0, size[0])
    case.compare(1, size[0])
    case.close()


def test_patch_grid_of_5_by_4(A, ctx):
    size = (6, 80, 64)
    nx, nz = (size[1] + 15) // 16, (size[2] + 15) // 16
    assert (nx, nz) == (5, 4)
    case = Case(A, ctx, 'x80z64', size, np.pi / 4)
    case.compare(0, size[0])
    case.compare(1, size[0])
    case.close()


@pytest.mark.parametrize('cls', list(SPLITS))
def test_two_launches_give_the_same_bits(A, ctx, cls):
    size, theta = SPLITS[cls]
    case = Case(A, ctx, 'twice_' + cls, size, theta)
    d_grot = ctx.array(_grot(case.cot, size, 1, size[0]))
    first, second = case.staged(d_grot, case.g0, 1, size[0]), case.staged(d_grot, case.g0, 1, size[0])
    assert RM.same_bits(first, second)
    assert RM.same_bits(first[:1], case.g0[:1]) and not RM.same_bits(first[1:], case.g0[1:])
    case.close()
