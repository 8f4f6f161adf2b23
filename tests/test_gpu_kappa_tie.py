"""The two kernels of the single-material constraint (adm_kappa_tie.hip) through the C ABI on the GPU (pytest -m gpu), against the
float32 mirrors of tests/fresnel_kappa_ref.py.

Tie and fold are bit for bit: kappa is formed in double and rounded once, the fold's product and sum are rounded separately.  The
sum S = sum_v delta_v g_beta_v is a double sum of exactly representable products (24 + 24 significant bits) in a fixed order; it is
held against math.fsum of the same products under the worst case of any order of n - 1 double additions,
(n - 1) * 2^-53 * sum |delta_v g_beta_v| -- derived, not measured -- and grad_lg_kappa against (float)(ln10 * kappa * S) of the S
the GPU left in scratch[0].

Sizes: the smallest at which each branch exists -- 1, 2, 3 voxels (a 16-byte access holds two), 511 / 512 / 513 (one thread short
of, at and past one access per thread of a workgroup), the first size with two workgroups, one past the grid cap (every thread
loops), a view that starts one voxel in (8-byte aligned only: the one-voxel accesses), a NULL grad_lg_kappa.
"""
import ctypes
import os
import re

import numpy as np
import pytest

from tests import fresnel_kappa_ref as KR

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _constants():
    """The walk's constants from the kernels' own sources: threads per workgroup, elements per thread until the cap, the cap."""
    with open(os.path.join(ROOT, 'adorym_amd', 'csrc', 'adm_optim.h')) as f:
        src = f.read()
    threads = int(re.search(r'#define FLAT_THREADS (\d+)', src).group(1))
    per = int(re.search(r'size_t b = \(n \+ (\d+) \* FLAT_THREADS - 1\) / \((\d+) \* FLAT_THREADS\);', src).group(1))
    with open(os.path.join(ROOT, 'include', 'adm.h')) as f:
        cap = int(re.search(r'#define ADM_CG_MAX_BLOCKS (\d+)', f.read()).group(1))
    return threads, per, cap


THREADS, PER_THREAD, MAX_BLOCKS = _constants()
FLOATS_PER_BLOCK = THREADS * PER_THREAD
TWO_BLOCKS = FLOATS_PER_BLOCK // 2 + 1                       # voxels: the first size whose 2 n floats need a second workgroup
PAST_CAP = MAX_BLOCKS * FLOATS_PER_BLOCK // 2 + 513          # ... and one the capped grid covers only by looping, with a ragged end
SMALL = (1, 2, 3, 511, 512, 513)
LG_KAPPAS = (-3., 0., 1.7, 3.)
bits = lambda a: np.ascontiguousarray(a, np.float32).view(np.uint32)


def grid(n_vox):
    b = (2 * n_vox + FLOATS_PER_BLOCK - 1) // FLOATS_PER_BLOCK
    return min(max(b, 1), MAX_BLOCKS)


def test_the_sizes_reach_what_they_name():
    assert (THREADS, PER_THREAD, MAX_BLOCKS) == (256, 16, 1024)
    assert grid(TWO_BLOCKS - 1) == 1 and grid(TWO_BLOCKS) == 2
    assert grid(PAST_CAP) == MAX_BLOCKS and PAST_CAP // 2 > MAX_BLOCKS * THREADS and PAST_CAP % 2 == 1
    assert 2 * THREADS in SMALL and 2 * THREADS - 1 in SMALL and 2 * THREADS + 1 in SMALL


@pytest.fixture(scope='module')
def A():
    import adorym_amd
    return adorym_amd


@pytest.fixture(scope='module')
def ctx(A):
    c = A.Context(0)
    yield c
    c.close()


def inputs(n, seed=0, cancel=False):
    """obj, grad_tied, grad_obj [n, 2] float32: deltas of both signs with exact zeros of both signs among them, gradients of both
    signs.  ``cancel``: the products delta_v g_beta_v come in pairs of opposite sign that differ in the last few bits, so that S is
    many orders below sum |delta_v g_beta_v|."""
    r = np.random.default_rng([n, seed, int(cancel)])
    obj = (1e-3 * r.standard_normal((n, 2))).astype(np.float32)
    obj[::7, 0] = 0.
    obj[3::11, 0] = -0.
    gt = r.standard_normal((n, 2)).astype(np.float32)
    go = r.standard_normal((n, 2)).astype(np.float32)
    if cancel and n > 1:
        h = n // 2
        obj[:, 0] = np.abs(obj[:, 0]) + np.float32(1e-4)
        obj[h:2 * h, 0] = obj[:h, 0]
        gt[h:2 * h, 1] = -gt[:h, 1] * np.float32(1 + 2. ** -18)
    return obj, gt, go


def dev(ctx, host, offset_voxels=0):
    """``host`` [n, 2] on the device; ``offset_voxels`` = 1: inside a larger allocation, one voxel in (8-byte aligned only)."""
    if not offset_voxels:
        return ctx.array(host, np.float32)
    n = host.shape[0]
    whole = ctx.array(np.concatenate([np.full((offset_voxels, 2), 7, np.float32), host]), np.float32)
    v = whole.view(2 * offset_voxels, (n, 2))
    v._keep = whole
    assert v.ptr % 16 == 8
    return v


def run_tie(ctx, obj, lg, offset=0):
    n = obj.shape[0]
    d_out = dev(ctx, np.full((n, 2), 5, np.float32), offset)
    d_obj, d_lg = dev(ctx, obj, offset), ctx.array(np.array([lg]), np.float32)         # (alive until the result has been read)
    rc = ctx.lib.adm_kappa_tie(ctx.handle, d_obj.ptr, d_lg.ptr, n, d_out.ptr)
    assert rc == 0
    return d_out.get()


def run_fold(ctx, A, obj, gt, go, lg, mode, offset=0, with_kappa=True, g0=0.25):
    from adorym_amd import _lib
    n = obj.shape[0]
    d_go = dev(ctx, go, offset)
    d_gk = ctx.array(np.array([g0]), np.float32)
    scratch = A.DeviceArray(ctx, (_lib.KAPPA_SCRATCH_DOUBLES,), np.float64)
    scratch.set(np.full(_lib.KAPPA_SCRATCH_DOUBLES, np.nan))
    d_obj, d_gt, d_lg = dev(ctx, obj, offset), dev(ctx, gt, offset), ctx.array(np.array([lg]), np.float32)      # (alive until read back)
    rc = ctx.lib.adm_kappa_fold(ctx.handle, d_obj.ptr, d_lg.ptr, d_gt.ptr, n, mode, d_go.ptr, d_gk.ptr if with_kappa else None,
                                scratch.ptr if with_kappa else None)
    assert rc == 0
    out = d_go.get(), d_gk.get()[0], scratch.get()
    del d_obj, d_gt, d_lg
    return out


def check_fold(ctx, A, n, lg, mode, offset=0, cancel=False, seed=0):
    obj, gt, go = inputs(n, seed, cancel)
    g0 = np.float32(0.25)
    got, gk, scratch = run_fold(ctx, A, obj, gt, go, lg, mode, offset, g0=g0)
    want = KR.fold(lg, gt, go, mode)
    assert np.array_equal(bits(got), bits(want)), ('grad_obj', n, lg, mode, int((bits(got) != bits(want)).sum()))
    if mode == 1:
        assert np.array_equal(bits(got[:, 1]), bits(go[:, 1]))
    else:
        assert np.array_equal(bits(got[:, 1]), np.zeros(n, np.uint32))
    S_gpu = float(scratch[0])
    S, scale = KR.fold_sum_exact(obj, gt)
    bound = (n - 1) * 2. ** -53 * scale
    print('n %d lg %g mode %d: S %.17g  |S_gpu - S| %.3e  bound %.3e  S / sum|.| %.1e' % (n, lg, mode, S, abs(S_gpu - S), bound, abs(S) / max(scale, 1e-300)))
    assert abs(S_gpu - S) <= bound, (S_gpu, S, bound)
    nb = grid(n)
    part = scratch[1:1 + nb]
    assert np.isfinite(part).all() and np.isnan(scratch[1 + nb:]).all()          # one partial per workgroup, none beyond
    t = 0.0
    for p in part:
        t += float(p)
    assert t == S_gpu                                                           # the partials in ascending order
    g = KR.grad_lg_kappa32(lg, S_gpu)
    want_gk = np.float32(g0 + g) if mode == 1 else g
    assert bits(np.array([gk]))[0] == bits(np.array([want_gk]))[0], (gk, want_gk)
    return got, gk, S_gpu


@pytest.mark.parametrize('n', SMALL + (TWO_BLOCKS,))
def test_tie_bit_for_bit(ctx, n):
    obj, _, _ = inputs(n)
    for lg in (1.7, -3.):
        got = run_tie(ctx, obj, lg)
        want = KR.tie(obj, lg)
        assert np.array_equal(bits(got), bits(want)), (n, lg)
        assert np.array_equal(bits(got[:, 0]), bits(obj[:, 0]))


@pytest.mark.parametrize('lg', LG_KAPPAS)
def test_tie_over_kappa_and_on_a_view(ctx, lg):
    obj, _, _ = inputs(513, seed=1)
    assert np.array_equal(bits(run_tie(ctx, obj, lg)), bits(KR.tie(obj, lg)))
    assert np.array_equal(bits(run_tie(ctx, obj, lg, offset=1)), bits(KR.tie(obj, lg)))


def test_tie_past_the_grid_cap(ctx):
    obj, _, _ = inputs(PAST_CAP, seed=2)
    assert np.array_equal(bits(run_tie(ctx, obj, 1.7)), bits(KR.tie(obj, 1.7)))


@pytest.mark.parametrize('mode', (1, 2))
@pytest.mark.parametrize('n', SMALL + (TWO_BLOCKS,))
def test_fold_bit_for_bit_and_the_sum(ctx, A, n, mode):
    check_fold(ctx, A, n, 1.7, mode)


@pytest.mark.parametrize('mode', (1, 2))
@pytest.mark.parametrize('lg', LG_KAPPAS)
def test_fold_over_kappa_on_a_view_and_with_cancellation(ctx, A, lg, mode):
    check_fold(ctx, A, 513, lg, mode, seed=3)
    check_fold(ctx, A, 513, lg, mode, offset=1, seed=3)               # the one-voxel accesses
    check_fold(ctx, A, 2 * TWO_BLOCKS, lg, mode, cancel=True, seed=4)
    obj, gt, _ = inputs(2 * TWO_BLOCKS, 4, True)
    S, scale = KR.fold_sum_exact(obj, gt)
    assert abs(S) < 1e-4 * scale                                         # (the sum nearly cancels)


@pytest.mark.parametrize('mode', (1, 2))
def test_fold_past_the_grid_cap_and_twice_the_same_bits(ctx, A, mode):
    a = check_fold(ctx, A, PAST_CAP, 1.7, mode, seed=5)
    obj, gt, go = inputs(PAST_CAP, 5)
    got, gk, scratch = run_fold(ctx, A, obj, gt, go, 1.7, mode, g0=np.float32(0.25))
    assert np.array_equal(bits(got), bits(a[0])) and bits(np.array([gk]))[0] == bits(np.array([a[1]]))[0]
    assert float(scratch[0]) == a[2]


@pytest.mark.parametrize('mode', (1, 2))
@pytest.mark.parametrize('offset', (0, 1))
def test_fold_without_the_kappa_gradient(ctx, A, mode, offset):
    obj, gt, go = inputs(TWO_BLOCKS + 1, seed=6)
    got, gk, _ = run_fold(ctx, A, obj, gt, go, 0., mode, offset, with_kappa=False)
    assert np.array_equal(bits(got), bits(KR.fold(0., gt, go, mode)))
    assert gk == np.float32(0.25)                                        # untouched


def test_refusals(ctx, A):
    from adorym_amd import _lib
    obj, gt, go = (ctx.array(a, np.float32) for a in inputs(4))
    lg = ctx.array(np.array([1.7]), np.float32)
    sc = A.DeviceArray(ctx, (_lib.KAPPA_SCRATCH_DOUBLES,), np.float64)
    lib, h = ctx.lib, ctx.handle
    assert lib.adm_kappa_fold(h, obj.ptr, lg.ptr, gt.ptr, 4, 3, go.ptr, None, None) == _lib.ADM_ERR_INVALID
    assert lib.adm_kappa_fold(h, obj.ptr, lg.ptr, gt.ptr, 0, 1, go.ptr, None, None) == _lib.ADM_ERR_INVALID
    assert lib.adm_kappa_fold(h, obj.ptr, lg.ptr, gt.ptr, 4, 1, go.ptr, lg.ptr, None) == _lib.ADM_ERR_INVALID
    assert lib.adm_kappa_fold(h, obj.ptr + 4, lg.ptr, gt.ptr, 2, 1, go.ptr, None, sc.ptr) == _lib.ADM_ERR_INVALID
    assert lib.adm_kappa_tie(h, obj.ptr, lg.ptr, 2, go.ptr + 4) == _lib.ADM_ERR_INVALID
    assert lib.adm_kappa_tie(h, None, lg.ptr, 2, go.ptr) == _lib.ADM_ERR_INVALID
    assert lib.adm_kappa_tie(h, obj.ptr, lg.ptr, 0, go.ptr) == 0
    ho = A.HomogeneousObject(ctx, (2, 2, 1, 2))
    assert ho.n_vox == 4 and ho.tie(obj, lg).shape == (2, 2, 1, 2) and ho.tied_grad().shape == (2, 2, 1, 2)
    with pytest.raises(ValueError, match='obj must be float32 of 8 values'):
        ho.tie(ctx.zeros((5, 2)), lg)
    with pytest.raises(ValueError, match='obj_shape must end in'):
        A.HomogeneousObject(ctx, (4, 4, 1))
