"""Every rotation entry point of the C ABI and every branch of its kernels (adm_rotate.hip, adm_rotcsr.hip) against reference S
under bar 1 (element-wise, derived) and the fp64 oracle under bar 2 (the 3x rule), with adjointness and bitwise canaries
(pytest -m gpu).  tests/rot_matrix.py holds the tables, the references and the bars;
tests/test_rotation_matrix_coverage.py proves on the CPU that the tables reach what the ids below name: the no-box branch
(`bw == 0`), both rim branches, the identity kernels, both lane orders of adm_rotate_adj_csr, npl = 1 / 2 / 4 of both stacked
forms.

Each row runs the whole y range (gradient into zeros: also the adjointness pair) and a partial range with y_lo > 0 and a
length that is no multiple of 4 (gradient into a non-zero buffer); the plans have pad_y0 = 3 and pad_x0 = 2.
"""
import numpy as np
import pytest

from tests import rot_matrix as RM

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
    """A bare plan of the case's geometry (no multislice engine, no transmission cache)."""
    from adorym_amd.device import Plan
    plan = Plan(ctx, size, (RM.P, RM.P), RM.pads_of(size), 1.0, np.ones((RM.P, RM.P), complex))
    Yp, Xp, py0, px0 = RM.frame(size)
    assert plan.rot_shape == (size[2], Yp, Xp, 2) and py0 > 0 and px0 > 0
    return plan


def run_forward(ctx, plan, c, d_coords, lo, hi):
    """adm_rotate_fwd of planes [lo, hi) into a buffer full of sentinels -> the rotated object [Y, X, Z, 2]; the sentinels
    everywhere else are checked here (bar 4)."""
    from adorym_amd._lib import check
    d_obj = ctx.array(c.obj)
    d_rot = ctx.array(np.full(plan.rot_shape, RM.SENTINEL, np.float32))
    check(ctx.lib.adm_rotate_fwd(plan.handle, d_obj.ptr, d_coords.ptr if d_coords is not None else None, d_rot.ptr, lo, hi))
    buf = d_rot.get()
    written = RM.frame_mask(c.size, lo, hi)
    assert RM.same_bits(buf[~written], np.full((~written).sum(), RM.SENTINEL, np.float32)), 'obj_rot written outside the range / in the pads'
    return RM.from_frame(buf, c.size)


def adjoint_launcher(A, ctx, plan, c, path, d_coords):
    """launch(d_grot, d_gobj, lo, hi) for one adjoint path, and what it must keep alive."""
    from adorym_amd._lib import check
    lib, h = ctx.lib, plan.handle
    if path == 'atomic':
        cp = d_coords.ptr if d_coords is not None else None
        return (lambda gr, go, lo, hi: check(lib.adm_rotate_adj(h, gr.ptr, cp, go.ptr, lo, hi))), None
    if path.startswith('csr_lanes'):
        ptr, src, w = RM.host_tables(c.size, c.theta, staged=False)
        keep = (ctx.array(ptr), ctx.array(src), ctx.array(w))
        lanes_x = int(path == 'csr_lanes_x')
        return (lambda gr, go, lo, hi: check(lib.adm_rotate_adj_csr(h, gr.ptr, keep[0].ptr, keep[1].ptr, keep[2].ptr, go.ptr, lo, hi,
                                                                      lanes_x))), keep
    assert path == 'staged'
    tab = A.RotationTable(ctx, c.size, np.float32(c.theta))              # table and CSR formed on the device
    p, s, ls, w, b = tab.csr(plan)
    return (lambda gr, go, lo, hi: check(lib.adm_rotate_adj_staged(h, gr.ptr, p.ptr, s.ptr, ls.ptr, w.ptr, b.ptr, go.ptr, lo, hi))), tab


def run_adjoint(ctx, plan, c, launch, lo, hi, g0, repeatable):
    """grad_obj = g0, then += R^T grad_rot over planes [lo, hi).  grad_rot holds 1e30 in its pads and outside the range; planes of
    grad_obj outside the range must keep their bits (bar 4); a deterministic path gives the same bits twice."""
    grot = RM.to_frame(c.cot, c.size, RM.POISON)
    grot[~RM.frame_mask(c.size, lo, hi)] = RM.POISON
    d_grot = ctx.array(grot)
    outs = []
    for _ in range(2 if repeatable else 1):
        d_g = ctx.array(g0)
        launch(d_grot, d_g, lo, hi)
        outs.append(d_g.get())
    got = outs[0]
    assert RM.same_bits(got[:lo], g0[:lo]) and RM.same_bits(got[hi:], g0[hi:]), 'grad_obj touched outside the y range'
    if repeatable:
        assert RM.same_bits(outs[0], outs[1]), 'a deterministic path gave different bits on its second run'
    return got


def device_coords(ctx, c):
    return None if c.coords is None else ctx.array(np.ascontiguousarray(c.coords).view(np.uint16))


def _fwd_id(name):
    size, theta, partial, y_chunk, _ = RM.CASES[name]
    return '%s-ychunk%d' % (name, y_chunk)


@pytest.mark.parametrize('name', list(RM.CASES), ids=[_fwd_id(n) for n in RM.CASES])
def test_forward_vs_references(A, ctx, name):
    """adm_rotate_fwd: rotate_fwd_kernel at y_chunk = 32 with a tail, 8, 2 and 1, with coords = NULL, and identity_fwd_kernel;
    whole and partial y range; bars 1, 2 and 4."""
    c = RM.case_refs(name)
    plan = make_plan(ctx, c.size)
    d_coords = device_coords(ctx, c)
    Y = c.size[0]
    for lo, hi in ((0, Y), c.partial):
        got = run_forward(ctx, plan, c, d_coords, lo, hi)
        what = '%s forward [%d, %d)' % (name, lo, hi)
        worst = RM.check_bar1(got[lo:hi], c.fwd_S[lo:hi], c.fwd_bound[lo:hi], what)
        e, e32 = RM.check_bar2(got[lo:hi], c.fwd_64[lo:hi], c.fwd_32[lo:hi], what)
        print('%s: bar 1 reached %.2f; rel(gpu, f64) %.2e, rel(f32 oracle, f64) %.2e' % (what, worst, e, e32))
    plan.close()


def _adj_cases():
    out = []
    for name, (size, theta, partial, y_chunk, classes) in RM.CASES.items():
        for path in RM.ADJ_PATHS:
            if theta is None and path != 'atomic':
                continue
            tag = '-' + '+'.join(k for k in RM.BOX_CLASSES if k in classes) if path == 'staged' else ''
            out.append(pytest.param(name, path, id='%s-%s%s' % (name, path, tag)))
    return out


@pytest.mark.parametrize('name,path', _adj_cases())
def test_adjoint_vs_references(A, ctx, name, path):
    """adm_rotate_adj (rotate_adj_kernel, identity_adj_kernel), adm_rotate_adj_csr in both lane orders (host-built tables) and
    adm_rotate_adj_staged (device-built tables: no-box, interior, two-plane and one-plane rim patches as the id says).  Whole
    range into zeros with the adjointness pair (bar 3), partial range into a non-zero gradient; bars 1, 2 and 4."""
    c = RM.case_refs(name)
    plan = make_plan(ctx, c.size)
    d_coords = device_coords(ctx, c)
    launch, keep = adjoint_launcher(A, ctx, plan, c, path, d_coords)
    Y = c.size[0]
    for (lo, hi), g0 in (((0, Y), np.zeros_like(c.g0)), (c.partial, c.g0)):
        got = run_adjoint(ctx, plan, c, launch, lo, hi, g0, repeatable=(path != 'atomic'))
        S, bound, f64, f32 = c.adjoint(g0)
        what = '%s %s [%d, %d)' % (name, path, lo, hi)
        worst = RM.check_bar1(got[lo:hi], S[lo:hi], bound[lo:hi], what)
        e, e32 = RM.check_bar2(got[lo:hi], f64[lo:hi], f32[lo:hi], what)
        print('%s: bar 1 reached %.2f; rel(gpu, f64) %.2e, rel(f32 oracle, f64) %.2e' % (what, worst, e, e32))
        if (lo, hi) == (0, Y):
            fwd = run_forward(ctx, plan, c, d_coords, 0, Y)
            RM.check_adjointness(fwd, got, c.obj, c.cot, c.fwd_bound, bound, what)
    del keep
    plan.close()


@pytest.mark.parametrize('name', RM.NOBOX_CASES, ids=['%s-nobox' % n for n in RM.NOBOX_CASES])
@pytest.mark.regression
def test_device_built_tables_equal_host_builder_at_nobox_cases(A, ctx, name):
    """adm_rotation_table_build + adm_rotation_csr_build where patches get no box (`too_big`: bw = 0, lsrc = 0): the fp16 table
    equal to the oracle's, ptr / src / lsrc / w / boxes equal to the host builder's (weights bit for bit)."""
    c = RM.case_refs(name)
    plan = make_plan(ctx, c.size)
    tab = A.RotationTable(ctx, c.size, np.float32(c.theta))
    assert np.array_equal(tab.coords.get().reshape(-1), np.ascontiguousarray(c.coords).view(np.uint16).reshape(-1))
    dev = [a.get() for a in tab.csr(plan)]
    ptr, src, lsrc, w, boxes = RM.host_tables(c.size, c.theta, staged=True)
    nnz = int(ptr[-1])
    assert (boxes[:, 2] == 0).any()
    assert np.array_equal(dev[0], ptr)
    assert np.array_equal(dev[1][:nnz], src)
    assert np.array_equal(dev[4].reshape(boxes.shape), boxes)
    assert np.array_equal(dev[2][:nnz], lsrc)
    assert RM.same_bits(dev[3][:nnz], w)
    cls, _, patch = RM.patch_classes(c.size, c.theta)
    rows = np.repeat(np.arange(len(ptr) - 1), np.diff(ptr))
    in_nobox = cls[patch[rows]] == 'nobox'
    assert in_nobox.any() and not dev[2][:nnz][in_nobox].any()
    plan.close()


@pytest.mark.parametrize('name', list(RM.STACK_CASES))
def test_stacked_rotations_vs_references(A, ctx, name):
    """adm_rotate_fwd_stack and adm_rotate_adj_staged_stack through the C ABI on a plan of R * Yb planes (as AngleBatch builds it):
    one block walking the angles (sequential) and the angles side by side + stack_sum_kernel (scratch), npl = 1, 2, 4 in each
    form, Yb % npl != 0, tables with no-box, two-plane and one-plane rim patches.  Bars 1 and 2 against the angles summed in
    float64, adjointness over the R angles, pads and bit-reproducibility."""
    from adorym_amd._lib import check
    from adorym_amd.device import DeviceArray
    Yb, scratch, npl = RM.STACK_CASES[name]
    s = RM.stack_refs(Yb)
    R, (X, Z) = s.R, RM.STACK_XZ
    assert RM.stack_npl(X, Z, Yb, R, scratch) == npl
    plan = make_plan(ctx, s.size)
    tabs = [A.RotationTable(ctx, s.real, np.float32(th)) for th in RM.STACK_THETAS]
    # forward: block r of the stacked frame = R_r obj
    d_tables = ctx.array(np.array([t.ptr for t in tabs], dtype=np.uint64))
    d_obj = ctx.array(s.obj)
    d_rot = ctx.array(np.full(plan.rot_shape, RM.SENTINEL, np.float32))
    check(ctx.lib.adm_rotate_fwd_stack(plan.handle, d_obj.ptr, d_tables.ptr, R, d_rot.ptr))
    buf = d_rot.get()
    pads = ~RM.frame_mask(s.size, 0, R * Yb)
    assert RM.same_bits(buf[pads], np.full(pads.sum(), RM.SENTINEL, np.float32)), 'obj_rot written in the pads'
    fwd = RM.from_frame(buf, s.size)
    RM.check_bar1(fwd, s.fwd_S, s.fwd_bound, name + ' forward')
    RM.check_bar2(fwd, s.fwd_64, s.fwd_32, name + ' forward')
    # adjoint: the one real gradient += sum over the angles
    parts = [t.csr(plan) for t in tabs]
    d_adj = ctx.array(np.array([[a.ptr for a in p] for p in parts], dtype=np.uint64))          # AdjTables: ptr, src, lsrc, w, boxes
    d_grot = ctx.array(RM.to_frame(s.cot, s.size, RM.POISON))
    d_scr = DeviceArray(ctx, (R * s.obj.size,), np.float32) if scratch else None
    for zero in (True, False):
        g0 = np.zeros_like(s.g0) if zero else s.g0
        outs = []
        for _ in range(2):
            d_g = ctx.array(g0)
            check(ctx.lib.adm_rotate_adj_staged_stack(plan.handle, d_grot.ptr, d_adj.ptr, R, d_g.ptr, d_scr.ptr if scratch else None,
                                                      d_scr.nbytes if scratch else 0))
            outs.append(d_g.get())
        assert RM.same_bits(outs[0], outs[1]), 'the stacked adjoint gave different bits on its second run'
        S, bound, f64, f32 = s.adjoint(zero)
        what = '%s adjoint into %s' % (name, 'zeros' if zero else 'a non-zero gradient')
        worst = RM.check_bar1(outs[0], S, bound, what)
        if zero:
            # sum_r <R_r x, y_r> = <x, sum_r R_r^T y_r>
            RM.check_adjointness(fwd, outs[0], s.obj, s.cot, s.fwd_bound, bound, what)
        else:
            e, e32 = RM.check_bar2(outs[0], f64, f32, what)
            print('%s: bar 1 reached %.2f; rel(gpu, f64) %.2e, rel(f32 oracle, f64) %.2e' % (what, worst, e, e32))
    plan.close()
