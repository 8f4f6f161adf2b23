"""The overlap-add of the per-position tile gradients -- cover_build_kernel, tile_accumulate_kernel (adm_overlap_add.hip) and the host
code around them: tile_geom, the key cache of the lists built ahead, the window / part form, the range passes and the overflow
flag -- called through the C ABI and compared BIT FOR BIT with the float32 host reference of tests/oa_matrix.py
(pytest -m gpu).  Every comparison is an equality of uint32 views; there is no tolerance anywhere in this module.

A synthetic case creates a plan, allocates a workspace of adm_plan_workspace_bytes, uploads seeded tile gradients into the gtile
section in the mirrored element order, fills grad_rot with a finite sentinel pattern, calls adm_tile_grad_accumulate[_part |
_range] / adm_tile_cover_build / adm_tile_grad_status and compares the whole of grad_rot with the reference computed from the
same sentinel: the rows written must hold the reference's bits and every other word the sentinel's.  The producer test ties the
mirrored layout to the real multislice kernels.  tests/test_overlap_add_coverage.py checks on the CPU that the mirror follows
the sources and that the tables reach what the case names say, and that a wrong order of additions would show.

Left out: the refusal "batch too large for 32-bit tile offsets" and tile offsets near 2^31 -- they need a tile-gradient section
of 16 GB or more; the speed of the overlap-add; the rotation adjoint behind it (tests/test_gpu_rotation_matrix.py).
"""
import ctypes as C

import numpy as np
import pytest

from tests import oa_matrix as OA
from tests import ms_matrix as MM

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


def INVALID():
    from adorym_amd import _lib
    return _lib.ADM_ERR_INVALID


def same_bits(got, ref, what, mask=None):
    """Equality of the uint32 views (``mask`` [Yp, Xp]: of these pixels only); prints the count before it asserts."""
    d = OA.bits(got) != OA.bits(ref)
    if mask is not None:
        d &= np.asarray(mask, bool)[None, :, :, None]
    n = int(d.sum())
    print('%s: %d of %d words differ' % (what, n, d.size))
    assert n == 0, (what, n, [tuple(int(v) for v in i) for i in np.argwhere(d)[:4]])


class Rig(object):
    """A plan of a case's geometry, positions on the device, a workspace (of ``ws_batch`` positions) and grad_rot filled with the
    sentinel."""

    def __init__(self, A, ctx, c, ws_batch=None, n_ws=1):
        self.ctx, self.lib, self.c, self.g = ctx, ctx.lib, c, c['geom']
        shape = OA.probe_shape(c['P'])
        self.plan = A.Plan(ctx, c['obj'], shape, c['pads'], 1.0, np.ones(shape, complex), binning=c['binning'])
        assert tuple(self.plan.rot_shape) == (self.g.Z, self.g.Yp, self.g.Xp, 2)
        self.h = self.plan.handle
        self.ws_batch = ws_batch or len(c['pos'])
        self.wss = [ctx.empty((self.plan.workspace_bytes(self.ws_batch),), np.uint8) for _ in range(n_ws)]
        self.ws = self.wss[0]
        self.before = OA.sentinel(self.g)
        self.grad = ctx.array(self.before)
        self.pos_host = np.ascontiguousarray(c['pos'], np.int32)
        self.pos = ctx.array(self.pos_host)
        self.tiles = None

    def upload(self, tiles, ws=None, batch=None):
        """Tile gradients [B, n_steps, Py, Px, 2] into the gtile section of a workspace laid out for ``batch`` positions."""
        g, ws = self.g, ws or self.ws
        B = batch or len(tiles)
        raw = OA.pack_gtile(g, tiles)
        off = OA.gtile_byte_offset(B, 1, g.n_steps, g.row_elems)
        assert off + raw.nbytes <= ws.nbytes
        ws.view(off, (raw.nbytes,)).set(raw.reshape(-1).view(np.uint8))
        self.tiles = tiles
        return tiles

    def refill(self, before=None):
        self.before = OA.sentinel(self.g) if before is None else before
        self.grad.set(self.before)

    def accumulate(self, ws=None, pos=None, pos_host=None, window=(0, 0), add=0, batch=None, nbytes=None):
        ws, pos, pos_host = ws or self.ws, pos or self.pos, self.pos_host if pos_host is None else pos_host
        return self.lib.adm_tile_grad_accumulate_part(self.h, ws.ptr, ws.nbytes if nbytes is None else nbytes, pos.ptr,
                                                      len(pos_host) if batch is None else batch, pos_host.ctypes.data, self.grad.ptr,
                                                      window[0], window[1], add)

    def build(self, ws=None, pos=None, pos_host=None, window=(0, 0), add=0, batch=None):
        ws, pos, pos_host = ws or self.ws, pos or self.pos, self.pos_host if pos_host is None else pos_host
        return self.lib.adm_tile_cover_build(self.h, ws.ptr, ws.nbytes, pos.ptr, len(pos_host) if batch is None else batch,
                                             pos_host.ctypes.data, window[0], window[1], add)

    def range_pass(self, lo, hi, add, ws=None, batch=None):
        ws = ws or self.ws
        return self.lib.adm_tile_grad_accumulate_range(self.h, ws.ptr, ws.nbytes, self.pos.ptr, len(self.pos_host) if batch is None else batch,
                                                       self.pos_host.ctypes.data, self.grad.ptr, lo, hi, add)

    def status(self, batch=None, ws=None):
        ws = ws or self.ws
        ov = C.c_int(-7)
        assert self.lib.adm_tile_grad_status(self.h, ws.ptr, ws.nbytes, batch or len(self.pos_host), C.byref(ov)) == 0, self.lib.adm_last_error()
        return ov.value

    def got(self):
        return self.grad.get()

    def close(self):
        self.plan.close()


def run_whole(A, ctx, c, name):
    """One call of adm_tile_grad_accumulate on a synthetic case against the reference; returns (rig, got, ref, cover)."""
    rig = Rig(A, ctx, c)
    t = rig.upload(OA.case_values(c))
    assert rig.lib.adm_tile_grad_accumulate(rig.h, rig.ws.ptr, rig.ws.nbytes, rig.pos.ptr, len(c['pos']), rig.pos_host.ctypes.data,
                                            rig.grad.ptr) == 0, rig.lib.adm_last_error()
    got = rig.got()
    ref, cover = OA.overlap_add_ref(t, c['pos'], c['geom'], rig.before)
    return rig, got, ref, cover


def outside_rows_hold_the_sentinel(rig, got, rows, what):
    r0, r1 = rows
    keep = np.ones(rig.g.Yp, bool)
    keep[r0:r1] = False
    assert keep.any(), what                     # (every case leaves padded rows outside what it writes)
    n = int((OA.bits(got[:, keep]) != OA.bits(rig.before[:, keep])).sum())
    print('%s: %d words outside rows [%d, %d) lost the sentinel' % (what, n, r0, r1))
    assert n == 0, what


# ---- (a) the producer ties the mirror to the real kernels -----------------------------------------------------------------------
@pytest.mark.parametrize('P,kind', OA.PRODUCER_CASES, ids=['%s-%s' % (('%dx%d' % OA.probe_shape(P)), k) for P, k in OA.PRODUCER_CASES])
def test_producer_real_tile_gradients_overlap_add_to_grad_rot(A, ctx, P, kind):
    """The real multislice at B = 11, S = 3 with positions over all four edges: the gtile section read back through the mirrored
    layout and overlap-added by the reference equals the engine's grad_rot bit for bit.  A wrong offset or permutation in the
    mirror fails grossly here, so the synthetic cases rest on a checked layout."""
    B, S = 11, 3
    obj, pos, probe, target = OA.producer_inputs(P, S=S, B=B, seed=5)
    shape = OA.probe_shape(P)
    eng = A.MultisliceEngine(ctx, obj.shape[:3], shape, pos, OA.ENERGY_EV, OA.PSIZE_CM, max_batch=B, generic=(kind == 'generic'),
                             streamed=(kind == 'streamed'))
    assert eng.streamed == (kind == 'streamed')
    g = OA.make_geom(obj.shape[:3], P, eng.pads, 1, pixel_major=(kind != 'tuned'))
    assert tuple(eng.plan.rot_shape) == (g.Z, g.Yp, g.Xp, 2) and g.pad_y0 > 0 and g.pad_x0 > 0
    eng.set_batch(pos, target)
    eng.rotate(ctx.array(obj, np.float32), None)
    d_probe, d_gp = ctx.array(MM.c2(probe[None])), ctx.zeros((1,) + shape + (2,))
    eng.multislice(d_probe, grad_probe=d_gp)
    got = eng.grad_rot.get()
    raw = eng._ws.get()
    off = OA.gtile_byte_offset(B, 1, g.n_steps, g.row_elems)
    t = OA.unpack_gtile(g, raw[off:off + B * g.n_steps * g.row_elems * 8], B)
    assert np.isfinite(t).all() and (np.abs(t).max(axis=(1, 2, 3, 4)) > 0).all()
    ref, cover = OA.overlap_add_ref(t, eng._pos_host, g, np.zeros(eng.plan.rot_shape, np.float32))
    assert cover.max() >= 3 and np.abs(ref).max() > 0
    same_bits(got, ref, 'producer %s %s' % (P, kind))
    eng.plan.close()


# ---- (b) steps and binning ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('name', list(OA.STEP_CASES))
def test_steps_and_binning(A, ctx, name):
    """n_steps 1, 2, 3, 16, 17, 33; Z = 7 binned by 3 and Z = 35 binned by 2: the full-chunk and the one-step branch, the second
    and third round of step chunks over the XCDs, the last bin cut by Z."""
    c = OA.STEP_CASES[name]
    rig, got, ref, cover = run_whole(A, ctx, c, name)
    same_bits(got, ref, name)
    outside_rows_hold_the_sentinel(rig, got, OA.rows_of(c['pos'], c['geom']), name)
    rig.close()


# ---- (c) cover counts ---------------------------------------------------------------------------------------------------------
def test_cover_counts_up_to_the_list_length_and_the_overflow_flag(A, ctx):
    """Pixels covered exactly 1, 3, 4, 5, 63 and 64 times are bitwise right and the status is 0; 65 tiles on one pixel raise the
    flag while every pixel covered at most 64 times is still right; the next batch of the same size on the same workspace brings
    the flag back to 0; a batch of 64 cannot overflow and reports 0 without the flag being maintained."""
    cases = OA.COVER_CASES
    rig = Rig(A, ctx, cases['upto64'], ws_batch=max(len(c['pos']) for c in cases.values()))
    g = rig.g
    for name in ('upto64', 'over65', 'after65', 'exactly64'):
        c = cases[name]
        assert c['geom'] == g
        B = len(c['pos'])
        rig.pos_host = np.ascontiguousarray(c['pos'])
        rig.pos = ctx.array(rig.pos_host)
        t = rig.upload(OA.case_values(c))
        rig.refill()
        flag = rig.ws.view(OA.overflow_byte_offset(B, 1, g.n_steps, g.row_elems, g.Yp, g.Xp), (4,))
        if B <= OA.MAXCOVER:
            flag.set(np.array([1], np.int32).view(np.uint8))           # (nobody looks at it or resets it for such a batch)
        assert rig.accumulate() == 0, rig.lib.adm_last_error()
        got = rig.got()
        ref, cover = OA.overlap_add_ref(t, c['pos'], g, rig.before)
        for n in c['named']:
            y, x = np.argwhere(cover == n)[0]
            if n <= OA.MAXCOVER:
                assert np.array_equal(OA.bits(got[:, y, x]), OA.bits(ref[:, y, x])), (name, n, y, x)
        same_bits(got, ref, name, mask=cover <= OA.MAXCOVER)
        outside_rows_hold_the_sentinel(rig, got, OA.rows_of(c['pos'], g), name)
        ov = rig.status()
        print('%s: B = %d, most-covered pixel %d, status %d' % (name, B, cover.max(), ov))
        assert ov == c['overflow'], (name, ov)
        word = int(flag.get().view(np.int32)[0])
        assert word == (1 if B <= OA.MAXCOVER else c['overflow']), (name, word)
    rig.close()


@pytest.mark.parametrize('name', ['exactly64', 'over65'])
def test_check_cover_is_the_reference_maximum(A, ctx, name):
    c = OA.COVER_CASES[name]
    eng = A.MultisliceEngine(ctx, c['obj'], (8, 8), c['pos'], OA.ENERGY_EV, OA.PSIZE_CM)
    _, cover = OA.partial_sums(OA.case_values(c), c['pos'], c['geom'])
    assert eng._check_cover(np.ascontiguousarray(c['pos'])) == cover.max() == len(c['pos'])
    eng.plan.close()


# ---- (d) large batches and the order of additions -----------------------------------------------------------------------------
@pytest.mark.parametrize('name', list(OA.LARGE_CASES))
def test_large_batches_add_in_position_order(A, ctx, name):
    """256, 257 and 513 positions (one, two and three 256-position chunks of cover_build_kernel, four waves each): the order pixels
    -- covered from every chunk and from several waves, where another order gives other bits (asserted by the coverage test) --
    and everything else bitwise."""
    c = OA.LARGE_CASES[name]
    rig, got, ref, cover = run_whole(A, ctx, c, name)
    assert cover.max() <= OA.MAXCOVER
    for y, x in OA.order_pixels(c):
        assert np.array_equal(OA.bits(got[:, y, x]), OA.bits(ref[:, y, x])), (name, 'order pixel', y, x, int(cover[y, x]))
    same_bits(got, ref, name)
    outside_rows_hold_the_sentinel(rig, got, OA.rows_of(c['pos'], c['geom']), name)
    assert rig.status() == 0
    rig.close()


# ---- (e) frame geometry -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('name', list(OA.FRAME_CASES))
def test_frame_geometry(A, ctx, name):
    """Xp 31, 32, 33, 65, row windows that are and are not multiples of 8, positions over all four edges, a tuned size with
    LPW = 7, one with odd R1, the generic 40 x 24 field on a non-square frame."""
    c = OA.FRAME_CASES[name]
    rig, got, ref, cover = run_whole(A, ctx, c, name)
    same_bits(got, ref, name)
    outside_rows_hold_the_sentinel(rig, got, OA.rows_of(c['pos'], c['geom']), name)
    rig.close()


# ---- (f) parts and windows ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('split', list(OA.PART_SPLITS))
def test_parts_of_a_batch_with_a_window(A, ctx, split):
    """The first part writes the whole window (two rows more than the batch on either side), the others add on their own rows:
    the reference's part-ordered sums, zeros in the window rows no part reaches, the sentinel outside the window."""
    c, parts = OA.PART_CASE, OA.PART_SPLITS[split]
    g, win = c['geom'], OA.part_window(c)
    rig = Rig(A, ctx, c, n_ws=len(parts))
    t = OA.case_values(c)
    for i, (o, n) in enumerate(parts):
        rig.upload(t[o:o + n], ws=rig.wss[i])
    for i, (o, n) in enumerate(parts):
        host = np.ascontiguousarray(c['pos'][o:o + n])
        rc = rig.accumulate(ws=rig.wss[i], pos=rig.pos.view(2 * o, (n, 2)), pos_host=host, window=win if i == 0 else (0, 0), add=1 if i else 0)
        assert rc == 0, rig.lib.adm_last_error()
    got = rig.got()
    ref, _ = OA.parts_ref(t, c['pos'], g, rig.before, parts, win)
    same_bits(got, ref, 'parts ' + split)
    w0, w1 = win[0] + g.pad_y0, win[1] + g.pad_y0
    r0, r1 = OA.rows_of(c['pos'], g)
    assert (OA.bits(got[:, w0:r0]) == 0).all() and (OA.bits(got[:, r1:w1]) == 0).all()
    outside_rows_hold_the_sentinel(rig, got, (w0, w1), 'parts ' + split)
    rig.close()


def test_parts_refuse_bad_arguments(A, ctx):
    c = OA.PART_CASE
    g, pos = c['geom'], c['pos']
    rig = Rig(A, ctx, c)
    rig.upload(OA.case_values(c))
    last = lambda: rig.lib.adm_last_error()
    y0, y1 = int(pos[:, 0].min()), int(pos[:, 0].max()) + g.Py
    for win in ((y0 + 1, y1), (y0, y1 - 1)):                                  # a window that does not contain the part's rows
        assert rig.accumulate(window=win) == INVALID() and b'window' in last()
        assert rig.build(window=win) == INVALID()
    for dy in (OA.y_range(g)[1] + 1 - y1 + g.Py, OA.y_range(g)[0] - 1 - y0):   # one row below / above the padded frame
        bad = np.ascontiguousarray(pos + np.array([dy, 0], np.int32))
        assert rig.accumulate(pos_host=bad) == INVALID() and b'outside the padded frame' in last()
    assert rig.accumulate(nbytes=rig.plan.workspace_bytes(len(pos)) - 1) == INVALID() and b'workspace too small' in last()
    for batch in (0, -1):
        assert rig.accumulate(batch=batch) == INVALID() and b'batch must be positive' in last()
        assert rig.build(batch=batch) == INVALID()
    # none of them wrote anything or left a key behind
    same_bits(rig.got(), rig.before, 'after the refusals')
    assert rig.accumulate() == 0
    same_bits(rig.got(), OA.overlap_add_ref(rig.tiles, pos, g, rig.before)[0], 'a good call after the refusals')
    rig.close()


@pytest.mark.parametrize('n_cu', [4, 2])
def test_engine_rounds_of_multislice_overlapped(A, ctx, n_cu):
    """MultisliceEngine.multislice_overlapped with N_CU forced small (11 positions in 3 rounds, lists built ahead on the side
    stream; in 6 rounds, lists built by each overlap-add): every round's gtile read back, the reference in the engine's round
    order (equal_parts) equals grad_rot bitwise."""
    from adorym_amd.propagate import equal_parts
    P, B, S = 16, 11, 3
    obj, pos, probe, target = OA.producer_inputs(P, S=S, B=B, seed=6)
    eng = A.MultisliceEngine(ctx, obj.shape[:3], (P, P), pos, OA.ENERGY_EV, OA.PSIZE_CM, max_batch=B)
    eng.N_CU = n_cu
    g = OA.make_geom(obj.shape[:3], P, eng.pads)
    eng.set_batch(pos, target)
    eng.rotate(ctx.array(obj, np.float32), None)
    d_probe, d_gp = ctx.array(MM.c2(probe[None])), ctx.zeros((1, P, P, 2))
    eng.multislice_overlapped(d_probe, grad_probe=d_gp)
    got = eng.grad_rot.get()
    parts = equal_parts(B, n_cu)
    assert len(parts) == {4: 3, 2: 6}[n_cu] and len(eng._ws_parts) >= len(parts)
    t = []
    for i, (o, n) in enumerate(parts):
        raw = eng._ws_parts[i].get()
        off = OA.gtile_byte_offset(n, 1, g.n_steps, g.row_elems)
        t.append(OA.unpack_gtile(g, raw[off:off + n * g.n_steps * g.row_elems * 8], n))
    t = np.concatenate(t)
    assert np.isfinite(t).all() and (np.abs(t).max(axis=(1, 2, 3, 4)) > 0).all()
    window = (int(pos[:, 0].min()), int(pos[:, 0].max()) + P)
    ref, cover = OA.parts_ref(t, eng._pos_host, g, np.zeros(eng.plan.rot_shape, np.float32), parts, window)
    assert cover.max() >= 3
    same_bits(got, ref, 'multislice_overlapped, N_CU = %d' % n_cu)
    eng.loss()                                                            # (reads the status of every round)
    eng.plan.close()


# ---- (g) lists built ahead ----------------------------------------------------------------------------------------------------
def _ahead_rig(A, ctx, n_ws):
    rig = Rig(A, ctx, OA.AHEAD_CASES[0], ws_batch=len(OA.AHEAD_LARGER['pos']), n_ws=n_ws)
    rig.dpos = [ctx.array(c['pos']) for c in OA.AHEAD_CASES]
    rig.vals = [OA.case_values(c) for c in OA.AHEAD_CASES]
    for ws, t in zip(rig.wss, rig.vals):
        rig.upload(t, ws=ws)
    return rig


def _ahead_check(rig, i, what, pos=None, values=None):
    """grad_rot against the whole-batch reference of ahead case i (or of other positions with the values of workspace i)."""
    c = OA.AHEAD_CASES[i]
    ref, _ = OA.overlap_add_ref(rig.vals[i] if values is None else values, c['pos'] if pos is None else pos, rig.g, rig.before)
    same_bits(rig.got(), ref, what)


def test_lists_built_ahead_and_a_rewritten_position_buffer(A, ctx):
    """Build then accumulate; build, then the SAME device buffer and host array rewritten with other positions, then accumulate
    (the fingerprint voids the key: the result is the new positions'); build with another batch size or another window, then
    accumulate; build, then range passes, then a one-pass accumulate on that workspace."""
    rig = _ahead_rig(A, ctx, 1)
    c0, c1 = OA.AHEAD_CASES[0], OA.AHEAD_CASES[1]
    err = rig.lib.adm_last_error
    # accumulate alone, then build + accumulate: the same bits
    assert rig.accumulate(pos=rig.dpos[0], pos_host=c0['pos']) == 0, err()
    alone = rig.got()
    _ahead_check(rig, 0, 'accumulate alone')
    rig.refill()
    assert rig.build(pos=rig.dpos[0], pos_host=c0['pos']) == 0, err()
    assert rig.accumulate(pos=rig.dpos[0], pos_host=c0['pos']) == 0, err()
    same_bits(rig.got(), alone, 'build + accumulate against accumulate alone')
    # the position buffer and the host array rewritten between the build and the accumulate
    host = np.array(c0['pos'], np.int32, copy=True)
    dev = ctx.array(host)
    rig.refill()
    assert rig.build(pos=dev, pos_host=host) == 0, err()
    dev.set(c1['pos'])
    host[:] = c1['pos']
    assert rig.accumulate(pos=dev, pos_host=host) == 0, err()
    _ahead_check(rig, 0, 'positions rewritten after the build', pos=c1['pos'])
    # ... and back again with the lists of the second positions built ahead
    rig.refill()
    assert rig.build(pos=dev, pos_host=host) == 0, err()
    dev.set(c0['pos'])
    host[:] = c0['pos']
    assert rig.accumulate(pos=dev, pos_host=host) == 0, err()
    _ahead_check(rig, 0, 'positions rewritten back after a second build')
    # built for another batch size
    big = OA.AHEAD_LARGER
    dbig = ctx.array(big['pos'])
    rig.refill()
    assert rig.build(pos=dbig, pos_host=big['pos']) == 0, err()
    assert rig.accumulate(pos=rig.dpos[0], pos_host=c0['pos']) == 0, err()
    _ahead_check(rig, 0, 'built for 13 positions, accumulated for 11')
    # built for a part of the same buffer (same address, fewer positions)
    rig.refill()
    assert rig.build(pos=rig.dpos[0], pos_host=c0['pos'], batch=7) == 0, err()
    rig.upload(rig.vals[0])               # (a workspace laid out for 7 positions keeps its lists where 11 keep tile gradients)
    assert rig.accumulate(pos=rig.dpos[0], pos_host=c0['pos']) == 0, err()
    _ahead_check(rig, 0, 'built for the first 7 positions, accumulated for 11')
    # built for another window
    y = c0['pos'][:, 0]
    win = (int(y.min()) - 2, int(y.max()) + rig.g.Py + 1)
    rig.refill()
    assert rig.build(pos=rig.dpos[0], pos_host=c0['pos'], window=win) == 0, err()
    assert rig.accumulate(pos=rig.dpos[0], pos_host=c0['pos']) == 0, err()
    _ahead_check(rig, 0, 'built for a window, accumulated without')
    rig.refill()
    assert rig.build(pos=rig.dpos[0], pos_host=c0['pos']) == 0, err()
    assert rig.accumulate(pos=rig.dpos[0], pos_host=c0['pos'], window=win) == 0, err()
    same_bits(rig.got(), OA.overlap_add_ref(rig.vals[0], c0['pos'], rig.g, rig.before, 'first', window=win)[0], 'built without a window, accumulated with one')
    rig.refill()
    assert rig.build(pos=rig.dpos[0], pos_host=c0['pos'], window=win) == 0, err()
    assert rig.accumulate(pos=rig.dpos[0], pos_host=c0['pos'], window=win) == 0, err()
    same_bits(rig.got(), OA.overlap_add_ref(rig.vals[0], c0['pos'], rig.g, rig.before, 'first', window=win)[0], 'built and accumulated with a window')
    # a build, then range passes on that workspace (their lists replace the ones built), then the one-pass form again
    rig.refill()
    rig.pos, rig.pos_host = rig.dpos[0], np.ascontiguousarray(c0['pos'])
    passes = [(0, 6), (6, 11)]
    assert rig.build() == 0, err()
    for lo, hi in passes:
        assert rig.range_pass(lo, hi, 1 if lo else 0) == 0, err()
    same_bits(rig.got(), OA.overlap_add_ref(rig.vals[0], c0['pos'], rig.g, rig.before, 'range', passes=passes)[0], 'build, then range passes')
    rig.refill()
    assert rig.accumulate() == 0, err()
    _ahead_check(rig, 0, 'one pass after the range passes')
    rig.close()


def test_four_workspaces_built_ahead_and_a_fifth(A, ctx):
    """Four workspaces built ahead and consumed in reverse order; five built ahead (a key is evicted) and consumed in order."""
    rig = _ahead_rig(A, ctx, 5)
    err = rig.lib.adm_last_error
    for n, order in ((4, (3, 2, 1, 0)), (5, (0, 1, 2, 3, 4)), (5, (4, 0, 3, 1, 2))):
        for i in range(n):
            assert rig.build(ws=rig.wss[i], pos=rig.dpos[i], pos_host=OA.AHEAD_CASES[i]['pos']) == 0, err()
        for i in order:
            rig.refill()
            assert rig.accumulate(ws=rig.wss[i], pos=rig.dpos[i], pos_host=OA.AHEAD_CASES[i]['pos']) == 0, err()
            _ahead_check(rig, i, '%d built ahead, workspace %d' % (n, i))
    # a workspace whose lists were built for other positions than it is consumed with
    for i in range(4):
        assert rig.build(ws=rig.wss[i], pos=rig.dpos[i], pos_host=OA.AHEAD_CASES[i]['pos']) == 0, err()
    for i in range(4):
        j = (i + 1) % 4
        rig.refill()
        assert rig.accumulate(ws=rig.wss[i], pos=rig.dpos[j], pos_host=OA.AHEAD_CASES[j]['pos']) == 0, err()
        _ahead_check(rig, i, 'workspace %d built for positions %d, consumed with %d' % (i, i, j), pos=OA.AHEAD_CASES[j]['pos'])
    rig.close()


# ---- (h) range passes ---------------------------------------------------------------------------------------------------------
def test_range_passes_of_an_overcovered_batch(A, ctx):
    """150 positions, 70 of them on one pixel, in passes of 64 / 64 / 22 as MultisliceEngine._overlap_add runs them: the
    reference's pass-structured sum, the sentinel outside the batch's rows."""
    c = OA.RANGE_CASE
    g = c['geom']
    rig = Rig(A, ctx, c)
    t = rig.upload(OA.case_values(c))
    for lo, hi in OA.RANGE_PASSES:
        assert rig.range_pass(lo, hi, 1 if lo else 0) == 0, rig.lib.adm_last_error()
    got = rig.got()
    ref, cover = OA.overlap_add_ref(t, c['pos'], g, rig.before, 'range', passes=OA.RANGE_PASSES)
    assert cover.max() == 70
    same_bits(got, ref, 'range passes')
    outside_rows_hold_the_sentinel(rig, got, OA.rows_of(c['pos'], g), 'range passes')
    # the one-pass form of the same batch overflows its lists and says so; the pixels within the lists are right
    rig.refill()
    assert rig.accumulate() == 0
    assert rig.status() == 1
    whole, _ = OA.overlap_add_ref(t, c['pos'], g, rig.before)
    same_bits(rig.got(), whole, 'one pass over the overcovered batch', mask=cover <= OA.MAXCOVER)
    rig.close()


def test_range_passes_refuse_bad_ranges(A, ctx):
    c = OA.RANGE_CASE
    rig = Rig(A, ctx, c)
    rig.upload(OA.case_values(c))
    B = len(c['pos'])
    for lo, hi in ((0, 65), (10, 150), (5, 5), (9, 3), (-1, 10), (100, B + 1), (B, B + 1)):
        assert rig.range_pass(lo, hi, 0) == INVALID(), (lo, hi)
        assert rig.range_pass(lo, hi, 1) == INVALID(), (lo, hi)
    assert rig.range_pass(0, 10, 0, batch=0) == INVALID()
    same_bits(rig.got(), rig.before, 'after the refused ranges')
    rig.close()
