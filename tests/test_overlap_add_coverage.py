"""The overlap-add suite (tests/test_gpu_overlap_add.py) rests on tests/oa_matrix.py: a mirror of the workspace layout that
cover_build_kernel reads, a float32 reference of the overlap-add and the case tables.  This CPU test

  * parses the sources -- ADM_MAXCOVER, TA_STEPS, the 256-position chunk, the 32 x 8 pixel block and the XCD deal of
    tile_accumulate_kernel, ADM_FOR_EACH_SIZE, the order of the sections in ws_layout, the tid / k expressions of
    cover_build_kernel -- so that a change there fails here until the mirror follows,
  * checks the mirror (elem_offset injective into the row at every tuned size) and the reference (against the oracle's fp64
    scatter_tiles_adj within the recursive-summation bound; the cover counts against a brute-force count),
  * computes from the tables that the cases reach what their names say, and
  * asserts the discrimination condition: at every "order" pixel the sum in another order differs in bits, so that the GPU test
    cannot pass with a wrong order of additions."""
import os
import re

import numpy as np
import pytest

from tests import oa_matrix as OA
from tests.test_kernel_matrix_coverage import _function_body
from oracle import adorym_oracle as O      # checker only

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, 'adorym_amd', 'csrc')


def _read(name):
    with open(os.path.join(CSRC, name)) as f:
        return f.read()


def _flat(text):
    return re.sub(r'\s+', ' ', text)


def _define(src, name):
    m = re.search(r'^#define\s+%s\s+(\d+)\b' % name, src, re.M)
    assert m, name
    return int(m.group(1))


# ---- the sources --------------------------------------------------------------------------------------------------------------
def test_the_mirror_uses_the_source_constants():
    from adorym_amd.propagate import MultisliceEngine
    assert _define(_read('adm_host.h'), 'ADM_MAXCOVER') == OA.MAXCOVER == MultisliceEngine.MAX_COVER
    assert _define(_read('adm_overlap_add.hip'), 'TA_STEPS') == OA.TA_STEPS
    m = re.search(r'#define\s+ADM_FOR_EACH_SIZE\(X\)(.*)', _read('adm_multislice.hip'))
    assert m, 'ADM_FOR_EACH_SIZE'
    sizes = {int(n): (int(a), int(b)) for n, a, b in re.findall(r'X\(\s*(\d+)\s*,\s*(\d+)\s*,\s*(\d+)\s*\)', m.group(1))}
    assert sizes == OA.SIZES and len(sizes) == 10, sizes
    assert [P for P, kind in OA.PRODUCER_CASES if kind == 'tuned'] == list(sizes)
    assert {kind for _, kind in OA.PRODUCER_CASES} == {'tuned', 'generic', 'streamed'}


def test_the_mirror_follows_cover_build_kernel():
    src = _read('adm_overlap_add.hip')
    head = re.search(r'__global__\s+__launch_bounds__\((\d+)\)\s+void\s+cover_build_kernel\s*\(', src)
    assert head and int(head.group(1)) == OA.CHUNK
    body = _flat(_function_body(src, r'void\s+cover_build_kernel\s*\('))
    # the pixel block, the chunk of positions, the waves
    for line in ('__shared__ int2 sp[%d];' % OA.CHUNK, '__shared__ int sb[%d];' % OA.CHUNK, '__shared__ int wcnt[%d];' % (OA.CHUNK // OA.WAVE),
                 'const int x = blockIdx.x * %d + (threadIdx.x & %d);' % (OA.BLOCK_X, OA.BLOCK_X - 1),
                 'const int r = blockIdx.y * %d + (threadIdx.x >> 5);' % OA.BLOCK_Y,
                 'const int wave = threadIdx.x >> 6, lane = threadIdx.x & %d;' % (OA.WAVE - 1),
                 'for (int c0 = b0; c0 < B; c0 += %d) {' % OA.CHUNK,
                 'hit = ty < by_lo + %d && ty + g.Py > by_lo && tx < bx_lo + %d && tx + g.Px > bx_lo;' % (OA.BLOCK_Y, OA.BLOCK_X),
                 'for (int w = 0; w < %d; ++w) { if (w < wave) off += wcnt[w]; n += wcnt[w]; }' % (OA.CHUNK // OA.WAVE),
                 'const int k = off + __popcll(m & ((1ull << lane) - 1ull));',
                 # the element of a covering tile: elem_offset
                 'if (g.pixel_major) off_e = (unsigned)(row * g.Px + col);',
                 'const int tid = (row / g.LPW) * 64 + (row % g.LPW) * g.G + col % g.R2;',
                 'off_e = adm::ws_elem_offset(g.R1, g.NT, col / g.R2, tid);',
                 'out[(size_t)(1 + cnt) * cplane] = (unsigned)sb[j] * per_pos + off_e;',
                 'const unsigned per_pos = (unsigned)g.n_steps * g.row_elems;',
                 # the list's bound and the flag
                 'if (cnt < ADM_MAXCOVER) {', 'if (cnt > ADM_MAXCOVER) { atomicExch(overflow, 1); cnt = ADM_MAXCOVER; }'):
        assert line in body, line
    assert (1 << 5) == OA.BLOCK_X and OA.BLOCK_X * OA.BLOCK_Y == OA.CHUNK and (1 << 6) == OA.WAVE
    # ws_elem_offset and the thread geometry it is called with
    math = _read('adm_ms_math.h')
    assert ('return (R1 % 2 == 0) ? (unsigned)(((k >> 1) * NT + tid) * 2 + (k & 1)) : (unsigned)(k * NT + tid);'
            in _flat(_function_body(math, r'unsigned\s+ws_elem_offset\s*\(int R1, int NT, int k, int tid\)')))
    geo = _flat(_function_body(math, r'template\s*<int N, int R1, int R2>\s*struct\s+Geo\b'))
    for line in ('static constexpr int G = (R1 > R2) ? R1 : R2;', 'static constexpr int LPW = 64 / G;',
                 'static constexpr int NWAVES = (N + LPW - 1) / LPW;', 'static constexpr int NT = NWAVES * 64;'):
        assert line in geo, line
    tg = _flat(_function_body(src, r'static\s+int\s+tile_geom\s*\('))
    for line in ('g.pixel_major = plan->generic ? 1 : 0;', 'g.row_elems = (int)ms_row_elems(plan);',
                 'g.R1 = ms_r1_for(N); g.R2 = ms_r2_for(N); g.G = g.R1 > g.R2 ? g.R1 : g.R2; g.LPW = 64 / g.G; g.NT = ms_threads_for(N);',
                 'g.row0 = ymin + d.pad_y0;', 'g.nrows = ymax - ymin + d.probe_y;',
                 'g.n_steps = plan->n_steps; g.binning = d.binning; g.Z = d.obj_z;'):
        assert line in tg, line
    ms = _read('adm_multislice.hip')
    assert 'case N_: return Geo<N_, A_, B_>::NT;' in _function_body(ms, r'int\s+ms_threads_for\s*\(int n\)')
    assert 'case N_: return A_;' in _function_body(ms, r'int\s+ms_r1_for\s*\(int n\)')
    assert 'case N_: return B_;' in _function_body(ms, r'int\s+ms_r2_for\s*\(int n\)')
    # a streamed plan is a generic plan as far as its rows go
    create = _flat(_function_body(_read('adm_api.hip'), r'static\s+int\s+plan_create\s*\('))
    assert 'const bool tuned = !streamed && (d.probe_y == d.probe_x) && ms_threads_for(d.probe_x) != 0;' in create
    assert 'p->generic = !tuned;' in create


def test_the_mirror_follows_tile_accumulate_kernel():
    src = _read('adm_overlap_add.hip')
    head = re.search(r'__global__\s+__launch_bounds__\((\d+)\)\s+void\s+tile_accumulate_kernel\s*\(', src)
    assert head and int(head.group(1)) == OA.BLOCK_X * OA.BLOCK_Y
    body = _flat(_function_body(src, r'void\s+tile_accumulate_kernel\s*\('))
    for line in ('const int nbx = (g.Xp + %d) / %d, nby = (g.nrows + %d) / %d;' % (OA.BLOCK_X - 1, OA.BLOCK_X, OA.BLOCK_Y - 1, OA.BLOCK_Y),
                 'const int idx = blockIdx.x >> 3;', 'const int zc = (blockIdx.x & %d) + %d * (idx / (nbx * nby));' % (OA.XCDS - 1, OA.XCDS),
                 'if (zc * TA_STEPS >= g.n_steps) return;', 'ta_block(gtile, cover, grad_rot, g, zc, idx % (nbx * nby));'):
        assert line in body, line
    assert (1 << 3) == OA.XCDS
    blk = _flat(_function_body(src, r'void\s+ta_block\s*\('))
    for line in ('const int x = (rem % nbx) * 32 + (threadIdx.x & 31);', 'const int r = (rem / nbx) * 8 + (threadIdx.x >> 5);',
                 'const int st0 = zc * TA_STEPS;', 'const int nst = min(TA_STEPS, g.n_steps - st0);',
                 'if (nst == TA_STEPS) {', '} else if (nst == 1) {', 'for (; c + 4 <= cnt; c += 4) {',
                 'const int s_lo = st * g.binning, s_hi = min(s_lo + g.binning, g.Z);',
                 'const bool add = (g.row0 + r >= g.add_lo) && (g.row0 + r < g.add_hi);'):
        assert line in blk, line
    host = _flat(_function_body(src, r'static\s+int\s+tile_accumulate\s*\('))
    assert 'const unsigned nz8 = ((plan->n_steps + TA_STEPS - 1) / TA_STEPS + 7) / 8;' in host
    assert 'dim3(8u * nz8 * grid.x * grid.y), dim3(256)' in host
    build = _flat(_function_body(src, r'static\s+int\s+cover_build\s*\('))
    assert 'if (b_hi - b_lo > ADM_MAXCOVER) ADM_HIP(hipMemsetAsync(overflow, 0, sizeof(int), st));' in build
    assert 'dim3 grid((g.Xp + 31) / 32, (g.nrows + 7) / 8, 1);' in build and 'dim3 grid((g.Xp + 31) / 32, (g.nrows + 7) / 8, 1);' in host


def test_the_mirror_follows_ws_layout():
    api = _read('adm_api.hip')
    body = _flat(_function_body(api, r'WsLayout\s+ws_layout\s*\('))
    order = re.findall(r'w\.(\w+)\s*=\s*take\(', body)
    assert tuple(order[:len(OA.WS_ORDER)]) == OA.WS_ORDER, order
    for line in ('const size_t pos = (size_t)plan->n_steps * ms_row_elems(plan) * sizeof(float2);',
                 'const size_t lists = (size_t)plan->Yp * plan->Xp * (ADM_MAXCOVER + 1) * sizeof(unsigned);',
                 'w.stash = take(B * M * pos);', 'w.gtile = take(B * pos);', 'w.cover = take(lists);', 'w.overflow = take(64);'):
        assert line in body, line
    rows = _flat(_function_body(api, r'size_t\s+ms_row_elems\s*\('))
    assert 'if (plan->generic) return (size_t)plan->d.probe_y * plan->d.probe_x;' in rows
    assert 'return (size_t)ms_r1_for(plan->d.probe_x) * ms_threads_for(plan->d.probe_x);' in rows
    assert OA.gtile_byte_offset(11, 3, 5, 128) == 11 * 3 * 5 * 128 * 8
    assert OA.overflow_byte_offset(11, 1, 5, 128, 25, 27) == 2 * 11 * 5 * 128 * 8 + 25 * 27 * 65 * 4


# ---- the mirror ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('N', list(OA.SIZES))
def test_elem_offset_is_injective_into_the_row(N):
    R1, R2, G, LPW, NT = OA.thread_geometry(N)
    assert R1 * R2 == N and OA.row_elems(N) == R1 * NT
    rr, cc = np.meshgrid(np.arange(N), np.arange(N), indexing='ij')
    off = np.asarray(OA.elem_offset(N, rr, cc)).reshape(-1)
    assert off.min() >= 0 and off.max() < R1 * NT and len(np.unique(off)) == N * N
    assert all(OA.elem_offset(N, r, c) == off[r * N + c] for r, c in ((0, 0), (N - 1, N - 1), (1, R2), (min(LPW, N - 1), 1)))
    # every thread id stays inside the NT threads of the kernel and the lines of a wave do not share lanes
    tid = (rr // LPW) * 64 + (rr % LPW) * G + cc % R2
    assert tid.max() < NT and (rr % LPW).max() * G + R2 - 1 < 64
    g = OA.make_geom((N + 3, N + 4, 2), N, ((1, 1), (1, 1)))
    t = OA.tile_values(1, 2, g)
    raw = OA.pack_gtile(g, t)
    assert np.array_equal(OA.unpack_gtile(g, raw, 2), t) and int((raw == OA.FILLER).sum()) == 2 * 2 * 2 * (R1 * NT - N * N)


def test_elem_offset_is_pixel_major_off_the_tuned_sizes():
    assert OA.elem_offset((40, 24), 3, 5) == 3 * 24 + 5 and OA.row_elems((40, 24)) == 960
    assert OA.elem_offset(8, 3, 5, pixel_major=True) == 29 and OA.row_elems(8, True) == 64
    assert OA.elem_offset(8, 3, 5) != 29


# ---- the reference ------------------------------------------------------------------------------------------------------------
def _all_cases():
    return list(OA.ALL_SYNTHETIC.items()) + [('ahead%d' % i, c) for i, c in enumerate(OA.AHEAD_CASES)] + [('ahead_larger', OA.AHEAD_LARGER)]


@pytest.mark.parametrize('name', [n for n, _ in _all_cases()])
def test_reference_vs_fp64_oracle_and_brute_force_cover(name):
    """overlap_add_ref (sequential float32) against the oracle's fp64 overlap-add within (n - 1) * 2^-24 * sum|v| per pixel -- the
    bound of recursive summation of n terms with unit roundoff 2^-24 (Higham, Accuracy and Stability, eq. 4.4, first order; the
    n = 1 case is exact) -- and its cover-count map against a brute-force count."""
    c = dict(_all_cases())[name]
    g, pos = c['geom'], c['pos']
    t = OA.case_values(c)
    before = OA.sentinel(g)
    out, cover = OA.overlap_add_ref(t, pos, g, before)
    assert np.array_equal(cover, OA.brute_cover(pos, g))
    r0, r1 = OA.rows_of(pos, g)
    # outside the batch's rows nothing changed
    keep = np.ones(g.Yp, bool)
    keep[r0:r1] = False
    assert np.array_equal(OA.bits(out[:, keep]), OA.bits(before[:, keep]))
    # the oracle on the padded frame (object = padded frame, no pads of its own): [Yp, Xp, n_steps, 2]
    t64 = np.moveaxis(t.astype(np.float64), 1, 3)                       # [B, Py, Px, n_steps, 2]
    ppos = pos + np.array([g.pad_y0, g.pad_x0])
    ref = O.scatter_tiles_adj(t64, ppos, (g.Yp, g.Xp, g.n_steps))
    mag = O.scatter_tiles_adj(np.abs(t64), ppos, (g.Yp, g.Xp, g.n_steps))
    bound = np.maximum(cover - 1, 0)[:, :, None, None] * 2.0 ** -24 * mag
    for st in range(g.n_steps):
        for sl in range(st * g.binning, min((st + 1) * g.binning, g.Z)):
            err = np.abs(out[sl, r0:r1].astype(np.float64) - ref[r0:r1, :, st])
            assert (err <= bound[r0:r1, :, st]).all(), (name, st, sl, float((err - bound[r0:r1, :, st]).max()))
    assert (out[:, r0:r1][:, cover[r0:r1] == 0] == 0).all()
    assert g.n_steps * g.binning >= g.Z > (g.n_steps - 1) * g.binning


@pytest.mark.parametrize('name', ['steps3', 'Z7_bin3', 'p18_Xp45_rows29', 'p27_Xp64_rows40', 'generic40x24_Xp37_rows53'])
def test_reference_equals_a_walk_through_the_packed_section(name):
    """The two kernels restated pixel by pixel on the PACKED section -- the list of (position * per_pos + elem_offset) sources in
    position order, then the gather from the flat array -- give the reference's bits: the packing, the mirror and the reference
    agree with one another before any of them meets the GPU."""
    c = OA.ALL_SYNTHETIC[name]
    g, pos = c['geom'], c['pos']
    t = OA.case_values(c)
    flat = OA.pack_gtile(g, t).reshape(-1, 2)
    per_pos = g.n_steps * g.row_elems
    ref, cover = OA.overlap_add_ref(t, pos, g, OA.sentinel(g))
    r0, r1 = OA.rows_of(pos, g)
    for y in range(r0, r1):
        for x in range(g.Xp):
            src = [int(b) * per_pos + int(OA.elem_offset(g.P, y - (pos[b][0] + g.pad_y0), x - (pos[b][1] + g.pad_x0), g.pixel_major))
                   for b in OA.covering(pos, g, y, x)]
            assert len(src) == cover[y, x]
            for st in range(g.n_steps):
                acc = np.zeros(2, np.float32)
                for e in src:
                    acc = acc + flat[e + st * g.row_elems]
                for sl in range(st * g.binning, min((st + 1) * g.binning, g.Z)):
                    assert np.array_equal(OA.bits(acc), OA.bits(ref[sl, y, x])), (name, y, x, st, sl)


def test_reference_modes_are_consistent():
    """Parts and range passes are re-associations of the same sum: within the same bound of the fp64 sum; where a pixel is
    reached by one part only they are the whole-batch bits."""
    c = OA.PART_CASE
    g, pos, t = c['geom'], c['pos'], OA.case_values(c)
    whole, cover = OA.overlap_add_ref(t, pos, g, OA.sentinel(g))
    win = OA.part_window(c)
    w0, w1 = win[0] + g.pad_y0, win[1] + g.pad_y0
    for parts in OA.PART_SPLITS.values():
        assert sum(n for _, n in parts) == len(pos) and [o for o, _ in parts] == list(np.cumsum([0] + [n for _, n in parts[:-1]]))
        out, cov = OA.parts_ref(t, pos, g, OA.sentinel(g), parts, win)
        assert np.array_equal(cov, cover)
        r0, r1 = OA.rows_of(pos, g)
        assert (w0, w1) == (r0 - 2, r1 + 2) and w0 >= 0 and w1 <= g.Yp
        assert (out[:, w0:r0] == 0).all() and (out[:, r1:w1] == 0).all()          # window rows no part reaches
        assert np.array_equal(OA.bits(out[:, :w0]), OA.bits(OA.sentinel(g)[:, :w0]))
        single = np.zeros((g.Yp, g.Xp), bool)
        for o, n in parts:
            single |= OA.brute_cover(pos[o:o + n], g) == cover
        single[:r0] = single[r1:] = False
        assert single.any() and not single[r0:r1].all()
        # (+0 from the other parts: x + 0 = x bit for bit, except -0 + 0 = +0, which compares equal as a number)
        assert np.array_equal(out[:, single], whole[:, single])
        assert (OA.bits(out[:, r0:r1]) != OA.bits(whole[:, r0:r1])).any()          # ... and the part order shows elsewhere
    # every part of 'three' reaches rows that another does not: the add rows differ from part to part
    rows = [OA.rows_of(pos[o:o + n], g) for o, n in OA.PART_SPLITS['three']]
    assert len(set(rows)) == 3, rows


# ---- the tables reach what their names say --------------------------------------------------------------------------------------
def _counts(c):
    return OA.brute_cover(c['pos'], c['geom'])


def test_cover_cases_reach_the_named_counts():
    reached = set()
    for name, c in OA.COVER_CASES.items():
        cover = _counts(c)
        for n in c['named']:
            assert (cover == n).any(), (name, n)
            reached.add(n)
        assert (cover.max() > OA.MAXCOVER) == bool(c['overflow']), name
        assert c['geom'].n_steps == 3                       # a full step chunk and the one-step branch
    assert reached >= {1, 3, 4, 5, 63, 64, 65}
    B = {n: len(c['pos']) for n, c in OA.COVER_CASES.items()}
    assert B['upto64'] > OA.MAXCOVER and _counts(OA.COVER_CASES['upto64']).max() == OA.MAXCOVER       # the flag is maintained and stays 0
    assert B['over65'] == 65 and _counts(OA.COVER_CASES['over65']).max() == 65
    assert (_counts(OA.COVER_CASES['over65']) <= OA.MAXCOVER).sum() > (_counts(OA.COVER_CASES['over65']) > OA.MAXCOVER).sum() > 0
    assert B['after65'] == B['over65'] and OA.COVER_CASES['after65']['geom'] == OA.COVER_CASES['over65']['geom']     # the same flag word
    assert B['exactly64'] == OA.MAXCOVER and _counts(OA.COVER_CASES['exactly64']).max() == OA.MAXCOVER
    # the covering positions of the 63 / 64 pixels are not a contiguous run of the batch
    c = OA.COVER_CASES['upto64']
    y, x = np.argwhere(_counts(c) == 64)[0]
    b = OA.covering(c['pos'], c['geom'], y, x)
    assert len(b) == 64 and b[-1] - b[0] > 63


def test_step_cases_reach_both_branches_and_three_xcd_rounds():
    chunks = lambda c: -(-c['geom'].n_steps // OA.TA_STEPS)
    last = lambda c: c['geom'].n_steps - (chunks(c) - 1) * OA.TA_STEPS
    S = OA.STEP_CASES
    assert [c['geom'].n_steps for c in S.values()] == [1, 2, 3, 16, 17, 33, 3, 18]
    assert any(last(c) == OA.TA_STEPS for c in S.values()) and any(last(c) == 1 for c in S.values())
    assert chunks(S['steps16']) == OA.XCDS                                   # exactly one round
    assert chunks(S['steps17']) == OA.XCDS + 1 and last(S['steps17']) == 1   # the second round, one step
    assert chunks(S['Z35_bin2']) == OA.XCDS + 1 and last(S['Z35_bin2']) == OA.TA_STEPS
    assert chunks(S['steps33']) == 2 * OA.XCDS + 1                           # the third round
    assert max(chunks(c) for c in S.values()) - 1 >= 16 and sum(chunks(c) - 1 >= 8 for c in S.values()) >= 3
    for name in ('Z7_bin3', 'Z35_bin2'):                                     # the last bin is cut by Z
        g = S[name]['geom']
        assert g.n_steps * g.binning > g.Z
    # the one-step branch walks the lists four entries at a time: full groups, a remainder, fewer than four
    for name, c in S.items():
        if last(c) == 1:
            cover = _counts(c)
            assert (cover >= 8).any() and ((cover > 4) & (cover % 4 != 0)).any() and ((cover > 0) & (cover < 4)).any(), name
        assert len(c['pos']) == 16 and c['geom'].pad_y0 > 0 and c['geom'].pad_x0 > 0


def test_large_cases_stay_within_the_lists_and_mix_chunks_and_waves():
    for name, c in OA.LARGE_CASES.items():
        g, pos = c['geom'], c['pos']
        assert _counts(c).max() <= OA.MAXCOVER, name
        px = OA.order_pixels(c)
        assert len(px) == 4
        n_chunks = -(-len(pos) // OA.CHUNK)
        for y, x in px:
            b = OA.covering(pos, g, y, x)
            assert len(set(b // OA.CHUNK)) == n_chunks, (name, y, x)
            assert max(len(set(b[b // OA.CHUNK == k] // OA.WAVE)) for k in range(n_chunks)) >= 2, (name, y, x)
    assert [len(c['pos']) for c in OA.LARGE_CASES.values()] == [256, 257, 513]
    c = OA.LARGE_CASES['B513']
    assert all(len(set(OA.covering(c['pos'], c['geom'], y, x) // OA.CHUNK)) >= 3 for y, x in OA.order_pixels(c))


def test_frame_cases_reach_the_block_edges():
    xp = [c['geom'].Xp for c in OA.FRAME_CASES.values()]
    assert {31, 32, 33, 65} <= set(xp)
    nrows = [np.subtract(*OA.rows_of(c['pos'], c['geom'])[::-1]) for c in OA.FRAME_CASES.values()]
    assert any(v % OA.BLOCK_X == 0 for v in xp) and any(v % OA.BLOCK_X for v in xp)
    assert any(v % OA.BLOCK_Y == 0 for v in nrows) and any(v % OA.BLOCK_Y for v in nrows)
    assert any(v > OA.BLOCK_X for v in xp) and all(v > OA.BLOCK_Y for v in nrows)                 # more than one block either way
    for name, c in OA.FRAME_CASES.items():
        g, pos = c['geom'], c['pos']
        Y, X = c['obj'][:2]
        assert g.pad_y0 > 0 and g.pad_x0 > 0, name
        assert pos[:, 0].min() < 0 and pos[:, 1].min() < 0 and (pos[:, 0] + g.Py).max() > Y and (pos[:, 1] + g.Px).max() > X, name
        r0, r1 = OA.rows_of(pos, g)
        assert r0 > 0 and r1 < g.Yp, name                                                          # rows outside the window exist
    g = OA.FRAME_CASES['generic40x24_Xp37_rows53']['geom']
    assert g.pixel_major and (g.Py, g.Px) == (40, 24) and g.Yp != g.Xp
    assert not OA.FRAME_CASES['p18_Xp45_rows29']['geom'].pixel_major and OA.SIZES[27][0] % 2 == 1


def test_range_case_needs_its_passes():
    c = OA.RANGE_CASE
    cover = _counts(c)
    assert len(c['pos']) == 150 and cover.max() == 70 and (cover == 70).any()
    assert OA.RANGE_PASSES == [(lo, min(lo + OA.MAXCOVER, 150)) for lo in range(0, 150, OA.MAXCOVER)] == [(0, 64), (64, 128), (128, 150)]
    g = c['geom']
    r0, r1 = OA.rows_of(c['pos'], g)
    rows = [OA.rows_of(c['pos'][lo:hi], g) for lo, hi in OA.RANGE_PASSES]
    assert any(r != (r0, r1) for r in rows)                   # a pass whose own rows are fewer than the batch's
    y, x = np.argwhere(cover == 70)[0]
    b = OA.covering(c['pos'], g, y, x)
    assert all(((b >= lo) & (b < hi)).any() for lo, hi in OA.RANGE_PASSES)


def test_ahead_cases_differ():
    keys = {c['pos'].tobytes() for c in OA.AHEAD_CASES}
    assert len(keys) == 5 and len({c['geom'] for c in OA.AHEAD_CASES + [OA.AHEAD_LARGER]}) == 1
    assert len(OA.AHEAD_LARGER['pos']) != len(OA.AHEAD_CASES[0]['pos'])
    a, b = OA.AHEAD_CASES[0], OA.AHEAD_CASES[1]
    ra, _ = OA.overlap_add_ref(OA.case_values(a), a['pos'], a['geom'], OA.sentinel(a['geom']))
    rb, _ = OA.overlap_add_ref(OA.case_values(a), b['pos'], b['geom'], OA.sentinel(a['geom']))
    assert (OA.bits(ra) != OA.bits(rb)).any()                 # stale lists would show


# ---- discrimination -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('name', list(OA.LARGE_CASES))
def test_order_pixels_tell_a_wrong_order(name):
    """At every order pixel the sum in reversed position order differs in bits from the forward sum, and so do the sums with the
    256-chunks or the waves inside a chunk taken backwards, where the batch has more than one of them (the kernel applies one order
    to every step and both components of a pixel: one differing word per pixel tells).  The seeds of the table were chosen so."""
    c = OA.LARGE_CASES[name]
    g, pos, t = c['geom'], c['pos'], OA.case_values(c)
    B = len(pos)
    fwd, _ = OA.partial_sums(t, pos, g)
    others = {'reversed': np.arange(B)[::-1], 'waves backwards': OA.wave_swapped_order(B)}
    if B > OA.CHUNK:
        others['chunks backwards'] = OA.chunk_swapped_order(B)
    for what, order in others.items():
        assert sorted(order) == list(range(B))
        alt, _ = OA.partial_sums(t, pos, g, order=order)
        for y, x in OA.order_pixels(c):
            assert (OA.bits(alt[:, y, x]) != OA.bits(fwd[:, y, x])).any(), (name, what, y, x)


@pytest.mark.parametrize('name', ['upto64', 'after65', 'exactly64'])
def test_most_covered_pixels_tell_a_wrong_order(name):
    c = OA.COVER_CASES[name]
    g, pos, t = c['geom'], c['pos'], OA.case_values(c)
    fwd, cover = OA.partial_sums(t, pos, g)
    rev, _ = OA.partial_sums(t, pos, g, order=range(len(pos) - 1, -1, -1))
    y, x = np.argwhere(cover == cover.max())[0]
    assert (OA.bits(rev[:, y, x]) != OA.bits(fwd[:, y, x])).any(), name


def test_values_spread_and_sentinel_is_finite():
    g = OA.STEP_CASES['steps3']['geom']
    t = OA.tile_values(3, 11, g)
    e = np.log2(np.abs(t))
    assert t.dtype == np.float32 and e.min() < -11 and e.max() > 11 and 0.4 < (t > 0).mean() < 0.6
    s = OA.sentinel(g)
    assert np.isfinite(s).all() and s.shape == (g.Z, g.Yp, g.Xp, 2) and len(np.unique(OA.bits(s))) == s.size
    assert np.array_equal(OA.tile_values(3, 11, g), t)
