"""The overlap-add of the per-position tile gradients (adm_overlap_add.hip: cover_build_kernel, tile_accumulate_kernel and the host
code around them) against a host reference that reproduces it BIT FOR BIT (test infrastructure only).

The operation is fp32 addition in a fixed order: per padded pixel and modulation step the elements of the covering positions are
added one by one in ascending position index, starting from +0; an ``add`` part then adds that partial sum to what the rows
hold.  ``overlap_add_ref`` does exactly that in numpy float32, so the GPU tests compare ``uint32`` views and allow no tolerance.

This module holds
  * the mirror of the workspace layout the kernels read: ``elem_offset`` (where element (row, col) of one step of one position
    sits in a workspace row), ``gtile_byte_offset`` / ``overflow_byte_offset`` (sections of ws_layout, adm_api.hip),
  * the reference and its pieces (``partial_sums``, ``overlap_add_ref``, ``parts_ref``),
  * the seeded value generator and the sentinel pattern,
  * the case tables of tests/test_gpu_overlap_add.py.
tests/test_overlap_add_coverage.py parses the sources and fails when a constant, the layout or the index arithmetic mirrored
here changes there, and computes from the tables that every case reaches what its name says.
"""
import collections

import numpy as np

# ---- constants of the sources (checked by tests/test_overlap_add_coverage.py) ---------------------------------------------------
MAXCOVER = 64            # ADM_MAXCOVER (adm_host.h) = MultisliceEngine.MAX_COVER: cover-list entries per pixel
TA_STEPS = 2             # modulation steps per block of tile_accumulate_kernel
CHUNK = 256              # positions cover_build_kernel reads at a time (= its block size)
WAVE = 64                # ... whose hits are ordered by a ballot per 64-lane wave and the waves' counts
BLOCK_X, BLOCK_Y = 32, 8  # pixels of one block of both kernels
XCDS = 8                 # tile_accumulate_kernel deals its step chunks over 8 XCDs: zc = (blockIdx & 7) + 8 * round
# ADM_FOR_EACH_SIZE of adm_multislice.hip: N -> (R1, R2)
SIZES = {8: (2, 4), 12: (3, 4), 16: (4, 4), 18: (2, 9), 24: (3, 8), 27: (3, 9), 32: (4, 8), 36: (4, 9), 64: (8, 8), 72: (8, 9)}
WS_ORDER = ('stash', 'gtile', 'cover', 'overflow')       # the first sections of ws_layout, in its order

ENERGY_EV, PSIZE_CM = 5000., 1e-7


# ---- the layout mirror --------------------------------------------------------------------------------------------------------
def is_pixel_major(P, pixel_major=None):
    """Rows of generic and streamed plans are pixel-major; the tuned sizes (a square probe of SIZES, not forced generic) use the
    multislice kernel's thread-native order."""
    if pixel_major is not None:
        return bool(pixel_major)
    return not (np.isscalar(P) and int(P) in SIZES)


def probe_shape(P):
    return (int(P), int(P)) if np.isscalar(P) else (int(P[0]), int(P[1]))


def thread_geometry(N):
    """(R1, R2, G, LPW, NT) of a tuned size: Geo<N, R1, R2> of adm_ms_math.h as tile_geom (adm_overlap_add.hip) fills it in."""
    R1, R2 = SIZES[N]
    G = max(R1, R2)
    LPW = 64 // G
    NT = -(-N // LPW) * 64
    return R1, R2, G, LPW, NT


def ws_elem_offset(R1, NT, k, tid):
    """ws_elem_offset of adm_ms_math.h: R1 even -- pairs [k / 2][tid][2]; R1 odd -- [k][tid]."""
    if R1 % 2 == 0:
        return ((k >> 1) * NT + tid) * 2 + (k & 1)
    return k * NT + tid


def row_elems(P, pixel_major=None):
    """float2 elements of one workspace row (one modulation step of one position): ms_row_elems of adm_api.hip."""
    Py, Px = probe_shape(P)
    if is_pixel_major(P, pixel_major):
        return Py * Px
    R1, _, _, _, NT = thread_geometry(Py)
    return R1 * NT


def elem_offset(P, row, col, pixel_major=None):
    """Where element (row, col) of one step of one position sits in its workspace row (ints or integer arrays)."""
    Py, Px = probe_shape(P)
    if is_pixel_major(P, pixel_major):
        return row * Px + col
    R1, R2, G, LPW, NT = thread_geometry(Py)
    tid = (row // LPW) * 64 + (row % LPW) * G + col % R2
    k = col // R2
    return ws_elem_offset(R1, NT, k, tid)


def gtile_byte_offset(B, M, n_steps, row_elems_):
    """Byte offset of the tile-gradient section: ws_layout puts the stash [B][M][n_steps][row] first and gtile second."""
    return B * M * n_steps * row_elems_ * 8


def overflow_byte_offset(B, M, n_steps, row_elems_, Yp, Xp):
    """Byte offset of the overflow flag: behind gtile [B][n_steps][row] and the cover lists [Yp * Xp][1 + MAXCOVER] u32."""
    return gtile_byte_offset(B, M, n_steps, row_elems_) + B * n_steps * row_elems_ * 8 + Yp * Xp * (1 + MAXCOVER) * 4


Geom = collections.namedtuple('Geom', 'Yp Xp pad_y0 pad_x0 Py Px Z binning n_steps P pixel_major row_elems')


def make_geom(obj_size, P, pads, binning=1, pixel_major=None):
    """The geometry of a plan: obj_size (Y, X, Z), probe P (a tuned size N, or (Py, Px)), pads ((y0, y1), (x0, x1))."""
    Y, X, Z = [int(v) for v in obj_size]
    Py, Px = probe_shape(P)
    pm = is_pixel_major(P, pixel_major)
    return Geom(Y + pads[0][0] + pads[0][1], X + pads[1][0] + pads[1][1], int(pads[0][0]), int(pads[1][0]), Py, Px, Z, int(binning),
                -(-Z // int(binning)), P, pm, row_elems(P, pm))


def _offsets(g):
    rr, cc = np.meshgrid(np.arange(g.Py), np.arange(g.Px), indexing='ij')
    return np.asarray(elem_offset(g.P, rr, cc, g.pixel_major)).reshape(-1)


FILLER = np.float32(1e30)      # what the row elements no pixel maps to hold in a packed section (a kernel reading one shows at once)


def pack_gtile(g, tiles):
    """tiles float32 [B, n_steps, Py, Px, 2] -> the gtile section [B, n_steps, row_elems, 2] in the mirrored element order."""
    B = tiles.shape[0]
    raw = np.full((B, g.n_steps, g.row_elems, 2), FILLER, np.float32)
    raw[:, :, _offsets(g)] = tiles.reshape(B, g.n_steps, g.Py * g.Px, 2)
    return raw


def unpack_gtile(g, raw, B):
    """The gtile section read back (any dtype / shape of B * n_steps * row_elems * 8 bytes) -> float32 [B, n_steps, Py, Px, 2]."""
    raw = np.ascontiguousarray(raw).view(np.float32).reshape(B, g.n_steps, g.row_elems, 2)
    return np.ascontiguousarray(raw[:, :, _offsets(g)].reshape(B, g.n_steps, g.Py, g.Px, 2))


# ---- the reference ------------------------------------------------------------------------------------------------------------
def partial_sums(gtile, pos, g, order=None):
    """(acc float32 [n_steps, Yp, Xp, 2], cover int [Yp, Xp]): per padded pixel and step the covering positions' elements added
    one by one in the order ``order`` (default: ascending position index) starting from +0, in float32; and how many cover it."""
    acc = np.zeros((g.n_steps, g.Yp, g.Xp, 2), np.float32)
    cover = np.zeros((g.Yp, g.Xp), np.int64)
    gtile = np.asarray(gtile)
    assert gtile.dtype == np.float32 and gtile.shape[1:] == (g.n_steps, g.Py, g.Px, 2), gtile.shape
    for b in (range(len(pos)) if order is None else order):
        y0, x0 = int(pos[b][0]) + g.pad_y0, int(pos[b][1]) + g.pad_x0
        assert 0 <= y0 and y0 + g.Py <= g.Yp and 0 <= x0 and x0 + g.Px <= g.Xp, (b, y0, x0)
        acc[:, y0:y0 + g.Py, x0:x0 + g.Px] += gtile[b]
        cover[y0:y0 + g.Py, x0:x0 + g.Px] += 1
    return acc, cover


def rows_of(pos, g):
    """The padded rows [r0, r1) the tiles of ``pos`` reach (tile_geom: row0, row0 + nrows)."""
    y = np.asarray(pos)[:, 0]
    return int(y.min()) + g.pad_y0, int(y.max()) + g.pad_y0 + g.Py


def _write(out, acc, g, r0, r1, add):
    for st in range(g.n_steps):
        for sl in range(st * g.binning, min(st * g.binning + g.binning, g.Z)):
            out[sl, r0:r1] = out[sl, r0:r1] + acc[st, r0:r1] if add else acc[st, r0:r1]


def overlap_add_ref(gtile, pos, g, grad_rot_before, mode='whole', window=None, passes=None):
    """What the overlap-add leaves in grad_rot [Z, Yp, Xp, 2] (float32; ``grad_rot_before`` is not changed), and the cover-count map.

    mode 'whole': adm_tile_grad_accumulate -- the batch's rows, all Xp columns, zeros where nothing covers;
         'first': adm_tile_grad_accumulate_part(add = 0) with ``window`` = (y_lo, y_hi) in object rows -- the whole window is written;
         'add':   adm_tile_grad_accumulate_part(add = 1) -- old + partial sum on the part's own rows;
         'range': adm_tile_grad_accumulate_range as MultisliceEngine._overlap_add calls it -- the batch's rows are zeroed, then every
                  pass ``(lo, hi)`` of ``passes`` (default: MAXCOVER positions each) adds its own partial sum on its own rows.
    Every slice of a step's bin receives the step's sum.  A pixel covered more than MAXCOVER times is summed over ALL its tiles
    here (the kernel keeps the first MAXCOVER and raises the overflow flag): the tests compare the other pixels only."""
    out = np.array(grad_rot_before, dtype=np.float32, copy=True)
    assert out.shape == (g.Z, g.Yp, g.Xp, 2), out.shape
    pos = np.asarray(pos).reshape(-1, 2)
    if mode == 'range':
        cover = np.zeros((g.Yp, g.Xp), np.int64)
        r0, r1 = rows_of(pos, g)
        out[:, r0:r1] = 0
        if passes is None:
            passes = [(lo, min(lo + MAXCOVER, len(pos))) for lo in range(0, len(pos), MAXCOVER)]
        for lo, hi in passes:
            acc, c = partial_sums(gtile[lo:hi], pos[lo:hi], g)
            cover += c
            _write(out, acc, g, *rows_of(pos[lo:hi], g), add=True)
        return out, cover
    acc, cover = partial_sums(gtile, pos, g)
    if mode == 'whole':
        _write(out, acc, g, *rows_of(pos, g), add=False)
    elif mode == 'first':
        r0, r1 = rows_of(pos, g)
        w0, w1 = window[0] + g.pad_y0, window[1] + g.pad_y0
        assert w0 <= r0 and r1 <= w1 and 0 <= w0 and w1 <= g.Yp, (window, r0, r1)
        _write(out, acc, g, w0, w1, add=False)
    elif mode == 'add':
        _write(out, acc, g, *rows_of(pos, g), add=True)
    else:
        raise ValueError(mode)
    return out, cover


def parts_ref(gtile, pos, g, grad_rot_before, parts, window):
    """A batch launched in ``parts`` [(offset, count), ...]: the first writes the whole ``window``, the others add on their rows
    (MultisliceEngine.multislice_overlapped).  Returns grad_rot and the whole batch's cover-count map."""
    out = grad_rot_before
    cover = 0
    for i, (o, n) in enumerate(parts):
        out, c = overlap_add_ref(gtile[o:o + n], pos[o:o + n], g, out, 'add' if i else 'first', window=window)
        cover = cover + c
    return out, cover


def brute_cover(pos, g):
    """Cover counts by asking every pixel about every position (the reference's map must equal it)."""
    pos = np.asarray(pos).reshape(-1, 2)
    yy, xx = np.meshgrid(np.arange(g.Yp), np.arange(g.Xp), indexing='ij')
    ty, tx = pos[:, 0] + g.pad_y0, pos[:, 1] + g.pad_x0
    inside = ((yy[None] >= ty[:, None, None]) & (yy[None] < ty[:, None, None] + g.Py) &
              (xx[None] >= tx[:, None, None]) & (xx[None] < tx[:, None, None] + g.Px))
    return inside.sum(0)


def covering(pos, g, y, x):
    """Indices of the positions whose tile covers padded pixel (y, x), ascending."""
    pos = np.asarray(pos).reshape(-1, 2)
    ty, tx = pos[:, 0] + g.pad_y0, pos[:, 1] + g.pad_x0
    return np.flatnonzero((y >= ty) & (y < ty + g.Py) & (x >= tx) & (x < tx + g.Px))


# ---- values -------------------------------------------------------------------------------------------------------------------
def tile_values(seed, B, g):
    """Seeded tile gradients float32 [B, n_steps, Py, Px, 2]: magnitudes spread over 2^-12 .. 2^12, mixed signs, so that fp32
    addition is visibly non-associative (a sum in another order differs in its last bits)."""
    r = np.random.default_rng([int(seed), B, g.n_steps, g.Py, g.Px])
    shape = (B, g.n_steps, g.Py, g.Px, 2)
    return (np.exp2(r.uniform(-12., 12., shape)) * r.choice([-1., 1.], shape)).astype(np.float32)


def sentinel(g):
    """A finite pattern for grad_rot [Z, Yp, Xp, 2], every word different from its neighbours: 2^23 + index (mod 2^22)."""
    n = g.Z * g.Yp * g.Xp * 2
    return (np.uint32(0x4B000000) + (np.arange(n, dtype=np.uint32) & np.uint32(0x3FFFFF))).view(np.float32).reshape(g.Z, g.Yp, g.Xp, 2)


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


# ---- positions ----------------------------------------------------------------------------------------------------------------
def y_range(g):
    """Object rows a tile may start at inside the padded frame: [lo, hi]."""
    return -g.pad_y0, g.Yp - g.pad_y0 - g.Py


def x_range(g):
    return -g.pad_x0, g.Xp - g.pad_x0 - g.Px


def spread_positions(seed, B, g, ylim=None, xlim=None):
    """B positions: the four corners of the allowed range first (they hang over all four edges of the object when the pads are
    positive), the rest anywhere inside it."""
    r = np.random.default_rng([int(seed), B, g.Yp, g.Xp])
    ylo, yhi = ylim if ylim is not None else y_range(g)
    xlo, xhi = xlim if xlim is not None else x_range(g)
    pos = [(ylo, xlo), (ylo, xhi), (yhi, xlo), (yhi, xhi)][:B]
    pos += [(int(r.integers(ylo, yhi + 1)), int(r.integers(xlo, xhi + 1))) for _ in range(B - len(pos))]
    return np.array(pos, np.int32)


def shuffled(seed, pos):
    pos = np.asarray(pos, np.int32).reshape(-1, 2)
    return np.ascontiguousarray(pos[np.random.default_rng(int(seed)).permutation(len(pos))])


# ---- case tables --------------------------------------------------------------------------------------------------------------
# A case: P (tuned size or (Py, Px)), obj (Y, X, Z), pads, binning, pos int32 [B, 2] (object coordinates), seed of the values.
def case(P, obj, pads, pos=None, B=11, binning=1, seed=0, ylim=None, **extra):
    g = make_geom(obj, P, pads, binning)
    if pos is None:
        pos = spread_positions(seed, B, g, ylim=ylim)
    pos = np.ascontiguousarray(np.asarray(pos, np.int32).reshape(-1, 2))
    return dict(P=P, obj=tuple(obj), pads=pads, binning=binning, pos=pos, seed=seed, geom=g, **extra)


def case_values(c):
    return tile_values(c['seed'], len(c['pos']), c['geom'])


_PADS = ((3, 2), (2, 3))

# (b) steps and binning at P = 8: both nst branches, the second and third round of step chunks over the XCDs, bins cut by Z
STEP_CASES = collections.OrderedDict()
def _step_case(Z, binning, seed):
    # four corners (a padded row above and below them stays untouched) and twelve tiles within a few pixels of one another:
    # covers from 1 to 12
    g = make_geom((20, 22, Z), 8, _PADS, binning)
    pos = np.concatenate([spread_positions(seed, 4, g, ylim=(-2, 13)), spread_positions(seed, 16, g, ylim=(4, 8), xlim=(5, 9))[4:]])
    return case(8, (20, 22, Z), _PADS, pos=pos, binning=binning, seed=seed)


for _n in (1, 2, 3, 16, 17, 33):
    STEP_CASES['steps%d' % _n] = _step_case(_n, 1, 10 + _n)
STEP_CASES['Z7_bin3'] = _step_case(7, 3, 51)          # 3 steps, the last bins one slice
STEP_CASES['Z35_bin2'] = _step_case(35, 2, 52)        # 18 steps, the last bins one slice


# (c) cover counts.  All at P = 8 and Z = 3 (a full step chunk and the one-step branch).
def _stack(y, x, n):
    return [(y, x)] * n


_COVER_OBJ, _COVER_PADS = (44, 41, 3), ((2, 3), (3, 2))
_CLUSTER = [(30, 0), (30, 1), (30, 2), (30, 3), (30, 4)]                          # covers 1, 2, 3, 4, 5 along a row
COVER_CASES = collections.OrderedDict()
# 63 tiles on one spot and one 7 columns beside them: 63 / 64 / 1; the cluster: 1, 3, 4, 5.  69 positions: the flag is maintained.
COVER_CASES['upto64'] = case(8, _COVER_OBJ, _COVER_PADS, pos=shuffled(1, _stack(10, 10, 63) + [(10, 17)] + _CLUSTER), seed=61,
                             named=(1, 3, 4, 5, 63, 64), overflow=0)
# 65 tiles on one pixel (three x two different corners, so that other pixels hold fewer): the flag is raised
COVER_CASES['over65'] = case(8, _COVER_OBJ, _COVER_PADS, pos=shuffled(2, [(10 + i % 2, 10 + i % 3) for i in range(65)]), seed=62,
                             named=(65,), overflow=1)
# the same workspace and batch size afterwards, nothing above 60: the flag is back to 0
COVER_CASES['after65'] = case(8, _COVER_OBJ, _COVER_PADS, pos=shuffled(3, _stack(10, 10, 60) + _CLUSTER), seed=63, named=(60,), overflow=0)
# 64 tiles on one spot: a batch that cannot overflow, the flag is not maintained
COVER_CASES['exactly64'] = case(8, _COVER_OBJ, _COVER_PADS, pos=_stack(12, 9, 64), seed=64, named=(64,), overflow=0)

# (d) large batches on a frame on which no pixel is covered more than MAXCOVER times: 1, 2 and 3 chunks of 256 positions
LARGE_CASES = collections.OrderedDict()
# (seeds for which the discrimination condition of tests/test_overlap_add_coverage.py holds at every order pixel)
for _B, _seed in ((256, 326), (257, 327), (513, 584)):
    LARGE_CASES['B%d' % _B] = case(8, (60, 59, 3), ((2, 2), (3, 2)), B=_B, seed=_seed, ylim=(-1, 53))


def order_pixels(c, n=4):
    """The "order" pixels of a case: the ``n`` pixels covered from the most (256-chunk, wave) groups -- first by the number of
    chunks, then of groups, then by cover count (ties: the first in row-major order)."""
    g, pos = c['geom'], c['pos']
    keys = []
    for y in range(g.Yp):
        for x in range(g.Xp):
            b = covering(pos, g, y, x)
            keys.append((len(set(b // CHUNK)), len(set(b // WAVE)), len(b), -(y * g.Xp + x)))
    best = sorted(range(len(keys)), key=lambda i: keys[i], reverse=True)[:n]
    return [(i // g.Xp, i % g.Xp) for i in best]


def wave_swapped_order(B):
    """Position order with the four waves of every 256-chunk taken backwards (what a wrong prefix over the waves' counts gives)."""
    b = np.arange(B)
    return b[np.lexsort((b % WAVE, -((b % CHUNK) // WAVE), b // CHUNK))]


def chunk_swapped_order(B):
    """Position order with the 256-chunks taken backwards."""
    b = np.arange(B)
    return b[np.lexsort((b % CHUNK, -(b // CHUNK)))]


# (e) frame geometry: Xp around the 32-pixel block, nrows a multiple of 8 or not; the batch hangs over all four edges of the
# object and leaves padded rows above and below itself untouched
def _frame_case(P, Xp, nrows, seed, Z=3):
    Py, Px = probe_shape(P)
    obj, pads = (nrows - 5, Xp - 5, Z), ((5, 5), (3, 2))
    g = make_geom(obj, P, pads)
    return case(P, obj, pads, pos=spread_positions(seed, 11, g, ylim=(-3, nrows - 3 - Py)), seed=seed)


FRAME_CASES = collections.OrderedDict([
    ('Xp31_rows16', _frame_case(8, 31, 16, 81)),
    ('Xp32_rows19', _frame_case(8, 32, 19, 82)),
    ('Xp33_rows24', _frame_case(8, 33, 24, 83)),
    ('Xp65_rows27', _frame_case(8, 65, 27, 84)),
    ('p18_Xp45_rows29', _frame_case(18, 45, 29, 85)),                # LPW = 7, R2 = 9: no power of two in the index arithmetic
    ('p27_Xp64_rows40', _frame_case(27, 64, 40, 86)),                # R1 odd: [k][tid] rows
    ('generic40x24_Xp37_rows53', _frame_case((40, 24), 37, 53, 87)),
])

# (f) parts and windows: one batch in two and in three parts, the window two rows larger than the batch on either side
_PART_PADS = ((6, 6), (2, 2))
PART_CASE = case(8, (40, 30, 3), _PART_PADS, pos=spread_positions(91, 40, make_geom((40, 30, 3), 8, _PART_PADS), ylim=(-2, 34)), seed=91)
PART_SPLITS = {'two': [(0, 20), (20, 20)], 'three': [(0, 14), (14, 13), (27, 13)]}


def part_window(c):
    y = c['pos'][:, 0]
    return int(y.min()) - 2, int(y.max()) + c['geom'].Py + 2


# (g) lists built ahead: five batches of one plan, different positions each
# (two padded rows stay free above and below every batch: a window larger than the batch fits the frame)
_AHEAD_GEOM = make_geom((30, 33, 3), 8, ((3, 3), (2, 2)))
AHEAD_CASES = [case(8, (30, 33, 3), ((3, 3), (2, 2)), pos=spread_positions(100 + i, 11, _AHEAD_GEOM, ylim=(-1, 23)), seed=100 + i)
               for i in range(5)]
AHEAD_LARGER = case(8, (30, 33, 3), ((3, 3), (2, 2)), pos=spread_positions(110, 13, _AHEAD_GEOM, ylim=(-1, 23)), seed=110)

# (h) range passes: 150 positions, 70 of them on one pixel, in passes of 64 / 64 / 22
_RANGE_PADS = ((5, 5), (2, 2))
_RG = make_geom((50, 47, 3), 8, _RANGE_PADS)
_HOT = [(20 + i % 3, 18 + i % 4) for i in range(70)]                  # all 70 cover object pixels [22, 28) x [21, 26)
_COLD = [p for p in spread_positions(120, 400, _RG, ylim=(-3, 45)).tolist() if not (14 < p[0] < 28 and 13 < p[1] < 26)][:80]
RANGE_CASE = case(8, (50, 47, 3), _RANGE_PADS, seed=120, pos=shuffled(5, _HOT + _COLD))
RANGE_PASSES = [(0, 64), (64, 128), (128, 150)]

# (a) the producer: the real multislice at every tuned size, one generic field and one streamed plan
PRODUCER_CASES = [(n, 'tuned') for n in SIZES] + [((40, 24), 'generic'), ((40, 24), 'streamed')]


def producer_inputs(P, S=3, B=11, seed=0):
    """Inputs of one real minibatch (no oracle run: only the overlap-add of what the kernel produced is checked): object
    [Y, X, S, 2], positions over all four edges, probe [Py, Px] complex, target magnitudes [B, Py, Px]."""
    from tests import ms_matrix as MM
    Py, Px = probe_shape(P)
    r = np.random.default_rng([Py, Px, S, B, int(seed)])
    Y, X = Py + 9, Px + 13
    obj = np.stack([2e-3 * r.uniform(size=(Y, X, S)), 2e-4 * r.uniform(size=(Y, X, S))], -1)
    pos = MM.edge_positions(r, B, Y, X, Py, Px)
    probe = (0.5 + r.uniform(0, 1, (Py, Px))) * np.exp(1j * r.uniform(-np.pi, np.pi, (Py, Px)))
    target = (np.abs(r.standard_normal((B, Py, Px))) * Py).astype(np.float32)
    return obj, pos, probe, target


ALL_SYNTHETIC = collections.OrderedDict()
for _grp in (STEP_CASES, COVER_CASES, LARGE_CASES, FRAME_CASES):
    ALL_SYNTHETIC.update(_grp)
ALL_SYNTHETIC['parts'] = PART_CASE
ALL_SYNTHETIC['range'] = RANGE_CASE
