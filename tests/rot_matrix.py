"""Every path of the rotation kernels (adm_rotate.hip, adm_rotcsr.hip) against two references (test infrastructure only: the
oracle is the checker, never the product).  Case tables, input builder, references and bars; the GPU tests are in
tests/test_gpu_rotation_matrix.py, and tests/test_rotation_matrix_coverage.py checks on the CPU -- from the kernel source and
the host table builder -- that the tables below reach every branch they claim.

References
  S    the oracle's float32 weights and indices (O.rotation_weights: the numbers the kernels form bit for bit), products and
       sums in float64.  Inputs are float32 on both sides.
  f64  O.rotate_fwd / O.rotate_adj in float64 (weights in float64 too), and their float32 forms for the 3x rule.

Bars
  1  per element, a theorem.  An output that is an initial value g0 plus n weighted inputs, evaluated in float32 in any order,
     with or without fused multiply-adds, obeys |out - S| <= gamma(n + 1) (|g0| + sum |w_j| |v_j|), gamma(k) = k u / (1 - k u),
     u = 2^-24: a term passes through its product's rounding, at most n - 1 inexact additions (the first one, to zero, is exact)
     and the addition to g0.  Forward: n = 4, g0 = 0.  Adjoint: n = entries of the voxel's CSR row.  R stacked angles:
     n = the rows' total, + R for the R `+=`.  No factor on top: the oracle's own float32 results, measured on the CPU with
     this module's inputs, reach 0.41 - 0.66 of the bound over the rows of CASES (0.43 - 0.48 stacked); a lost or doubled entry
     does not stay under it (tests/test_rotation_matrix_coverage.py shows both on the CPU).
  2  the 3x rule: rel(gpu, f64) <= 3 rel(f32 oracle, f64) + FLOOR, relative L2 over the planes written.  The float32 oracle's
     own error, measured on the CPU with this module's inputs (forward / adjoint into zeros):
         256 x 256, pi/4: 4.1e-8 / 8.8e-8       64 x 64, 0.7: 4.3e-8 / 6.1e-8       (power-of-two sizes: 0.7 - 1.5 u)
         200 x 120, 0.3: 4.3e-6 / 5.2e-6        384 x 384, pi/4: 3.9e-6 / 4.8e-6    37 x 53, 0.3: 1.3e-6 / 1.4e-6
         48 x 80, pi/4: 2.9e-6 / 3.3e-6         stacked 200 x 120, R = 3: 5.2e-6 / 4.9e-6
     (at sizes that are no power of two the float32 coordinate normalisation loses bits -- the same bits in the kernels, whose
     weights are the oracle's).  At the power-of-two sizes 3 x 4e-8 leaves little room for a sum taken in another order, so
     FLOOR = u = 2^-24 = 6.0e-8: about one more float32 oracle's worth of error.  Bar 1 allows each element gamma(5) ~ 5 u of
     its magnitude sum, so in L2 terms bar 2 with this floor (3 - 5 u in all) stays the tighter of the two there; the
     coords = NULL cases (weights 1, 0, 0, 0) have a float32 oracle error of zero and one rounding per element in the adjoint's
     `+=`: at most u (2.7e-8 measured for the oracle).
  3  adjointness, both sides from the GPU: |<R x, y> - <x, R^T y>| <= sum |y| bound1(R x) + sum |x| bound1(R^T y), inner
     products in float64 on the host.
  4  canaries, bit for bit: pads and planes outside [y_lo, y_hi) of obj_rot keep a sentinel, planes of grad_obj outside the
     range keep their values; the pads and the planes outside the range of grad_rot hold 1e30, so reading one shows under bar 1.
     Every path but the atomic one gives the same bits twice.
"""
import functools
import re

import numpy as np

from oracle import adorym_oracle as O
from adorym_amd.util import build_rotation_adjoint_csr, calculate_pad_len

U = 2.0 ** -24
FLOOR = U
P = 8                     # probe side of the plans: only its overhang matters here (pads)
SENTINEL = np.float32(-12345.678)
POISON = np.float32(1e30)

# --------------------------------------------------------------------------- what the launch code decides, restated
# (defaults = the constants of adm_rotate.hip / adm_rotcsr.hip / util.py; the coverage test parses them from the source,
# asserts they are these and recomputes every claim below from the parsed values)
STAGE_MAX = 1024          # ADM_STAGE_MAX: float2 per plane when four planes are staged
BOX_LIMIT = 4096          # boxes above it get bw = 0 (device and host builder)
RIM2_PLANES = (2, 4)      # `2 * per <= 4 * ADM_STAGE_MAX`: two planes per pass
FWD_CHUNK, FWD_MIN_BLOCKS = 32, 512
ADJ_CHUNK = 32            # rotate_adj_kernel's planes per block
NPL, NPL_MIN_BLOCKS, STACK_MIN_BLOCKS = 4, 1024, 2048

BOX_CLASSES = ('nobox', 'interior', 'rim2', 'rim1')


def n_patches(X, Z):
    return ((X + 15) // 16) * ((Z + 15) // 16)


def fwd_y_chunk(X, Z, ny, chunk=FWD_CHUNK, min_blocks=FWD_MIN_BLOCKS):
    """y planes per block of rotate_fwd_kernel (adm_rotate_fwd)."""
    while chunk > 1 and n_patches(X, Z) * ((ny + chunk - 1) // chunk) < min_blocks:
        chunk >>= 1
    return chunk


def stack_npl(X, Z, Yb, R, scratch, npl=NPL, min_blocks=NPL_MIN_BLOCKS, stack_min_blocks=STACK_MIN_BLOCKS):
    """planes per block of rotate_adj_staged_stack_kernel (adm_rotate_adj_staged_stack)."""
    if scratch:
        while npl > 1 and n_patches(X, Z) * ((Yb + npl - 1) // npl) * R < stack_min_blocks:
            npl >>= 1
    else:
        while npl > 1 and n_patches(X, Z) * ((Yb + npl - 1) // npl) < min_blocks:
            npl >>= 1
    return npl


def box_class(bw, bh, stage_max=STAGE_MAX, rim2=RIM2_PLANES):
    """The branch of rotate_adj_staged_kernel / rotate_adj_staged_stack_kernel (npl >= 2) a patch's box takes."""
    per = int(bw) * int(bh)
    if bw == 0:
        return 'nobox'
    if per <= stage_max:
        return 'interior'
    return 'rim2' if rim2[0] * per <= rim2[1] * stage_max else 'rim1'


# --------------------------------------------------------------------------- case tables
PI = np.pi
ALL4 = frozenset(BOX_CLASSES)
# name: (Y, X, Z), theta (None: coords = NULL), partial y range (y_lo > 0, length % 4 in {1, 2, 3}), y_chunk of the forward
# launch over the whole range, box classes of the staged tables.  Every row runs forward and every adjoint path, whole range
# into zeros and partial range into a non-zero gradient; positions hang over the edges: pads (3, 1) x (2, 4).
CASES = {
    'x200z120_t0.3':  ((9, 200, 120), 0.3, (2, 9), 2, ALL4),                       # all four classes; rows of 2753 entries
    'x384z384_pi4':   ((5, 384, 384), PI / 4, (1, 4), 32, ALL4),                   # square with no-box patches; 32 with a tail
    'x256z256_pi4':   ((9, 256, 256), PI / 4, (3, 8), 8, frozenset({'interior', 'rim2', 'rim1'})),
    'x48z80_pi4':     ((35, 48, 80), PI / 4, (5, 35), 1, frozenset({'interior', 'rim2', 'rim1'})),     # > 32 planes: two atomic chunks
    'x80z48_pi4':     ((7, 80, 48), PI / 4, (1, 7), 1, frozenset({'interior', 'rim1'})),
    'x37z53_t0.3':    ((7, 37, 53), 0.3, (2, 5), 1, frozenset({'interior', 'rim2'})),                  # patch tails along both axes
    'x64z64_t0.7':    ((6, 64, 64), 0.7, (1, 4), 1, frozenset({'interior'})),                          # no patch tails
    'x40z72_t0':      ((6, 40, 72), 0.0, (1, 6), 1, frozenset({'interior', 'rim1'})),
    'x40z72_halfpi':  ((6, 40, 72), PI / 2, (1, 6), 1, frozenset({'interior'})),
    'x40z72_pi':      ((6, 40, 72), PI, (1, 6), 1, frozenset({'interior'})),
    'x40z72_twopi':   ((6, 40, 72), 2 * PI, (1, 6), 1, frozenset({'interior', 'rim1'})),
    'x40z72_t4.0':    ((6, 40, 72), 4.0, (1, 6), 1, frozenset({'interior', 'rim2'})),                  # above pi
    'x40z24_nullcoords':  ((6, 40, 24), None, (1, 4), 1, None),                    # coords = NULL, Z >= 16: the general kernels
    'x50z9_identity':     ((6, 50, 9), None, (2, 5), 1, None),                     # coords = NULL, Z < 16: identity_*_kernel
    'x33z1_identity':     ((7, 33, 1), None, (1, 6), 1, None),
}
ROTATED = [n for n, c in CASES.items() if c[1] is not None]
ADJ_PATHS = ('atomic', 'csr_lanes_z', 'csr_lanes_x', 'staged')          # csr_lanes_z: lanes_along_x = 0
NOBOX_CASES = [n for n, c in CASES.items() if c[4] and 'nobox' in c[4]]

# the stacked forms: 200 x 120, R = 3 angles whose tables all hold no-box, rim2 and rim1 patches; name: (Yb, scratch, npl)
STACK_XZ, STACK_THETAS = (200, 120), (0.3, 2.0, 4.0)
STACK_CASES = {
    'sequential_yb6_npl1':  (6, False, 1),
    'sequential_yb21_npl2': (21, False, 2),        # 21 % 2: a short last group
    'sequential_yb41_npl4': (41, False, 4),        # 41 % 4: a short last group
    'scratch_yb6_npl1':     (6, True, 1),
    'scratch_yb14_npl2':    (14, True, 2),
    'scratch_yb41_npl4':    (41, True, 4),
}

# every rotation entry point of the C ABI, the kernels it launches, and the test of test_gpu_rotation_matrix.py that puts it
# under bars 1 and 2 (the table builders: under bit-equality with the host builders, and under every staged case's bars)
ENTRY_POINTS = {
    'adm_rotate_fwd': (('rotate_fwd_kernel', 'identity_fwd_kernel'), 'test_forward_vs_references'),
    'adm_rotate_adj': (('rotate_adj_kernel', 'identity_adj_kernel'), 'test_adjoint_vs_references'),
    'adm_rotate_adj_csr': (('rotate_adj_csr_kernel<true>', 'rotate_adj_csr_kernel<false>'), 'test_adjoint_vs_references'),
    'adm_rotate_adj_staged': (('rotate_adj_staged_kernel',), 'test_adjoint_vs_references'),
    'adm_rotate_fwd_stack': (('rotate_fwd_stack_kernel',), 'test_stacked_rotations_vs_references'),
    'adm_rotate_adj_staged_stack': (('rotate_adj_staged_stack_kernel', 'stack_sum_kernel'), 'test_stacked_rotations_vs_references'),
    'adm_rotation_csr_build': (('rotcsr_init_kernel', 'rotcsr_emit_kernel', 'rotcsr_boxes_kernel', 'rotcsr_finish_kernel'),
                               'test_device_built_tables_equal_host_builder_at_nobox_cases'),
    'adm_rotation_csr_scratch_bytes': ((), 'test_device_built_tables_equal_host_builder_at_nobox_cases'),
    'adm_rotation_table_build': (('rot_table_kernel',), 'test_device_built_tables_equal_host_builder_at_nobox_cases'),
}


# --------------------------------------------------------------------------- geometry, inputs
def positions(Y, X):
    """Two probe positions hanging over all four edges: pads ((3, 1), (2, 4))."""
    return np.array([(-3, -2), (Y - P + 1, X - P + 4)])


def pads_of(size):
    return calculate_pad_len(size, positions(size[0], size[1]), (P, P))


def frame(size):
    """(Yp, Xp, pad_y0, pad_x0) of the padded rotated frame of a plan of this size."""
    (py0, py1), (px0, px1) = [(int(a), int(b)) for a, b in pads_of(size)]
    return size[0] + py0 + py1, size[1] + px0 + px1, py0, px0


def _seed(name):
    return [ord(ch) for ch in name]


def fields(name, size):
    """O(1) random float32 fields (not smooth: smooth fields hide index errors): object, rotated-frame cotangent, the
    gradient buffer's initial contents."""
    r = np.random.default_rng(_seed(name))
    shape = tuple(size) + (2,)
    return ((0.5 + r.standard_normal(shape)).astype(np.float32), r.standard_normal(shape).astype(np.float32),
            r.standard_normal(shape).astype(np.float32))


def coords_of(size, theta):
    return None if theta is None else O.rotation_coords(size, np.float32(theta))


def to_frame(a, size, fill):
    """[Y, X, Z, 2] in the reference layout -> the padded slice-major [Z][Yp][Xp][2] buffer, ``fill`` in the pads."""
    Y, X, Z = size
    Yp, Xp, py0, px0 = frame(size)
    out = np.full((Z, Yp, Xp, 2), fill, np.float32)
    out[:, py0:py0 + Y, px0:px0 + X] = np.transpose(a, (2, 0, 1, 3))
    return out


def from_frame(buf, size):
    Y, X, Z = size
    _, _, py0, px0 = frame(size)
    return np.ascontiguousarray(np.transpose(buf[:, py0:py0 + Y, px0:px0 + X], (1, 2, 0, 3)))


def frame_mask(size, y_lo, y_hi):
    """True where the padded buffer holds a voxel of planes [y_lo, y_hi) of the object (False: pads, other planes)."""
    Y, X, Z = size
    Yp, Xp, py0, px0 = frame(size)
    m = np.zeros((Z, Yp, Xp, 2), bool)
    m[:, py0 + y_lo:py0 + y_hi, px0:px0 + X] = True
    return m


def host_tables(size, theta, staged):
    Yp, Xp, _, px0 = frame(size)
    return build_rotation_adjoint_csr(coords_of(size, theta), size, Yp, Xp, px0, staged=staged)


def patch_classes(size, theta, **limits):
    """(class of every 16 x 16 patch [n_patch], CSR row lengths [X*Z], patch of every voxel [X*Z]) from the host builder."""
    _, X, Z = size
    ptr, _, _, _, boxes = host_tables(size, theta, True)
    cls = np.array([box_class(b[2], b[3], **limits) for b in boxes])
    t = np.arange(X * Z)
    return cls, np.diff(ptr), ((t % Z) // 16) * ((X + 15) // 16) + (t // Z) // 16


# --------------------------------------------------------------------------- the references
def gamma(k):
    k = np.asarray(k, np.float64)
    return k * U / (1 - k * U)


def operator(size, theta):
    """(idx [4, X*Z], w float32 [4, X*Z]) of the angle; coords = NULL: weights 1, 0, 0, 0 on the voxel itself."""
    _, X, Z = size
    if theta is None:
        idx = np.tile(np.arange(X * Z), (4, 1))
        w = np.zeros((4, X * Z), np.float32)
        w[0] = 1
        return idx, w
    return O.rotation_weights(coords_of(size, theta), X, Z, 'float32')


def sharp_forward(op, obj32):
    """Reference S of R x and the bar-1 bound per element, [Y, X, Z, 2] float64 each."""
    idx, w = op
    assert obj32.dtype == np.float32 and w.dtype == np.float32
    Y, X, Z, C = obj32.shape
    o = obj32.reshape(Y, X * Z, C).astype(np.float64)
    w = w.astype(np.float64)
    S = sum(o[:, idx[k], :] * w[k][None, :, None] for k in range(4))
    mag = sum(np.abs(o[:, idx[k], :]) * np.abs(w[k])[None, :, None] for k in range(4))
    return S.reshape(obj32.shape), (gamma(5) * mag).reshape(obj32.shape)


def sharp_adjoint_terms(op, cot32):
    """(R^T y, sum |w| |y|, entries per voxel) with float32 weights, sums in float64: [Y, X, Z, 2] x 2, [X * Z]."""
    idx, w = op
    assert cot32.dtype == np.float32 and w.dtype == np.float32
    Y, X, Z, C = cot32.shape
    g = cot32.reshape(Y, X * Z, C).astype(np.float64)
    keep = w.ravel() != 0
    tg = idx.ravel()[keep]
    sp = np.tile(np.arange(X * Z), 4)[keep]
    ww = w.ravel()[keep].astype(np.float64)
    n = np.bincount(tg, minlength=X * Z)
    S, mag = np.empty((Y, X * Z, C)), np.empty((Y, X * Z, C))
    for y in range(Y):
        for c in range(C):
            v = g[y, sp, c]
            S[y, :, c] = np.bincount(tg, weights=ww * v, minlength=X * Z)
            mag[y, :, c] = np.bincount(tg, weights=ww * np.abs(v), minlength=X * Z)
    return S.reshape(cot32.shape), mag.reshape(cot32.shape), n


def sharp_adjoint(op, cot32, g0_32):
    """Reference S of g0 + R^T y and the bar-1 bound per element."""
    S, mag, n = sharp_adjoint_terms(op, cot32)
    _, X, Z, _ = cot32.shape
    g0 = g0_32.astype(np.float64)
    return g0 + S, gamma(n + 1).reshape(1, X, Z, 1) * (np.abs(g0) + mag)


def rel(a, b):
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    return np.linalg.norm(a - b) / np.linalg.norm(b)


class CaseRefs(object):
    """Inputs and CPU references of one row of CASES (cached: the forward and the four adjoint paths share them)."""

    def __init__(self, name):
        self.name = name
        self.size, self.theta, self.partial, self.y_chunk, self.classes = CASES[name]
        self.obj, self.cot, self.g0 = fields(name, self.size)
        self.coords = coords_of(self.size, self.theta)
        self.op = operator(self.size, self.theta)
        self.fwd_S, self.fwd_bound = sharp_forward(self.op, self.obj)
        self._adj = sharp_adjoint_terms(self.op, self.cot)
        o64, c64 = self.obj.astype(np.float64), self.cot.astype(np.float64)
        if self.theta is None:
            self.fwd_64, self.fwd_32, self.adj_64, self.adj_32 = o64, self.obj, c64, self.cot
        else:
            self.fwd_64, self.fwd_32 = O.rotate_fwd(o64, self.coords, 'float64'), O.rotate_fwd(self.obj, self.coords, 'float32')
            self.adj_64, self.adj_32 = O.rotate_adj(c64, self.coords, 'float64'), O.rotate_adj(self.cot, self.coords, 'float32')

    def adjoint(self, g0):
        """(S, bound, f64, f32 oracle) of g0 + R^T cot for a float32 g0."""
        S, mag, n = self._adj
        _, X, Z = self.size
        g64 = g0.astype(np.float64)
        return (g64 + S, gamma(n + 1).reshape(1, X, Z, 1) * (np.abs(g64) + mag), g64 + self.adj_64,
                (g0 + self.adj_32.astype(np.float32)).astype(np.float32))


@functools.lru_cache(maxsize=4)
def case_refs(name):
    return CaseRefs(name)


class StackRefs(object):
    """Inputs and references of the stacked forms at one Yb: block r of the stacked rotated object is R_r x, and the one
    real gradient is g0 + sum_r R_r^T (block r of the stacked cotangent), the angles summed in float64."""

    def __init__(self, Yb):
        X, Z = STACK_XZ
        R = len(STACK_THETAS)
        self.Yb, self.R = Yb, R
        self.real, self.size = (Yb, X, Z), (R * Yb, X, Z)
        self.obj, _, self.g0 = fields('stack%d' % Yb, self.real)
        _, self.cot, _ = fields('stackcot%d' % Yb, self.size)
        fS, fB, f64, f32 = [], [], [], []
        aS, amag, n = 0, 0, 0
        a64, a32 = 0, self.g0.copy()
        o64 = self.obj.astype(np.float64)
        for r, th in enumerate(STACK_THETAS):
            op, coords = operator(self.real, th), coords_of(self.real, th)
            s, b = sharp_forward(op, self.obj)
            fS.append(s); fB.append(b)
            f64.append(O.rotate_fwd(o64, coords, 'float64')); f32.append(O.rotate_fwd(self.obj, coords, 'float32'))
            blk = self.cot[r * Yb:(r + 1) * Yb]
            s, m, k = sharp_adjoint_terms(op, blk)
            aS, amag, n = aS + s, amag + m, n + k
            a64 = a64 + O.rotate_adj(blk.astype(np.float64), coords, 'float64')
            a32 = (a32 + O.rotate_adj(blk, coords, 'float32').astype(np.float32)).astype(np.float32)      # R launches' `+=`
        self.fwd_S, self.fwd_bound = np.concatenate(fS), np.concatenate(fB)
        self.fwd_64, self.fwd_32 = np.concatenate(f64), np.concatenate(f32)
        self._adj = (aS, amag, n, a64, a32)

    def adjoint(self, zero):
        """(S, bound, f64, f32 oracle) of g0 + sum_r R_r^T cot_r; ``zero``: g0 = 0 (the adjointness run)."""
        aS, amag, n, a64, a32 = self._adj
        _, X, Z = self.real
        g64 = np.zeros_like(aS) if zero else self.g0.astype(np.float64)
        f32 = None if zero else a32                    # (bar 2 is applied to the g0 != 0 run)
        return g64 + aS, gamma(n + self.R).reshape(1, X, Z, 1) * (np.abs(g64) + amag), g64 + a64, f32


@functools.lru_cache(maxsize=2)
def stack_refs(Yb):
    return StackRefs(Yb)


# --------------------------------------------------------------------------- the bars
def check_bar1(got, S, bound, what):
    """Element-wise, no factor.  On failure: the worst element, for the patch / plane / box-class post-mortem."""
    err = np.abs(got.astype(np.float64) - S)
    bad = err > bound
    if bad.any():
        ratio = np.where(bound > 0, err / np.where(bound > 0, bound, 1), np.where(err > 0, np.inf, 0))
        y, x, z, c = np.unravel_index(np.argmax(ratio), ratio.shape)
        raise AssertionError('%s: bar 1 violated at %d elements; worst (y, x, z, c) = (%d, %d, %d, %d), patch (%d, %d): got %r, S %r, '
                             '|err| / bound = %.3g' % (what, bad.sum(), y, x, z, c, x // 16, z // 16, got[y, x, z, c], S[y, x, z, c],
                                                       ratio[y, x, z, c]))
    with np.errstate(divide='ignore', invalid='ignore'):
        return float(np.nanmax(np.where(bound > 0, err / bound, 0)))


def check_bar2(got, f64, f32, what):
    e, e32 = rel(got, f64), rel(f32, f64)
    assert e <= 3 * e32 + FLOOR, '%s: bar 2: rel(gpu, f64) = %.3e, rel(f32 oracle, f64) = %.3e, floor %.1e' % (what, e, e32, FLOOR)
    return e, e32


def check_adjointness(fwd_gpu, adj_gpu, x, y, fwd_bound, adj_bound, what):
    """<R x, y> against <x, R^T y>, both operators from the GPU, the inner products in float64."""
    x, y = x.astype(np.float64), y.astype(np.float64)
    lhs, rhs = np.sum(fwd_gpu.astype(np.float64) * y), np.sum(x * adj_gpu.astype(np.float64))
    tol = np.sum(np.abs(y) * fwd_bound) + np.sum(np.abs(x) * adj_bound)
    assert abs(lhs - rhs) <= tol, '%s: <Rx, y> = %.17g, <x, R^T y> = %.17g, difference %.3e > %.3e' % (what, lhs, rhs, abs(lhs - rhs), tol)


def same_bits(a, b):
    return np.array_equal(np.ascontiguousarray(a).view(np.uint32), np.ascontiguousarray(b).view(np.uint32))


# --------------------------------------------------------------------------- source parsing (coverage test)
def function_body(src, signature):
    """Text of the brace-balanced body of the first function whose head matches ``signature``."""
    m = re.search(signature, src)
    assert m, signature
    i = src.index('{', m.end())
    depth = 0
    for j in range(i, len(src)):
        depth += {'{': 1, '}': -1}.get(src[j], 0)
        if depth == 0:
            return src[i:j + 1]
    raise AssertionError('unbalanced body: ' + signature)
