"""Case tables, inputs, float32 mirrors and fp64 references of the element-wise matrix (tests/test_gpu_elementwise_matrix.py): the
optimiser steps of adm_optim.h / adm_optimize.hip and the regularisers of adm_regularize.hip at every flag, range and launch
geometry.  tests/test_elementwise_coverage.py (CPU) parses the constants below from the sources and fails when a table no longer
has a case on both sides of one of them, or when a kernel or entry point of the two files has no row in KERNELS / ENTRY_POINTS.

Mirrors.  adam_value, gd_value and momentum_value are compiled with contraction off and use + - * / and sqrtf only, all of them
correctly rounded in the build, so the oracle run in float32 (NumPy rounds every operation once, in the same order) followed by
O.apply_constraints gives the kernel's BITS.  The fp64 run of the same oracle functions is the reference that does not share
the mirror's precision: 2e-6 relative L2, the bar of tests/test_gpu_parity.py.

Lattice objects.  The real_imag regularisers take signs of differences (u - u', ph - ph', |o| - mean|o|); the lattice makes
u = re^2 + im^2 exact in float32, so ties are exact zeros in both precisions, and the guards of lattice_conditions keep every
other argument of a sign further from zero than float32 can move it.  No voxel is excluded from any comparison.
"""
import numpy as np

from oracle import adorym_oracle as O

# ---- constants of the sources (parsed and compared by tests/test_elementwise_coverage.py) ---------------------------------------
NONNEG, ZERO_CH0, ZERO_CH1 = 1, 2, 4        # ADM_FLAG_* (include/adm.h)
THREADS = 256
STREAM_BLOCKS = 4096                        # stream_grid (adm_host.h): at most 4096 blocks of 256 threads
STREAM_CAP = STREAM_BLOCKS * THREADS        # beyond it a grid-stride loop makes a second trip
BLOCK_CAP = 1024                            # ri_stats_launch / adm_rwl1_update: nb > 1024 -> 1024
REG_THREADS = (96, 192)                     # reg_threads: obj_z >= 192 ? 256 : (obj_z >= 96 ? 128 : 64)
REDUCE_THREADS = 1024                       # reg_value_reduce_kernel: one block of 1024 over the (y, x) row partials
SMALL_WHOLE_RPT = 8                         # rows per thread of the register-resident drift guard
SMALL_CHUNK = (4096, 256, 2048)             # small_chunk: n > 4096 ? 256 : 2048
SMALL_PARAMS_MAX = 6                        # ADM_SMALL_PARAMS_MAX
BIG = STREAM_CAP + 257


def stream_grid(n):
    b = (n + THREADS - 1) // THREADS
    return min(b, STREAM_BLOCKS) if b else 1


def reg_threads(z):
    return 256 if z >= REG_THREADS[1] else (128 if z >= REG_THREADS[0] else 64)


def small_chunk(n):
    return SMALL_CHUNK[1] if n > SMALL_CHUNK[0] else SMALL_CHUNK[2]


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def rel(a, b):
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    nb = np.linalg.norm(b)
    return np.linalg.norm(a - b) / nb if nb else float(np.linalg.norm(a - b))


# ---- block_sum_f32 and center_rows_kernel in float32 (moved here from tests/test_gpu_elementwise.py) ----------------------------
def block_sum_mirror(v, descending=False):
    """block_sum_f32 of 256 per-thread float32 values: inside each wave of 64 lanes v[l] += v[l + off] for off = 32 ... 1 (lane 0
    ends with the wave's sum), then the wave sums one by one, ascending (descending: the order the kernel must NOT use)."""
    v = np.array(v, np.float32).reshape(4, 64)
    for off in (32, 16, 8, 4, 2, 1):
        v[:, :off] = v[:, :off] + v[:, off:2 * off]
    red = v[:, 0][::-1] if descending else v[:, 0]
    t = red[0]
    for w in range(1, 4):
        t = np.float32(t + red[w])
    return t


def center_rows_mirror(x, descending=False):
    x = np.array(x, np.float32)
    n_rows, n_cols = x.shape
    per = -(-n_rows // 256)
    for c in range(n_cols):
        col = np.zeros(per * 256, np.float32)
        col[:n_rows] = x[:, c]
        acc = np.zeros(256, np.float32)
        for j in range(per):                           # thread t adds the rows t, t + 256, ... in this order (+0 where it has none)
            acc = acc + col[j * 256:(j + 1) * 256]
        mu = np.float32(block_sum_mirror(acc, descending) / np.float32(n_rows))
        x[:, c] = x[:, c] - mu
    return x


# ---- optimiser steps ------------------------------------------------------------------------------------------------------------
OPTIMISERS = ('adam', 'gd', 'momentum')
HYPER = dict(step=1e-2, b1=0.9, b2=0.999, eps=1e-7, gamma=0.9)
I_BATCHES = (0, 1, 2, 7, 91, 1000, 100000)
N_FLAGS = 2 * 333
RANGE_FLAGS = NONNEG | ZERO_CH0

# (optimiser, n, lo, hi, flags, mask present, i_batch)
FLAG_CASES = [(o, N_FLAGS, 0, N_FLAGS, f, mk, 3) for o in OPTIMISERS for f in range(8) for mk in (False, True)]
RANGES = [(N_FLAGS, 7, 93), (N_FLAGS, 7, 94), (N_FLAGS, 8, 93),                          # (odd, odd), (odd, even), (even, odd)
          (N_FLAGS, 3, 4), (N_FLAGS, 3, 258), (N_FLAGS, 3, 259), (N_FLAGS, 3, 260),      # hi - lo = 1, 255, 256, 257
          (N_FLAGS, 5, 5), (N_FLAGS, 93, 7),                                             # hi == lo, hi < lo: nothing changes
          (BIG, 3, BIG)]                                                                 # the second trip of the grid-stride loop
RANGE_CASES = [(o, n, lo, hi, RANGE_FLAGS, True, 3) for o in OPTIMISERS for n, lo, hi in RANGES]
I_BATCH_CASES = [('adam', N_FLAGS, 0, N_FLAGS, RANGE_FLAGS, True, ib) for ib in I_BATCHES]
OPT_CASES = FLAG_CASES + RANGE_CASES + I_BATCH_CASES
AXPY_CASES = [(a, n) for a in (1.0, -0.375) for n in (1, 257, BIG)]


def case_id(c):
    return '-'.join(str(v) for v in c)


def seeded(shape, seed, lo=-20, hi=3):
    """Non-zero values of mixed sign over the binades 2^lo ... 2^hi."""
    r = np.random.default_rng(seed)
    return (r.standard_normal(shape) * np.exp2(r.integers(lo, hi + 1, shape))).astype(np.float32)


def opt_inputs(n, seed=11):
    """x, g, m, v >= 0 of n elements, a 0/1 mask per pair, and the planted elements: `still` (g = m = v = 0: the step is zero
    and x keeps its bits apart from the constraints) and `negative` (x < 0: NONNEG gives +0, `* 0.f` gives -0)."""
    x, g, m = seeded(n, seed), seeded(n, seed + 1), seeded(n, seed + 2)
    v = np.abs(seeded(n, seed + 3))
    still = np.unique([i for i in (0, 1, 20, 21, n // 3, n // 3 + 1, 100, 101, n - 1) if n > 32]).astype(int)
    negative = np.unique([i for i in (1, 2, 3, 21, 22, 23, n // 2, n // 2 + 1, 100, n - 2) if n > 32]).astype(int)
    for a in (g, m, v):
        a[still] = 0
    x[negative] = -np.abs(x[negative])
    mask = np.random.default_rng(seed + 4).integers(0, 2, (n + 1) // 2).astype(np.float32)
    return dict(x=x, g=g, m=m, v=v, mask=mask, still=still, negative=negative)


def constrain_mirror(x, flags, mask):
    """constrain() of adm_optim.h on a flat array whose element i is channel i & 1 of pair i >> 1: O.apply_constraints."""
    n = x.size
    y = np.zeros(n + (n & 1), x.dtype)
    y[:n] = x
    y = y.reshape(-1, 2)
    y = O.apply_constraints(y, non_negativity=bool(flags & NONNEG), object_type='absorption_only' if flags & ZERO_CH0 else 'normal')
    if flags & ZERO_CH1:
        y = O.apply_constraints(y, object_type='phase_only')
    if mask is not None:
        y = O.apply_constraints(y, mask=mask)
    return np.ascontiguousarray(y).reshape(-1)[:n]


def adam_scalars(i_batch, b1, b2):
    """q1, q2 as adam_scalars of adm_optim.h forms them: repeated multiplication in double, then a cast."""
    p1 = p2 = 1.0
    for _ in range(i_batch + 1):
        p1 *= b1
        p2 *= b2
    return np.float32(1.0 - p1), np.float32(1.0 - p2)


def adam_spelled_out(x, g, m, v, i_batch, step, b1, b2, eps):
    """adam_value operation by operation in float32, with adam_scalars' q1, q2 (the oracle in float32 must equal it)."""
    f = np.float32
    q1, q2 = adam_scalars(i_batch, b1, b2)
    mv = f(b1) * m
    mv = mv + f(1.0 - b1) * g
    vv = f(b2) * v
    vv = vv + f(1.0 - b2) * (g * g)
    mhat = mv / q1
    vhat = vv / q2
    d = f(step) * mhat / (np.sqrt(vhat) + f(eps))
    return x - d, mv, vv


def step_reference(opt, inp, lo, hi, flags, with_mask, i_batch, dtype):
    """{name: array} after one step on [lo, hi) in `dtype` (float32: the mirror; float64: the reference): the oracle's step on the
    whole array, the constraints at the absolute index, then everything outside the range put back."""
    h = HYPER
    a = {k: inp[k].astype(dtype) for k in ('x', 'g', 'm', 'v')}
    mask = inp['mask'].astype(dtype) if with_mask else None
    if opt == 'adam':
        x, m, v = O.adam_step(a['x'], a['g'], a['m'], a['v'], i_batch, h['step'], h['b1'], h['b2'], h['eps'])
        new = dict(x=x, m=m, v=v)
    elif opt == 'momentum':
        x, v = O.momentum_step(a['x'], a['g'], a['v'], h['step'], h['gamma'])
        new = dict(x=x, v=v)
    else:
        new = dict(x=O.gd_step(a['x'], a['g'], 0, h['step'], dynamic_rate=False))
    new['x'] = constrain_mirror(new['x'], flags, mask)
    e = np.arange(a['x'].size)
    inside = (e >= lo) & (e < hi)
    return {k: np.where(inside, val, a[k]).astype(dtype) for k, val in new.items()}


# ---- adm_adam_step_small: ADM_SMALL_PARAMS_MAX arrays in one call ---------------------------------------------------------------
SMALL_ARRAYS = [
    dict(n=1, center_cols=0, pin_n=0, step=1e-2),              # one element
    dict(n=2049, center_cols=0, pin_n=0, step=3e-3),           # two chunks of 2048
    dict(n=4097, center_cols=0, pin_n=0, step=1e-3),           # 17 chunks of 256
    dict(n=4097, center_cols=0, pin_n=300, step=2e-2),         # the pin crosses a chunk boundary
    dict(n=2 * 2048, center_cols=2, pin_n=5, step=5e-3),       # register-resident drift guard, the pin after the re-centring
    dict(n=3 * 100, center_cols=3, pin_n=4, step=7e-3),        # the generic drift guard
]
EMPTY = dict(n=0, center_cols=0, pin_n=0, step=1e-2)           # a zero-length element-wise array
SMALL_CALLS = {'forward': [0, 1, 2, 3, 4, 5], 'reversed': [5, 4, 3, 2, 1, 0], 'zero_length': [0, 3, EMPTY, 4, 5, 2]}
SMALL_I_BATCH = 3


def small_inputs(k, spec):
    inp = opt_inputs(max(spec['n'], 1), seed=40 + 7 * k)
    inp = {name: inp[name][:spec['n']] for name in ('x', 'g', 'm', 'v')}
    inp['pin'] = seeded(max(spec['pin_n'], 1), 90 + k, -3, 3)
    return inp


def small_mirror(spec, inp, zero_grad):
    """Adam, then center_rows, then the pin, then the zero fill: {x, g, m, v} in float32."""
    h = HYPER
    if spec['n'] == 0:
        return {k: inp[k].copy() for k in ('x', 'g', 'm', 'v')}
    x, m, v = O.adam_step(inp['x'], inp['g'], inp['m'], inp['v'], SMALL_I_BATCH, spec['step'], h['b1'], h['b2'], h['eps'])
    if spec['center_cols']:
        x = center_rows_mirror(x.reshape(-1, spec['center_cols'])).reshape(-1)
    x = x.copy()
    x[:spec['pin_n']] = inp['pin'][:spec['pin_n']]
    return dict(x=x, g=np.zeros_like(inp['g']) if zero_grad else inp['g'].copy(), m=m, v=v)


def small_blocks(spec):
    if spec['center_cols']:
        return 1
    c = small_chunk(spec['n'])
    return (spec['n'] + c - 1) // c


def small_register_resident(spec):
    return 0 < spec['center_cols'] <= 2 and spec['n'] // spec['center_cols'] <= THREADS * SMALL_WHOLE_RPT


# ---- delta_beta regulariser: the launch shapes tests/test_gpu_elementwise.py leaves out -----------------------------------------
DB_SHAPES = [(2, 2, 257), (2, 3, 300),                 # the second trip of the z loop, partial
             (2, 2, 95), (2, 2, 191), (2, 2, 192),     # both sides of reg_threads' thresholds (96 is in test_gpu_elementwise.py)
             (33, 32, 3)]                              # 1056 row partials: the second trip of reg_value_reduce_kernel
DB_ALPHAS = [(.7, .3, 0.), (0., 0., .5), (.7, .3, .5)]
DB_RANGE_SHAPE = (2, 3, 300)                           # 3600 floats, planes of 1800, rows of 600
DB_RANGE = (1121, 2961)                                # odd ends inside planes, both in the second trip of the z loop (z = 260, 280)
DB_WINDOWS = {'empty': (0, 0), 'interior': (1500, 2500), 'everything': (0, 3600)}

# ---- real_imag regularisers on a lattice object ---------------------------------------------------------------------------------
RI_SHAPES = [(1, 1, 1), (2, 2, 2), (1, 5, 7), (5, 1, 7), (5, 7, 1), (4, 8, 8), (1, 1, 257), (5, 7, 300), (4, 257, 257)]
RI_BIG = (4, 1030, 257)                                # 1 058 840 voxels: past stream_grid's cap
RI_ALPHAS = [(.8, .3, 0.), (0., 0., .7), (.8, .3, .7)]
RI_CASES = [(s, a) for s in RI_SHAPES for a in RI_ALPHAS] + [(RI_BIG, RI_ALPHAS[2])]
RWL1_SHAPES = [(3, 4, 5), (1, 1, 257), (4, 257, 257), (4, 1030, 257)]
RWL1_ALPHAS = (.8, .3)
UNKNOWN_TYPES = ('delta_beta', 'real_imag')


def lattice_object(shape, seed=21, reweighted=False):
    """re, im = integers / 64.  Plain: both in [-96, 96], voxels with |o| < 1/2 moved by +1 in re, a voxel copied onto its
    +z, +x and +y neighbour at a few places (sgn(0) = 0 in the TV terms), and a voxel on the ray of a different neighbour moved by
    1 / 64 in re, away from zero (in im where im = 0).  Reweighted L1: re in [16, 160], |im| >= 1 (the joint
    mean is positive, no component is zero, the weights stay within about 2^8 of each other)."""
    r = np.random.default_rng(seed)
    re, im = r.integers(-96, 97, shape), r.integers(-96, 97, shape)
    if reweighted:
        re = r.integers(16, 161, shape)
        im = np.where(im == 0, 1, im)
    else:
        re = np.where(re * re + im * im < 32 * 32, re + 64, re)
        V = int(np.prod(shape))
        flat_re, flat_im = re.reshape(-1).copy(), im.reshape(-1).copy()
        for k in range(min(12, max(1, V // 8))):
            y, x, z = np.unravel_index((k * 7919 + 3) % V, shape)
            for d in ((0, 0, 1), (0, 1, 0), (1, 0, 0)):
                j = np.ravel_multi_index(((y + d[0]) % shape[0], (x + d[1]) % shape[1], (z + d[2]) % shape[2]), shape)
                i = np.ravel_multi_index((y, x, z), shape)
                flat_re[j], flat_im[j] = flat_re[i], flat_im[i]
        re, im = flat_re.reshape(shape), flat_im.reshape(shape)
        for _ in range(50):                            # no neighbour on the same ray at another modulus (see phase_ties_apart)
            bad = phase_ties_apart(re, im)
            if not bad.any():
                break
            re, im = np.where(bad & (im != 0), re + np.where(re >= 0, 1, -1), re), np.where(bad & (im == 0), 1, im)
    return (np.stack([re, im], -1) / 64.0).astype(np.float32)


def phase_ties_apart(re, im):
    """Voxels whose -1 neighbour along some axis lies on the same ray from the origin at another modulus (integers re, im): their
    phases are equal in exact arithmetic, but an atan2f that divides with rcp and a product need not return the same float for
    3 / 7 and 9 / 21, and the sign of a difference of 1 ulp is nobody's error.  The lattice keeps phase ties to equal voxels."""
    bad = np.zeros(re.shape, bool)
    for ax in range(3):
        r2, i2 = np.roll(re, 1, ax), np.roll(im, 1, ax)
        bad |= (re * i2 - im * r2 == 0) & (re * r2 + im * i2 > 0) & ((re != r2) | (im != i2))
    return bad


def lattice_conditions(obj):
    """The guards every real_imag case asserts on the host before it launches; returns the figures."""
    o64 = obj.astype(np.float64)
    re, im = o64[..., 0], o64[..., 1]
    u = re * re + im * im
    u32 = obj[..., 0] * obj[..., 0] + obj[..., 1] * obj[..., 1]
    assert u32.dtype == np.float32 and (u32.astype(np.float64) == u).all(), 'u = re^2 + im^2 is not exact in float32'
    om = np.sqrt(u)
    dev = np.abs(om - om.mean())
    ph = np.arctan2(im, re)
    dph = np.concatenate([np.abs(np.roll(ph, 1, ax) - ph).reshape(-1) for ax in range(3)])
    fig = dict(min_dev=float(dev.min()),
               min_dph=float(dph[dph > 0].min()) if (dph > 0).any() else np.inf,
               min_ph=float(np.abs(ph)[ph != 0].min()) if (ph != 0).any() else np.inf,
               tv_ties=int(sum((np.roll(u, 1, ax) == u).sum() for ax in range(3))))
    assert obj.size == 2 or fig['min_dev'] >= 1e-5, fig          # (one voxel: dev = 0 exactly in both precisions, sgn(0) = 0)
    assert fig['min_dph'] >= 1e-5 and fig['min_ph'] >= 1e-3, fig
    lat = np.round(o64 * 64).astype(np.int64)
    fig['phase_ties_apart'] = int(phase_ties_apart(lat[..., 0], lat[..., 1]).sum())
    return fig


def ri_reference(obj, alphas, dtype):
    """(gradient, value) of alpha_d, alpha_b L1 + gamma TV on a real_imag object, the oracle in `dtype`."""
    o = obj.astype(dtype)
    ad, ab, gm = alphas
    v1, g1 = O.l1_value_grad_ri(o, ad, ab)
    v2, g2 = O.tv_value_grad_ri(o, gm) if gm else (0., np.zeros_like(o))
    g = g1 + g2
    assert g.dtype == np.dtype(dtype)
    return g, float(v1) + float(v2)


def rwl1_weight_reference(obj, dtype):
    return O.reweighted_l1_weight(obj.astype(dtype))


def rwl1_reference(obj, weight, unknown_type, dtype):
    fn = O.reweighted_l1_value_grad_ri if unknown_type == 'real_imag' else O.reweighted_l1_value_grad
    val, g = fn(obj.astype(dtype), weight.astype(dtype), *RWL1_ALPHAS)
    assert g.dtype == np.dtype(dtype)
    return g, float(val)


def grad_bar(floor, e32):
    """The project's 3x rule: three times the float32 oracle's own error, with a floor."""
    return max(floor, 3 * e32)


# ---- which test holds which kernel and entry point (tests/test_elementwise_coverage.py compares the keys with the sources) ------
M, E = 'test_gpu_elementwise_matrix', 'test_gpu_elementwise'
KERNELS = {
    'center_rows_kernel': [(E, 'test_center_rows_is_the_mirrored_sum')],
    'adam_kernel': [(M, 'test_optimiser_step')],
    'gd_kernel': [(M, 'test_optimiser_step')],
    'momentum_kernel': [(M, 'test_optimiser_step')],
    'small_adam_kernel': [(M, 'test_small_adam_with_the_most_arrays_of_one_call')],
    'axpy_kernel': [(M, 'test_axpy')],
    'reg_grad_kernel': [(M, 'test_delta_beta_launch_shapes')],
    'reg_value_reduce_kernel': [(M, 'test_delta_beta_launch_shapes')],
    'reg_grad_range_kernel': [(M, 'test_delta_beta_range_in_the_second_trip')],
    'ri_stats_kernel': [(M, 'test_real_imag_vs_fp64'), (M, 'test_reweighted_l1_gradient_vs_fp64')],
    'reg_grad_ri_kernel': [(M, 'test_real_imag_vs_fp64')],
    'reg_grad_ri_weighted_kernel': [(M, 'test_reweighted_l1_gradient_vs_fp64')],
    'reg_grad_weighted_kernel': [(M, 'test_reweighted_l1_gradient_vs_fp64')],
    'reg_value_add_kernel': [(M, 'test_reweighted_l1_gradient_vs_fp64')],
    'rwl1_partial_kernel': [(M, 'test_reweighted_l1_weights_vs_fp64')],
    'rwl1_final_kernel': [(M, 'test_reweighted_l1_weights_vs_fp64')],
    'rwl1_weight_kernel': [(M, 'test_reweighted_l1_weights_vs_fp64')],
}
ENTRY_POINTS = {
    'adm_center_rows': [(E, 'test_center_rows_is_the_mirrored_sum')],
    'adm_adam_step': [(M, 'test_optimiser_step')],
    'adm_gd_step': [(M, 'test_optimiser_step')],
    'adm_momentum_step': [(M, 'test_optimiser_step')],
    'adm_adam_step_small': [(M, 'test_small_adam_with_the_most_arrays_of_one_call'), (M, 'test_small_adam_refusals')],
    'adm_axpy': [(M, 'test_axpy')],
    'adm_reg_grad': [(M, 'test_delta_beta_launch_shapes'), (M, 'test_real_imag_vs_fp64')],
    'adm_reg_grad_set': [(M, 'test_delta_beta_launch_shapes'), (M, 'test_real_imag_vs_fp64')],
    'adm_reg_grad_range': [(M, 'test_delta_beta_range_in_the_second_trip')],
    'adm_rwl1_update': [(M, 'test_reweighted_l1_weights_vs_fp64')],
    'adm_reg_grad_weighted': [(M, 'test_reweighted_l1_gradient_vs_fp64')],
}
