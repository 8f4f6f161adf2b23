"""The element-wise matrix (tests/test_gpu_elementwise_matrix.py, tables in tests/ew_matrix.py) covers what adm_optimize.hip and
adm_regularize.hip compile and launch.  This CPU test parses the two files, adm_optim.h, adm_host.h and include/adm.h: every
__global__ kernel and extern "C" entry point must have a row in the tables, and every constant that decides a launch geometry --
stream_grid's 4096, the nb > 1024 caps, reg_threads' 96 / 192, reg_value_reduce_kernel's 1024, SMALL_WHOLE_RPT, small_chunk's
4096 / 256 / 2048, ADM_SMALL_PARAMS_MAX, the three flag values -- must equal the table's copy, and the cases must lie on both
sides of it.  It also runs on the host what the GPU module relies on: the float32 mirrors against the oracle's fp64, the equality
of adam_scalars' q1 / q2 with the oracle's, and the guards of the lattice objects."""
import os
import re

import numpy as np
import pytest

from oracle import adorym_oracle as O
from tests import ew_matrix as EM
from tests import test_gpu_elementwise as E

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def read(*parts):
    with open(os.path.join(ROOT, *parts)) as f:
        return f.read()


def sources():
    return read('adorym_amd', 'csrc', 'adm_optimize.hip'), read('adorym_amd', 'csrc', 'adm_regularize.hip')


def one(pattern, text, what):
    m = re.findall(pattern, text)
    assert len(m) >= 1, what
    return m


# ---- every kernel and entry point has a row -------------------------------------------------------------------------------------
def test_the_tables_name_exactly_the_kernels_and_entry_points_of_the_sources():
    opt, reg = sources()
    kernels, entries = set(), set()
    for src in (opt, reg):
        found = re.findall(r'__global__\s+(?:__launch_bounds__\(\d+\)\s+)?void\s+(\w+)\s*\(', src)
        assert len(found) == len(re.findall(r'__global__', src)), 'a __global__ the parser does not read'
        kernels |= set(found)
        entries |= set(re.findall(r'extern "C" int (\w+)\(', src))
        assert len(re.findall(r'extern "C"', src)) == len(re.findall(r'extern "C" int (\w+)\(', src))
    assert kernels == set(EM.KERNELS), kernels ^ set(EM.KERNELS)
    assert entries == set(EM.ENTRY_POINTS), entries ^ set(EM.ENTRY_POINTS)
    header = read('include', 'adm.h')
    for name in entries:
        assert re.search(r'\b%s\(' % name, header), name
    text = {m: read('tests', m + '.py') for m in (EM.M, EM.E)}
    for name, tests in list(EM.KERNELS.items()) + list(EM.ENTRY_POINTS.items()):
        assert tests, name
        for module, test in tests:
            assert re.search(r'^def %s\(' % test, text[module], re.M), (name, module, test)
    # an entry point's test calls it (through the library handle, or through the test it re-runs)
    for name, tests in EM.ENTRY_POINTS.items():
        assert any(('lib.%s(' % name) in text[m] or ('lib.%s,' % name) in text[m] or ('lib.%s)' % name) in text[m] for m, _ in tests), name


# ---- the constants --------------------------------------------------------------------------------------------------------------
def test_flags_and_the_small_parameter_limit():
    header = read('include', 'adm.h')
    flags = {k: int(v) for k, v in re.findall(r'#define ADM_FLAG_(\w+) (\d+)', header)}
    assert flags == dict(NONNEG=EM.NONNEG, ZERO_CH0=EM.ZERO_CH0, ZERO_CH1=EM.ZERO_CH1), flags
    optim = read('adorym_amd', 'csrc', 'adm_optim.h')
    assert '(flags & ADM_FLAG_ZERO_CH0) && !(i & 1)' in optim and '(flags & ADM_FLAG_ZERO_CH1) && (i & 1)' in optim and 'mask[i >> 1]' in optim
    for opt in EM.OPTIMISERS:                              # all 8 combinations, with and without a mask, for every optimiser
        assert {(c[4], c[5]) for c in EM.FLAG_CASES if c[0] == opt} == {(f, m) for f in range(8) for m in (False, True)}
    assert int(one(r'#define ADM_SMALL_PARAMS_MAX (\d+)', header, 'ADM_SMALL_PARAMS_MAX')[0]) == EM.SMALL_PARAMS_MAX
    from adorym_amd import _lib
    assert _lib.SMALL_PARAMS_MAX == EM.SMALL_PARAMS_MAX and (_lib.FLAG_NONNEG, _lib.FLAG_ZERO_CH0, _lib.FLAG_ZERO_CH1) == (1, 2, 4)
    assert len(EM.SMALL_ARRAYS) == EM.SMALL_PARAMS_MAX and all(len(c) == EM.SMALL_PARAMS_MAX for c in EM.SMALL_CALLS.values())
    assert 'refused(EM.SMALL_PARAMS_MAX + 1' in read('tests', EM.M + '.py')


def test_stream_grid_and_the_block_caps_have_cases_on_both_sides():
    host = read('adorym_amd', 'csrc', 'adm_host.h')
    m = re.search(r'inline int stream_grid\(size_t n\) \{[^\n]*\n\s*size_t b = \(n \+ (\d+)\) / (\d+);\s*return \(int\)\(b > (\d+) \? (\d+) : \(b \? b : 1\)\);', host)
    assert m, 'stream_grid'
    assert (int(m.group(1)) + 1, int(m.group(2)), int(m.group(3)), int(m.group(4))) == (EM.THREADS, EM.THREADS, EM.STREAM_BLOCKS, EM.STREAM_BLOCKS)
    for n in (0, 1, 256, 257, EM.STREAM_CAP, EM.STREAM_CAP + 1):
        b = (n + 255) // 256
        assert EM.stream_grid(n) == (4096 if b > 4096 else (b if b else 1))
    opt, reg = sources()
    assert len(re.findall(r'dim3\(stream_grid\(', opt)) == 4 and 'dim3(256)' in opt
    cap = EM.STREAM_CAP
    for o in EM.OPTIMISERS:                                # the grid-stride loops of adam / gd / momentum: one trip and two
        lens = [hi - lo for c, n, lo, hi, *_ in EM.RANGE_CASES if c == o]
        assert min(l for l in lens if l > 0) == 1 and max(lens) > cap and any(0 < l <= cap for l in lens), o
        assert {255, 256, 257} <= set(lens) and 0 in lens and any(l < 0 for l in lens)
        ends = {(lo & 1, hi & 1) for c, n, lo, hi, *_ in EM.RANGE_CASES if c == o and hi > lo}
        assert ends == {(1, 1), (1, 0), (0, 1)} or ends > {(1, 1), (1, 0), (0, 1)}, ends
    for a in (1.0, -0.375):
        ns = [n for aa, n in EM.AXPY_CASES if aa == a]
        assert min(ns) == 1 and max(ns) > cap and any(EM.THREADS < n <= cap for n in ns)
    # the nb > 1024 caps of ri_stats_launch and adm_rwl1_update
    caps = [int(v) for v in re.findall(r'if \(nb > (\d+)\) nb = (?:\d+);', reg)]
    assert caps == [EM.BLOCK_CAP, EM.BLOCK_CAP] and re.findall(r'if \(nb > \d+\) nb = (\d+);', reg) == [str(EM.BLOCK_CAP)] * 2
    block_cap = EM.BLOCK_CAP * EM.THREADS
    V = [int(np.prod(s)) for s, _ in EM.RI_CASES]
    assert min(V) == 1 and any(EM.THREADS < v <= block_cap for v in V) and any(block_cap < v <= cap for v in V) and any(v > cap for v in V)
    assert 256 in V and 257 in V                           # one and two workgroups
    for ax in range(3):                                    # each axis at extent 1, and the extent-2 wrap
        assert any(s[ax] == 1 and min(s[(ax + 1) % 3], s[(ax + 2) % 3]) > 1 for s in EM.RI_SHAPES), ax
    assert (2, 2, 2) in EM.RI_SHAPES
    assert [a for s, a in EM.RI_CASES if s == EM.RI_BIG] == [EM.RI_ALPHAS[2]] and all(EM.RI_ALPHAS[2])
    assert {a for s, a in EM.RI_CASES if s != EM.RI_BIG} == set(EM.RI_ALPHAS)
    n = [2 * int(np.prod(s)) for s in EM.RWL1_SHAPES]      # adm_rwl1_update runs over both channels
    assert any(v <= block_cap for v in n) and any(block_cap < v <= cap for v in n) and any(v > cap for v in n)
    assert any(int(np.prod(s)) > cap for s in EM.RWL1_SHAPES)          # reg_grad_ri_weighted_kernel's second trip (V voxels)


def test_reg_threads_and_the_value_reduction_have_cases_on_both_sides():
    _, reg = sources()
    m = re.search(r'static inline int reg_threads\(int obj_z\) \{ return obj_z >= (\d+) \? (\d+) : \(obj_z >= (\d+) \? (\d+) : (\d+)\); \}', reg)
    assert m, 'reg_threads'
    assert (int(m.group(3)), int(m.group(1))) == EM.REG_THREADS and (int(m.group(2)), int(m.group(4)), int(m.group(5))) == (256, 128, 64)
    Z = {s[2] for s in EM.DB_SHAPES} | {s[2] for s in E.SHAPES}
    for t in EM.REG_THREADS:
        assert t in Z and t - 1 in Z, t
    top = EM.reg_threads(10 ** 6)
    assert any(top < z < 2 * top for z in Z)               # a partial second trip of the z loop
    assert EM.DB_RANGE_SHAPE[2] > top and EM.DB_RANGE_SHAPE in EM.DB_SHAPES
    m = re.search(r'__launch_bounds__\((\d+)\) void reg_value_reduce_kernel.*?i < n; i \+= (\d+)\)', reg, re.S)
    assert m and int(m.group(1)) == int(m.group(2)) == EM.REDUCE_THREADS
    assert 'dim3(1), dim3(%d), 0, st, (const float*)partial' % EM.REDUCE_THREADS in reg
    rows = [s[0] * s[1] for s in EM.DB_SHAPES + E.SHAPES]
    assert any(r > EM.REDUCE_THREADS for r in rows) and any(1 < r <= EM.REDUCE_THREADS for r in rows)
    assert set(EM.DB_ALPHAS) == {(.7, .3, 0.), (0., 0., .5), (.7, .3, .5)}


def test_the_small_parameter_launch_has_cases_on_both_sides():
    opt, _ = sources()
    m = re.search(r'static inline int small_chunk\(uint64_t n\) \{ return n > (\d+) \? (\d+) : (\d+); \}', opt)
    assert m and tuple(int(v) for v in m.groups()) == EM.SMALL_CHUNK
    assert int(one(r'#define SMALL_WHOLE_RPT (\d+)', opt, 'SMALL_WHOLE_RPT')[0]) == EM.SMALL_WHOLE_RPT
    assert 'q.center_cols <= 2 && q.n / (size_t)q.center_cols <= (size_t)256 * SMALL_WHOLE_RPT' in opt
    limit, few, many = EM.SMALL_CHUNK
    ew = [s for s in EM.SMALL_ARRAYS if not s['center_cols']]
    assert any(s['n'] == 1 for s in ew)
    assert any(many < s['n'] <= limit and EM.small_blocks(s) == 2 for s in ew)                       # two chunks of 2048
    assert any(s['n'] > limit and EM.small_blocks(s) == -(-s['n'] // few) > 2 for s in ew)           # chunks of 256
    assert any(s['n'] > limit and few < s['pin_n'] < s['n'] and s['pin_n'] % few for s in ew)        # a pin across a chunk boundary
    whole = [s for s in EM.SMALL_ARRAYS if s['center_cols']]
    assert all(s['pin_n'] and s['n'] % s['center_cols'] == 0 for s in whole)
    assert any(EM.small_register_resident(s) and s['n'] // s['center_cols'] == EM.THREADS * EM.SMALL_WHOLE_RPT for s in whole)
    assert any(not EM.small_register_resident(s) and s['center_cols'] == 3 for s in whole)
    assert sum(isinstance(k, dict) and k['n'] == 0 for k in EM.SMALL_CALLS['zero_length'][1:-1]) == 1
    assert EM.SMALL_CALLS['reversed'] == EM.SMALL_CALLS['forward'][::-1]
    assert len({s['step'] for s in EM.SMALL_ARRAYS}) == len(EM.SMALL_ARRAYS)


# ---- the mirrors on the host ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('i_batch', EM.I_BATCHES)
def test_adam_scalars_and_the_float32_oracle_are_the_spelled_out_mirror(i_batch):
    h = EM.HYPER
    q1, q2 = EM.adam_scalars(i_batch, h['b1'], h['b2'])
    assert q1 == np.float32(1 - h['b1'] ** (i_batch + 1)) and q2 == np.float32(1 - h['b2'] ** (i_batch + 1))
    inp = EM.opt_inputs(200000, seed=3)
    got = O.adam_step(inp['x'], inp['g'], inp['m'], inp['v'], i_batch, h['step'], h['b1'], h['b2'], h['eps'])
    want = EM.adam_spelled_out(inp['x'], inp['g'], inp['m'], inp['v'], i_batch, h['step'], h['b1'], h['b2'], h['eps'])
    for a, b in zip(got, want):
        assert a.dtype == np.float32 and (EM.bits(a) == EM.bits(b)).all()
    x64 = O.adam_step(*[inp[k].astype(np.float64) for k in ('x', 'g', 'm', 'v')], i_batch, h['step'], h['b1'], h['b2'], h['eps'])[0]
    e = EM.rel(got[0], x64)
    print('i_batch %d: float32 vs fp64 %.3e' % (i_batch, e))
    assert e < 2e-7


@pytest.mark.parametrize('case', [c for c in EM.OPT_CASES if c[1] != EM.BIG] + [c for c in EM.RANGE_CASES if c[1] == EM.BIG][:1], ids=EM.case_id)
def test_the_float32_mirror_is_within_the_bar_of_fp64(case):
    opt, n, lo, hi, flags, with_mask, i_batch = case
    inp = EM.opt_inputs(n)
    mirror = EM.step_reference(opt, inp, lo, hi, flags, with_mask, i_batch, np.float32)
    ref = EM.step_reference(opt, inp, lo, hi, flags, with_mask, i_batch, np.float64)
    for k in mirror:
        assert mirror[k].dtype == np.float32 and EM.rel(mirror[k], ref[k]) < 2e-6 / 3, k
    e = np.arange(n)
    inside = (e >= lo) & (e < hi)
    for k in mirror:
        assert (EM.bits(mirror[k])[~inside] == EM.bits(inp[k])[~inside]).all()
    if not inside.any():
        return
    x = mirror['x']
    kept = EM.constrain_mirror(inp['x'], flags, inp['mask'] if with_mask else None)
    still = [i for i in inp['still'] if inside[i]]
    assert (EM.bits(x)[still] == EM.bits(kept)[still]).all()
    if hi - lo > 64:
        neg = np.array([i for i in inp['negative'] if inside[i]], int)
        assert len(still) and len(neg) and (inp['x'][neg] < 0).all()
    if hi - lo == n:                                       # the planted elements meet both signed zeros
        zero_ch = [i for i in range(n) if (flags & EM.ZERO_CH0 and not i & 1) or (flags & EM.ZERO_CH1 and i & 1)]
        if zero_ch and not flags & EM.NONNEG:
            assert (EM.bits(x)[zero_ch] == 0x80000000).any() and not x[zero_ch].any()
        if flags & EM.NONNEG:
            assert (x >= 0).all() and (EM.bits(x) == 0).any()
        if with_mask:
            off = np.repeat(inp['mask'], 2)[:n] == 0
            assert off.any() and not x[off].any() and (~off).any()


def test_small_mirror_pins_after_the_recentring():
    for k, spec in enumerate(EM.SMALL_ARRAYS):
        inp = EM.small_inputs(k, spec)
        w = EM.small_mirror(spec, inp, 1)
        assert not w['g'].any() and (EM.bits(w['x'][:spec['pin_n']]) == EM.bits(inp['pin'][:spec['pin_n']])).all()
        if spec['center_cols']:
            cols = w['x'].reshape(-1, spec['center_cols'])[-(-spec['pin_n'] // spec['center_cols']):]
            full = EM.small_mirror(dict(spec, pin_n=0), inp, 1)['x'].reshape(-1, spec['center_cols'])
            assert np.abs(full.mean(0)).max() < 1e-6 * np.abs(full).max() and (EM.bits(cols) == EM.bits(full[-len(cols):])).all()


# ---- the lattice objects --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('shape', EM.RI_SHAPES + [(3, 4, 5)], ids=EM.case_id)
def test_lattice_guards_and_the_float32_oracle(shape):
    obj = EM.lattice_object(shape)
    assert obj.dtype == np.float32 and ((obj * 64) == np.round(obj * 64)).all()
    assert (obj.astype(np.float64) ** 2).sum(-1).min() >= 0.25
    fig = EM.lattice_conditions(obj)
    assert fig['phase_ties_apart'] == 0
    V = int(np.prod(shape))
    if V > 1:
        assert fig['tv_ties'] >= 3                         # the planted copies: sgn(0) = 0 is exercised
    for alphas in EM.RI_ALPHAS:
        g64, v64 = EM.ri_reference(obj, alphas, np.float64)
        g32, v32 = EM.ri_reference(obj, alphas, np.float32)
        if np.abs(g64).max() == 0:
            assert not g32.any()
            continue
        e32 = EM.rel(g32, g64)
        print(shape, alphas, 'float32 oracle: %.3e' % e32, fig)
        assert e32 < 1e-6 / 3 and abs(v32 - v64) <= 1e-6 * abs(v64)
        assert (np.sign(g32) == np.sign(g64)).all() or e32 < 1e-6 / 3


@pytest.mark.parametrize('shape', EM.RWL1_SHAPES[:-1], ids=EM.case_id)
def test_reweighted_lattice_guards_and_the_float32_oracle(shape):
    obj = EM.lattice_object(shape, reweighted=True)
    assert np.abs(obj).min() >= 1 / 64 and obj[..., 0].min() >= 0.25 and obj.mean() > 0
    EM.lattice_conditions(obj)
    w64 = EM.rwl1_weight_reference(obj, np.float64)
    assert w64.max() / w64.min() < 2 ** 8.5 and w64.min() > 0
    assert EM.rel(EM.rwl1_weight_reference(obj, np.float32), w64) < 2e-6 / 3
    w = w64.astype(np.float32)
    for ut in EM.UNKNOWN_TYPES:
        g64, v64 = EM.rwl1_reference(obj, w, ut, np.float64)
        g32, v32 = EM.rwl1_reference(obj, w, ut, np.float32)
        assert EM.rel(g32, g64) < 2e-6 / 3 and abs(v32 - v64) <= 1e-6 * abs(v64), ut
