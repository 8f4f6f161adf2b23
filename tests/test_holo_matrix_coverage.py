"""The holography matrix (tests/test_gpu_holo_matrix.py) covers what adm_holo.hip compiles and launches: tests/holo_matrix.py
mirrors its launch arithmetic, and this CPU test parses the source -- ADM_LINE_SIZES, the LineGeo expressions, TwLds::USE and
blocks_for in adm_line_fft.h, line_side_ok and its bounds in adm_line_host.h, the n_dists limit, every __global__ kernel and the
switch over nx or ny that instantiates it in adm_holo.hip -- so that a new size, a new kernel or a deleted field fails here until
the tables follow.  It also checks the delta/beta wrapper of the oracle against
finite differences and, for every field, what the oracle pair alone decides: the ill-conditioning guard and the 5 % cap on
bands without signal."""
import os
import re

import numpy as np
import pytest

from tests import holo_matrix as HM

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def source(name='adm_holo.hip'):
    with open(os.path.join(ROOT, 'adorym_amd', 'csrc', name)) as f:
        return f.read()


def c_to_py(e):
    """A C expression of names, integer literals, comparisons, / and (nested) ?: as a Python expression."""
    e = e.strip()
    depth = 0
    for i, ch in enumerate(e):
        depth += (ch == '(') - (ch == ')')
        if ch == '?' and depth == 0:
            d2 = 0
            for j in range(i + 1, len(e)):
                d2 += (e[j] == '(') - (e[j] == ')')
                if e[j] == ':' and d2 == 0:
                    return '((%s) if (%s) else (%s))' % (c_to_py(e[i + 1:j]), c_to_py(e[:i]), c_to_py(e[j + 1:]))
            raise AssertionError(e)
    out, i = '', 0
    while i < len(e):
        if e[i] == '(':
            d, j = 1, i + 1
            while d:
                d += (e[j] == '(') - (e[j] == ')')
                j += 1
            out += '(' + c_to_py(e[i + 1:j - 1]) + ')'
            i = j
        else:
            out += e[i]
            i += 1
    return out


def c_expr(expr, env):
    return eval(c_to_py(expr).replace('/', '//'), {'__builtins__': {}}, dict(env))


def sizes():
    m = re.search(r'#define\s+ADM_LINE_SIZES\(X\)((?:\s*X\(\d+\))+)', source('adm_line_fft.h'))
    assert m, 'ADM_LINE_SIZES'
    return tuple(int(v) for v in re.findall(r'X\((\d+)\)', m.group(1)))


def test_the_mirror_uses_the_sizes_and_limits_of_the_source():
    src, host = source(), source('adm_line_host.h')
    assert sizes() == HM.SIZES
    m = re.search(r'constexpr int ADM_LINE_MIN_SIDE = (\d+), ADM_LINE_MAX_SIDE = (\d+);', host)
    assert m and (int(m.group(1)), int(m.group(2))) == (HM.MIN_SIDE, HM.MAX_SIDE)
    assert 'inline bool line_side_ok(int n) { return n >= ADM_LINE_MIN_SIDE && n <= ADM_LINE_MAX_SIDE && (n & (n - 1)) == 0; }' in host
    assert 'if (!line_side_ok(d.ny) || !line_side_ok(d.nx))' in src
    assert HM.SIZES == tuple(n for n in range(1, 5000) if HM.pow2_in_range(n))          # every accepted side has its instantiation
    m = re.search(r'if \(d\.n_dists < 1 \|\| d\.n_dists > (\d+)\)', src)
    assert m and int(m.group(1)) == HM.MAX_DISTS
    assert set(re.findall(r'__launch_bounds__\((\d+)\)', src)) == {str(HM.THREADS), '64'}
    assert set(re.findall(r'dim3\((\d+)\)', src)) == {str(HM.THREADS), '64'}


def test_the_mirror_follows_linegeo_and_twlds():
    src, hdr = source(), source('adm_line_fft.h')
    geo = re.search(r'template <int N> struct LineGeo \{(.*?)\n\};', hdr, re.S).group(1)
    ex = {n: re.search(r'static constexpr int %s = ([^;]+);' % n, geo).group(1) for n in ('TPR', 'LPB', 'LP')}
    use = re.search(r'template <int N> struct TwLds \{\s*static constexpr bool USE = ([^;]+);', hdr).group(1)
    for n in HM.SIZES:
        env = dict(N=n)
        for k in ('TPR', 'LPB', 'LP'):
            env[k] = int(c_expr(ex[k], env))
        g = HM.line_geo(n)
        assert (g['TPR'], g['LPB'], g['LP']) == (env['TPR'], env['LPB'], env['LP']), (n, g, env)
        assert g['tw_lds'] == bool(c_expr(use, env)), n
        assert g['TPR'] * g['LPB'] == HM.THREADS
    assert [HM.line_geo(n)['LPB'] for n in HM.SIZES] == [128, 64, 32, 16, 8, 4, 2, 1]
    assert [HM.line_geo(n)['LP'] - n for n in HM.SIZES] == [1, 1, 1, 2, 4, 8, 16, 0]
    # blocks_for, K3's jobs, K4's one block per line and its rounds
    assert 'static int blocks_for(int lines) { return (lines + LineGeo<N>::LPB - 1) / LineGeo<N>::LPB; }' in hdr
    assert 'const int job0 = blockIdx.x * LG::LPB, job = job0 + ll;' in src and 'const int d = ok ? job / A.ny : 0, y = ok ? job % A.ny : 0;' in src
    assert 'for (int d0 = 0; d0 < A.nd; d0 += LG::LPB) {' in src and 'const int kx = blockIdx.x;' in src
    g = HM.geometry(64, 16, 3)
    assert g['k3_blocks'] == [(0, 128), (128, 192)] and g['k3_spans'] == [True, False] and g['row_blocks'] == [(0, 64)]
    g = HM.geometry(512, 64, 5)
    assert (g['k4_rounds'], g['k4_ragged'], len(g['col_blocks']), len(g['row_blocks'])) == (2, True, 16, 16)
    g = HM.geometry(256, 16, 64)
    assert (g['k4_rounds'], g['k4_ragged'], g['n_sums'], len(g['row_blocks'])) == (8, False, 512, 2)
    g = HM.geometry(2048, 16, 3)
    assert (g['k4_rounds'], g['k4_ragged'], len(g['col_blocks'])) == (3, False, 16)


def kernels_of(src):
    """{family: number of template parameters} of every __global__ of the source, the bool / int parameters spelled out."""
    found = {}
    for m in re.finditer(r'(?:template <([^>]*)>\s*)?__global__\s+__launch_bounds__\(\d+\)\s+void\s+(\w+)\s*\(', src):
        params, name = m.group(1), m.group(2)
        if not params:
            found[name] = None
            continue
        params = [p.strip() for p in params.split(',')]
        assert params[0].startswith('int N'), (name, params)
        if len(params) == 1:
            found[name + '<N>'] = params
        else:
            assert len(params) == 2, (name, params)
            values = ('true', 'false') if params[1].startswith('bool') else ('0', '1')
            for v in values:
                found['%s<N, %s>' % (name, v)] = params
    return found


def launched_by(src):
    """{family: 'nx' | 'ny'}: which length instantiates a kernel, from the X-macros and the switches of holo_run and launch_*."""
    macros, out = {}, {}
    modes = sorted(set(re.findall(r'launch_slf<(\d)>\(', src)))
    text = src.replace('\\\n', ' ')
    for m in re.finditer(r'#define (\w+)\(N_\) (.*)|switch \([AS]\.(nx|ny)\) \{ ADM_LINE_SIZES\((\w+)\)', text):
        if m.group(1):
            body = m.group(2)
            ks = re.findall(r'\(\((holo_\w+)<N_(?:, (\w+))?>\)', body) + [(k, '') for k in re.findall(r'K_X\((holo_\w+), N_', body)]
            assert ks, body
            macros[m.group(1)] = ks
            continue
        axis, macro = m.group(3), m.group(4)
        for name, arg in macros[macro]:
            for a in (modes if arg == 'MODE' else [arg]):
                fam = '%s<N%s>' % (name, ', ' + a if a else '')
                assert out.setdefault(fam, axis) == axis, fam
    return out


def test_the_matrix_names_exactly_the_kernels_of_the_source():
    src = source()
    found = kernels_of(src)
    assert len(re.findall(r'__global__', src)) == 11 and len(found) == 14, sorted(found)
    assert set(found) == set(HM.KERNELS), set(found) ^ set(HM.KERNELS)
    axes = launched_by(src)
    assert set(axes) == {k for k in HM.KERNELS if '<' in k}, set(axes) ^ set(HM.KERNELS)
    for k, (axis, fields, tests) in HM.KERNELS.items():
        assert axis == axes.get(k), (k, axis, axes.get(k))
    with open(os.path.join(ROOT, 'tests', 'test_gpu_holo_matrix.py')) as f:
        text = f.read()
    for k, (_, _, tests) in HM.KERNELS.items():
        assert tests, k
        for t in tests:
            assert re.search(r'^def %s\(' % t, text, re.M), (k, t)
    # the two fixed kernels are launched where the table says
    assert 'hipLaunchKernelGGL(holo_sums_kernel, dim3(A.nd * 8), dim3(64), 0, st, A);' in src
    assert 'hipLaunchKernelGGL(holo_shift_sum_kernel, dim3(S.nd * 2), dim3(64), 0, h->ctx->stream, S);' in src


def test_every_instantiation_is_reached():
    want = {(k, n if '<' in k else 0) for k in HM.KERNELS for n in sizes()}
    missing = sorted(want - HM.reached())
    assert not missing, 'instantiations no field launches: %s' % missing
    assert len(want) == 12 * 8 + 2
    assert len(HM.BIG8) == 8 and all(ny * nx <= 32768 for ny, nx in HM.FIELDS)
    assert set(HM.NEW_KERNELS) == {(16, 2048), (2048, 16)} and HM.VARIANT_FIELD in HM.FIELDS and HM.VARIANT_FIELD_K4 in HM.FIELDS
    assert {nx for _, nx in HM.SPECTRUM_FIELDS} == {16, 32, 64} and {ny for ny, _ in HM.SPECTRUM_FIELDS} >= {16, 2048}
    assert all(1 <= nd <= HM.MAX_DISTS for nd in HM.FIELDS.values())


def test_every_class_is_reached():
    got = {}
    for (ny, nx), nd in HM.FIELDS.items():
        for c in HM.classes(ny, nx, nd):
            got.setdefault(c, []).append((ny, nx))
    assert set(got) <= set(HM.ALL_CLASSES)
    missing = [c for c in HM.ALL_CLASSES if c not in got]
    assert not missing, 'classes no field reaches: %s' % missing
    # what each field is listed for
    assert 'partial_block' in HM.classes(16, 16, 1) and 'nd_1' in HM.classes(16, 16, 1)
    assert 'k3_block_spans_distances' in HM.classes(64, 16, 3) and 'k3_block_spans_distances' in HM.classes(32, 32, 5)
    assert HM.geometry(32, 32, 5)['k3_blocks'][-1] == (128, 160)
    assert 'k4_ragged_last_round' in HM.classes(512, 64, 5) and 'nd_64' in HM.classes(256, 16, 64)
    assert {'k4_several_rounds', 'twiddles_global', 'tpr_gt_64'} <= HM.classes(2048, 16, 3) and 'k4_ragged_last_round' not in HM.classes(2048, 16, 3)
    assert {'twiddles_global', 'k4_one_round'} <= HM.classes(16, 2048, 3)


def test_variants_name_every_argument_value():
    v = HM.VARIANTS
    assert {'delta_beta', 'sigma_minus', 'magnitude', 'delta_beta_sigma_minus', 'plane_probe', 'no_affine', 'grad_affine_without_affine',
            'clamped_translation', 'grad_dists_only', 'grad_affine_only', 'no_small_gradients', 'no_grad_probe', 'no_pred', 'forward_only',
            'accumulate', 'overwrite_sentinel'} <= set(v)
    for name, (ckw, lkw, k4) in v.items():
        c = HM.inputs(16, 16, 2, **ckw)
        assert set(lkw) <= {'want', 'want_pred', 'want_grad', 'seed', 'overwrite'}, name
    assert [n for n, x in v.items() if x[2]] == [n for n, _ in [c for c in HM.VARIANT_CASES if c[1] == HM.VARIANT_FIELD_K4]]
    c = HM.inputs(128, 256, 3, affine='clamp')
    cx, cy = HM.clamped_samples(c)
    assert cx > 0.05 * c['data'].size and cy > 0.05 * c['data'].size, (cx, cy)
    assert HM.clamped_samples(HM.inputs(128, 256, 3)) < (0.02 * c['data'].size,) * 2
    assert not HM.inputs(16, 16, 1, affine='none')['has_affine'] and np.iscomplexobj(HM.inputs(16, 16, 1)['probe'])
    assert np.abs(HM.inputs(16, 16, 1)['probe'].imag).max() > 0.01 and not HM.inputs(16, 16, 1, probe='plane')['probe'].imag.any()


@pytest.mark.parametrize('sigma', [1, -1])
def test_delta_beta_wrapper_against_finite_differences(sigma):
    """dL/d(delta) and dL/d(beta) of oracle_run at 16 x 16 against central differences of the wrapped fp64 loss, to 1e-6."""
    c = HM.inputs(16, 16, 2, unknown_type='delta_beta', sigma=sigma)
    c['obj'] = c['obj'].astype(np.float64)
    g = HM.oracle_run(c, 'float64')['g_obj']
    k1 = float(HM.k1_of())
    assert abs(k1 - 8.64e4) < 1e2 and np.abs(k1 * c['obj'][..., 0]).max() < 1 and np.abs(k1 * c['obj'][..., 0]).max() > 0.05
    for (y, x, ch) in ((0, 0, 0), (3, 11, 0), (15, 15, 1), (8, 2, 1), (5, 5, 0), (12, 7, 1)):
        h = 1e-9 if ch == 0 else 1e-9
        p, m = c['obj'].copy(), c['obj'].copy()
        p[y, x, 0, ch] += h
        m[y, x, 0, ch] -= h
        fd = (HM.wrapped_loss(c, p) - HM.wrapped_loss(c, m)) / (2 * h)
        assert abs(fd - g[y, x, 0, ch]) <= 1e-6 * abs(g[y, x, 0, ch]), ((y, x, ch), fd, g[y, x, 0, ch])
    # the float32 yardstick is the same computation: within float32 of it
    g32 = HM.oracle_run(dict(c, obj=c['obj'].astype(np.float32)), 'float32')['g_obj']
    assert g32.dtype == np.float32 and HM.rel(g32, g) < 1e-5


def _all_cases():
    for (ny, nx), nd in HM.FIELDS.items():
        yield (ny, nx, nd, ()), False
        if (ny, nx) in HM.SPECTRUM_FIELDS:
            yield (ny, nx, nd, (('broadband', True), ('probe', 'plane'))), True
        if (ny, nx) in HM.SHIFT_FIELDS:
            yield (ny, nx, nd, (('shifts', True),)), False
    for name, field in HM.VARIANT_CASES:
        ckw = HM.VARIANTS[name][0]
        if ckw:
            yield field + (HM.FIELDS[field], tuple(sorted(ckw.items()))), False


@pytest.mark.parametrize('key,spectral', sorted(set(_all_cases())), ids=lambda v: '-'.join(str(x) for x in v[:3]) + ''.join('-%s=%s' % kv for kv in v[3])
                         if isinstance(v, tuple) else ('spectral' if v else 'rows'))
def test_the_oracle_pair_satisfies_the_guard_and_the_band_cap(key, spectral):
    """For every case of the GPU module: the fp32 oracle is within a third of the bar (prediction, object and probe gradient),
    and at most 5 % of the bands of any judged array lack signal."""
    ny, nx, nd, kw = key
    print(HM.oracle_conditions(HM.case(ny, nx, nd, **dict(kw)), spectral=spectral))
