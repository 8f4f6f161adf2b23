"""The streamed-path sweep (tests/test_gpu_streamed_matrix.py) covers what adm_ms_streamed.hip launches: tests/st_matrix.py
mirrors its launch arithmetic, and this CPU test parses the source -- the constants, st_cw, st_col_threads and the column-launch
geometry of adm_ms_col.h, the row-group rule of ms_streamed_launch, GEN_E, factor()'s radix list and the __global__ kernels -- so
that a change there fails here until the tables follow.  It also asserts that the tables reach every class of geometry they name
and that the column helpers which the translation units of the path share are defined once."""
import os
import re

import pytest

from tests import st_matrix as SM
from tests.test_kernel_matrix_coverage import _function_body

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, 'adorym_amd', 'csrc')


def _read(name):
    with open(os.path.join(CSRC, name)) as f:
        return f.read()


def constants(src, names):
    """constexpr int NAME = <integer expression of literals and earlier names>;"""
    out = {}
    for n in names:
        m = re.search(r'constexpr\s+int\s+%s\s*=\s*([^;]+);' % n, src)
        assert m, n
        out[n] = int(eval(m.group(1), {'__builtins__': {}}, dict(out)))
    return out


def c_int_function(body, consts):
    """A Python callable from the body of a small C function of one int argument ``py``: declarations, ``if (c) x = v;`` and a
    return of integer expressions (C's / on the non-negative ints here is //)."""
    body = body.strip()[1:-1]
    lines = []
    for stmt in [s.strip() for s in body.split(';') if s.strip()]:
        stmt = re.sub(r'\b(const\s+)?int\s+', '', stmt).replace('/', '//')
        m = re.match(r'if\s*\((.*)\)\s*(\w+\s*=.*)$', stmt)
        if m:
            lines.append('if %s: %s' % (m.group(1), m.group(2)))
            continue
        m = re.match(r'return\s+(.*?)\s*\?\s*(.*?)\s*:\s*(.*)$', stmt)
        if m:
            lines.append('return (%s) if (%s) else (%s)' % (m.group(2), m.group(1), m.group(3)))
            continue
        lines.append(stmt)
    code = 'def f(py):\n' + ''.join('    %s\n' % ln for ln in lines)
    env = dict(consts)
    exec(code, env)
    return env['f']


def parsed():
    st, col, gen, api = _read('adm_ms_streamed.hip'), _read('adm_ms_col.h'), _read('adm_ms_gen.h'), _read('adm_api.hip')
    c = constants(st, ['ST_ROW_NT', 'ST_ROW_E', 'ST_ROW_ELEMS', 'ST_MAX_SIDE', 'ST_MAX_SLICES'])
    c.update(constants(col, ['ST_COL_NT']))
    c.update(constants(gen, ['GEN_E']))
    cw = c_int_function(_function_body(col, r'int\s+st_cw\s*\(\s*int\s+py\s*\)'), c)
    nt = c_int_function(_function_body(col, r'inline\s+int\s+st_col_threads\s*\(\s*int\s+py\s*\)'), dict(c, st_cw=cw))
    m = re.search(r'const\s+int\s+pref\[\]\s*=\s*\{([^}]*)\}', api)
    assert m, 'pref[] of factor()'
    pref = tuple(int(v) for v in m.group(1).split(','))
    return st, api, c, cw, nt, pref


def test_the_mirror_uses_the_source_constants():
    _, api, c, _, _, pref = parsed()
    for n, v in c.items():
        assert getattr(SM, n) == v, (n, v)
    assert SM.PREF == pref, pref
    # factor(): at most 8 radices, the leftover primes from 11 in steps of 2
    body = _function_body(api, r'auto\s+factor\s*=\s*\[\]\s*\(int n, int\* r\)')
    assert set(re.findall(r'cnt\s*<\s*(\d+)', body)) == {str(SM.MAX_RADICES)}
    assert re.search(r'for\s*\(int q = 11;[^;]*;\s*q \+= 2\)', body)


def test_the_mirror_follows_st_cw_and_st_col_threads():
    _, _, _, cw, nt, _ = parsed()
    for py in (1, 2, 7, 8, 255, 256, 257, 512, 513, 640, 1000, 1024, 1025, 1031, 1536, 1792, 1793, 2047, 2048):
        assert SM.st_cw(py) == cw(py), py
        assert SM.st_col_threads(py) == nt(py), py
    for py in range(1, SM.ST_MAX_SIDE + 1):
        assert SM.st_cw(py) == cw(py) and SM.st_col_threads(py) == nt(py), py
    assert [SM.st_cw(p) for p in (512, 513, 1024, 1025, 2048)] == [8, 8, 8, 4, 4]
    assert [SM.st_col_threads(p) for p in (512, 513, 1024, 1025, 2048)] == [256, 320, 512, 320, 512]
    assert max(SM.st_col_threads(p) for p in range(1, 2049)) == SM.ST_COL_NT
    # every thread's elements fit its registers and the detector kernel's LDS the attribute of ms_streamed_launch
    for py in range(1, 2049):
        g = SM.geometry(py, 2048)
        assert g['col_ne'] <= SM.GEN_E and g['row_ne'] <= SM.ST_ROW_E and g['det_lds_bytes'] <= 160 * 1024 - 256, py


def test_the_mirror_follows_the_row_groups_of_the_launch():
    st = parsed()[0]
    body = _function_body(st, r'hipError_t\s+ms_streamed_launch\s*\(')
    assert re.search(r'int rows = ST_ROW_ELEMS / Px;\s*if \(rows < 1\) rows = 1;\s*if \(rows > Py\) rows = Py;', body)
    # the column launches: the one geometry function of adm_ms_col.h; the detector kernel's float plane on top of its LDS bytes
    assert 'const StColGeom cg = st_col_geom(Py, Px);' in body
    assert 'const int ngr = (Py + rows - 1) / rows, ncg = cg.ncg;' in body
    assert 'int ms_streamed_col_groups(int py, int px) { return st_col_geom(py, px).ncg; }' in st
    assert re.search(r'StColGeom dg = cg;\s*dg\.lds \+= \(size_t\)Py \* cg\.cw \* sizeof\(float\);', body)
    assert 'st_col_launch(st_det_kernel, dg, batch, st, p, fld, part);' in body
    # ... and the one launch line: groups * cg.ncg workgroups of cg.threads threads with cg.lds bytes
    launch = _function_body(_read('adm_ms_col.h'), r'inline\s+hipError_t\s+st_col_launch\s*\(')
    assert 'hipLaunchKernelGGL(kernel, dim3((unsigned)(groups * cg.ncg)), dim3((unsigned)cg.threads), cg.lds, st, args...);' in launch
    geom = _function_body(_read('adm_ms_col.h'), r'inline\s+StColGeom\s+st_col_geom\s*\(\s*int\s+Py\s*,\s*int\s+Px\s*\)')
    for line in ('const int cw = st_cw(Py);', 'c.cw = cw; c.ncg = (Px + cw - 1) / cw; c.threads = st_col_threads(Py);',
                 'c.lds = ((size_t)Py * cw + Py) * sizeof(float2);'):
        assert line in geom, line
    g = SM.geometry(2048, 2048)
    assert (g['rows'], g['n_row_groups'], g['row_ne'], g['cw'], g['col_threads'], g['n_col_groups'], g['col_ne']) == (1, 2048, 8, 4, 512, 512, 16)
    g = SM.geometry(2048, 5)
    assert (g['rows'], g['n_row_groups'], g['rows_last'], g['n_col_groups'], g['cw_last']) == (409, 6, 3, 2, 1)
    g = SM.geometry(24, 24)
    assert (g['rows'], g['rows_unclipped'], g['n_row_groups'], g['n_col_groups']) == (24, 85, 1, 3)
    for shape in SM.SHAPES:
        assert SM.row_bands(*shape)[-1][1] == shape[0] and len(SM.row_bands(*shape)) == SM.geometry(*shape)['n_row_groups']
        assert SM.col_bands(*shape)[-1][1] == shape[1] and len(SM.col_bands(*shape)) == SM.geometry(*shape)['n_col_groups']


def test_radix_lists_multiply_back_to_the_side():
    for n in range(1, SM.ST_MAX_SIDE + 1):
        r = SM.factor(n)
        p = 1
        for q in r:
            p *= q
        assert p == n and len(r) <= SM.MAX_RADICES, (n, r)
        left = [q for q in r if q not in SM.PREF]
        assert all(q >= 11 and all(q % d for d in range(2, int(q ** 0.5) + 1)) for q in left), (n, r)     # what is left is prime
    assert SM.factor(1890) == [2, 9, 3, 5, 7] and SM.factor(2048) == [8, 8, 8, 4] and SM.factor(1331) == [11, 11, 11]
    assert SM.factor(2039) == [2039]


def test_every_class_is_reached():
    reached = {}
    for shape in SM.SHAPES:
        for c in SM.classes(*shape):
            reached.setdefault(c, []).append(shape)
    assert set(reached) <= set(SM.ALL_CLASSES), set(reached) - set(SM.ALL_CLASSES)
    missing = [c for c in SM.ALL_CLASSES if c not in reached]
    assert not missing, 'classes no entry of SHAPES reaches: %s' % missing
    assert (1024, 1024) in SM.SHAPES and (2048, 2048) in SM.SHAPES
    assert all(kw['B'] >= 4 for kw in SM.SHAPES.values())         # (one position over each corner)


def test_every_sequence_is_filed_at_both_column_classes():
    assert set(SM.SEQUENCE_SHAPES) == {'cw8_nt_gt256', 'cw4'}
    for cls, shape in SM.SEQUENCE_SHAPES.items():
        assert cls in SM.classes(*shape), (cls, shape)
    assert set(SM.SEQUENCE_CASES) == {(n, c) for n in SM.SEQUENCES for c in SM.SEQUENCE_SHAPES}
    reached = set().union(*(SM.features(n) for n in SM.SEQUENCES))
    assert reached == set(SM.REQUIRED_FEATURES), (reached ^ set(SM.REQUIRED_FEATURES))
    for n in SM.SEQUENCES:
        kw, _ = SM.sequence_kw(n)
        assert kw['B'] >= 4 and 'pp' not in kw and 'generic' not in kw, n


def test_sparse_cases_reach_the_new_geometries():
    cl = {n: SM.classes(*((kw['P'],) * 2 if isinstance(kw['P'], int) else kw['P'])) for n, kw in SM.SPARSE_CASES.items()}
    reached = set().union(*cl.values())
    for c in ('cw8_nt_gt256', 'cw4', 'nt_nonpow2_waves', 'nt512', 'row_single_ragged', 'rows_many_ragged', 'rows_clipped_to_Py',
              'leftover_prime_large_y', 'colgroup_ragged'):
        assert c in reached, c
    assert any(not isinstance(kw['P'], int) and kw['P'][0] % 2 and kw['P'][1] % 2 for kw in SM.SPARSE_CASES.values())      # odd sides
    assert max(kw['S'] for kw in SM.SPARSE_CASES.values()) - 1 > 7           # more gaps than any earlier test


def test_the_matrix_names_exactly_the_kernels_of_the_source():
    st = parsed()[0]
    found = set()
    for m in re.finditer(r'(template\s*<\s*bool\s+\w+\s*>\s*)?__global__\s+(?:__launch_bounds__\([^)]*\)\s+)?void\s+(\w+)\s*\(', st):
        name = m.group(2)
        found |= {name + '<false>', name + '<true>'} if m.group(1) else {name}
    assert len(re.findall(r'__global__', st)) == 9 and len(found) == 11, sorted(found)
    assert found == set(SM.KERNELS), found ^ set(SM.KERNELS)
    for k, (module, tests) in SM.KERNELS.items():
        with open(os.path.join(ROOT, 'tests', module + '.py')) as f:
            text = f.read()
        for t in tests:
            assert re.search(r'^def %s\(' % t, text, re.M), (k, module, t)
    # every instantiation of the templates is launched
    for name in ('st_col_conv_kernel', 'st_col_conv_sparse_kernel'):
        assert re.findall(r'st_col_launch\(conj \? %s<(\w+)> : %s<(\w+)>,' % (name, name), st) == [('true', 'false')], name


def test_the_column_helpers_are_defined_once():
    """What the translation units of the path share is defined exactly once under adorym_amd/csrc, in adm_ms_col.h, and no copy
    under the prefix of a translation unit exists."""
    names = ('st_cw', 'st_col_threads', 'st_col_fft', 'st_col_ctx', 'st_col_load', 'st_col_store', 'st_freq_index', 'st_freq',
             'st_col_geom', 'st_col_raise_lds', 'st_block_sum_f64', 'st_col_begin', 'st_shift_phase', 'st_col_raise_lds_once',
             'st_col_launch')
    srcs = {f: _read(f) for f in sorted(os.listdir(CSRC)) if f.endswith(('.hip', '.h'))}
    path = ('adm_ms_col.h', 'adm_ms_streamed.hip', 'adm_ms_exitshift.hip', 'adm_ms_probeshift.hip', 'adm_ms_multidist.hip')
    assert not any(re.search(r'\b(es|ps)_phase\b|\battr_set\b', srcs[f]) for f in path)      # (the copies that were)
    # a definition: the name, its parameter list, its body (a call is followed by ';', an operator or ')')
    definition = r'\b%s\s*\([^;{}()]*(?:\([^;{}()]*\)[^;{}()]*)*\)\s*\{'
    where = lambda text, files: [f for f in files for _ in re.finditer(text, srcs[f])]
    for n in names:
        assert where(definition % n, srcs) == ['adm_ms_col.h'], n
        assert not where(definition % ('es_' + n[3:]), srcs) + where(definition % ('ps_' + n[3:]), srcs), n
    # the constant, the LDS bytes (in no other spelling either), the dynamic-LDS limit and the attribute call
    for text, files in ((r'constexpr\s+int\s+ST_COL_NT\b', srcs), (re.escape('((size_t)Py * cw + Py) * sizeof(float2)'), srcs),
                        (r'sizeof\(float2\)', path), (re.escape('160 * 1024 - 256'), path), ('hipFuncAttributeMaxDynamicSharedMemorySize', path)):
        assert where(text, files) == ['adm_ms_col.h'], text
    assert not where(r'constexpr\s+int\s+(ES|PS)_COL_NT\b', srcs)
    assert all('#include "adm_ms_col.h"' in srcs[f] for f in path[1:])
    assert "'adm_ms_col.h'" in re.search(r'^HDRS = \[.*\]$', _read('build.py'), re.M).group(0)


@pytest.mark.parametrize('shape', list(SM.SHAPES))
def test_shape_classes_are_stable(shape):
    """What each swept field is there for (a table edited without a look at the classes fails here first)."""
    cl = SM.classes(*shape)
    assert len(cl & set(SM.ROW_CLASSES)) == 1, cl
    assert len(cl & {'cw8_nt256', 'cw8_nt_gt256', 'cw4'}) == 1, cl
