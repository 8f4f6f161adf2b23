"""CPU: the tables of tests/ctfinv_matrix.py against the text of adorym_amd/csrc/adm_ctf_invert.hip and of the line machinery it
includes (adm_line_fft.h, adm_line_host.h), and the layout of that machinery: one definition of each piece.  Fails when a
__global__ kernel, an extern "C" entry point, an accepted size or a class of the mirror lacks a row or a test, or when the mirror's
launch arithmetic no longer restates the source's."""
import os
import re

from tests import ctfinv_matrix as M

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _read(*p):
    with open(os.path.join(ROOT, *p)) as f:
        return f.read()


SRC = _read('adorym_amd', 'csrc', 'adm_ctf_invert.hip')
HDR = _read('adorym_amd', 'csrc', 'adm_line_fft.h')
HOST = _read('adorym_amd', 'csrc', 'adm_line_host.h')
CODE = re.sub(r'//[^\n]*', '', SRC)
GPU_TESTS = set(re.findall(r'^def (test_\w+)\(', _read('tests', 'test_gpu_ctfinv.py'), re.M))


def source_kernels():
    """{family: template parameter list or None} of every __global__ function."""
    out = {}
    for m in re.finditer(r'(?:template\s*<([^>]*)>\s*)?__global__\s+(?:__launch_bounds__\(\d+\)\s+)?void\s+(\w+)\s*\(', CODE):
        out[m.group(2)] = m.group(1)
    return out


def test_every_kernel_has_a_row_and_every_row_a_kernel():
    fams = {'%s<N>' % name if tpl else name for name, tpl in source_kernels().items()}
    assert fams == set(M.KERNELS), (fams ^ set(M.KERNELS))
    assert len(source_kernels()) == len(re.findall(r'__global__', CODE)) == 3
    assert 'atomic' not in CODE.lower()


def test_every_row_names_tests_that_exist():
    for table in (M.KERNELS, M.ENTRY_POINTS):
        for k, row in table.items():
            tests = row[-1] if table is M.KERNELS else row
            assert tests and set(tests) <= GPU_TESTS, (k, set(tests) - GPU_TESTS)


def test_every_entry_point_has_a_row():
    defined = set(re.findall(r'^extern "C"\s+[\w \t*]+?\b(adm_\w+)\s*\(', SRC, re.M))
    assert defined == set(M.ENTRY_POINTS) and len(defined) == 3
    header = re.sub(r'/\*.*?\*/', '', _read('include', 'adm.h'), flags=re.S)
    assert defined == set(re.findall(r'\b(adm_ctfinv_\w+)\s*\(', header))
    from adorym_amd import _lib
    assert defined == {k for k in _lib.SIGNATURES if k.startswith('adm_ctfinv_')}
    # the descriptor of the header is the ctypes structure
    desc = re.search(r'typedef struct adm_ctfinv_desc \{(.*?)\} adm_ctfinv_desc;', header, re.S).group(1)
    names = [n.strip() for line in desc.split(';') if line.strip() for n in line.split(None, 1)[1].split(',')]
    assert names == [n for n, _ in _lib.CtfInvDesc._fields_], names


def test_every_accepted_size_is_launched_in_both_roles():
    sizes = tuple(int(v) for v in re.findall(r'X\((\d+)\)', re.search(r'#define ADM_LINE_SIZES\(X\)([^\n]*)', HDR).group(1)))
    assert sizes == M.SIZES
    assert all(M.pow2_in_range(n) for n in sizes) and not M.pow2_in_range(sizes[0] // 2) and not M.pow2_in_range(sizes[-1] * 2)
    assert re.search(r'ADM_LINE_MIN_SIDE = 16, ADM_LINE_MAX_SIDE = 2048;', HOST)
    assert re.search(r'n >= ADM_LINE_MIN_SIDE && n <= ADM_LINE_MAX_SIDE && \(n & \(n - 1\)\) == 0', HOST)
    assert re.search(r'if \(!line_side_ok\(d\.ny\) \|\| !line_side_ok\(d\.nx\)\)', SRC)
    assert re.search(r'#define ADM_CTFINV_MAX_DISTS 64', SRC) and M.MAX_DISTS == 64
    want = {(k, n) for k in M.KERNELS for n in sizes}
    assert M.reached() == want, sorted(want - M.reached())
    # every switch of ctfinv_run dispatches over the whole list
    assert len(re.findall(r'ADM_LINE_SIZES\(I\d\)', SRC)) == 3


def test_every_class_is_reached_and_every_field_is_small():
    got = set()
    for name, kw in M.CASES.items():
        f = kw['field']
        assert f[0] * f[1] <= 32768 and M.pow2_in_range(f[0]) and M.pow2_in_range(f[1]) and 1 <= f[2] <= M.MAX_DISTS, name
        got |= M.classes(*f, **{k: v for k, v in kw.items() if k != 'field'})
    assert got == set(M.ALL_CLASSES), set(M.ALL_CLASSES) ^ got
    assert all(M.CASES['%dx%dx%d' % f] == dict(field=f) for f in M.FIELDS)
    # what the issue names
    assert 'i1_block_spans_distances' in M.classes(16, 16, 3)
    g = M.geometry(16, 16, 3, 3)
    assert [hi - lo for lo, hi in g['i1_blocks']] == [128, 16] and g['i1_spans_batch'] == [True, False]       # 144 jobs in blocks of 128
    assert {'i1_block_spans_batch', 'batch_3', 'one_round'} <= M.classes(16, 16, 3, nb=3, max_batch=3)
    assert {'several_rounds', 'ragged_last_round', 'batch_3'} <= M.classes(16, 16, 3, nb=3, max_batch=2) and M.rounds(3, 2) == [(0, 2), (2, 1)]
    assert {'spare_batch_capacity', 'batch_1'} <= M.classes(16, 16, 3, nb=1, max_batch=2)
    assert {'twiddles_global', 'tpr_gt_64'} <= M.classes(2048, 16, 3) & M.classes(16, 2048, 2)
    assert 'nd_1' in M.classes(16, 16, 1) and 'nd_odd' in M.classes(16, 16, 3) and 'nd_64' in M.classes(256, 16, 64)
    assert any(kw.get('out_stride') == 2 for kw in M.CASES.values()) and any(kw.get('alpha') == 'table' for kw in M.CASES.values())
    assert M.VALUE_CASES['pure_phase']['lg_kappa'] == 30. and len(M.VALUE_CASES) == len(M.PHASE_RUNGS) + 1


def test_the_mirror_restates_the_launch_arithmetic():
    assert re.search(r'TPR = N / 8;', HDR) and re.search(r'LPB = 256 / TPR;', HDR)
    assert re.search(r'LP = N \+ \(LPB > 1 \? 32 / \(LPB < 32 \? LPB : 32\) : 0\);', HDR)
    assert re.search(r'USE = \(N <= 1024\);', HDR)
    assert re.search(r'return \(lines \+ LineGeo<N>::LPB - 1\) / LineGeo<N>::LPB;', HDR)
    launches = dict(re.findall(r'#define (I\d)\(N_\) case N_: hipLaunchKernelGGL\(\(ctfinv_i\d<N_>\), (dim3\(.*?\)), dim3\(256\)', SRC))
    assert launches == {'I1': 'dim3(blocks_for<N_>(A.nb * A.nd * A.ny))', 'I2': 'dim3(blocks_for<N_>(A.nx), A.nb)',
                        'I3': 'dim3(blocks_for<N_>(A.nb * A.ny))'}, launches
    assert re.search(r'const int j = job0 \+ c, bd = j / ny, yy = j % ny;', SRC)                      # I1's jobs (b, d, y)
    assert re.search(r'for b0 in range\(0, B, self\.max_batch\):', _read('adorym_amd', 'holography.py'))   # retrieve's rounds
    g = M.geometry(1024, 16, 3)
    assert (g['gy']['LPB'], len(g['i1_blocks']), len(g['i3_blocks']), g['i2_grid']) == (2, 24, 8, (8, 1))
    g = M.geometry(64, 32, 3, 2)
    assert (len(g['i1_blocks']), len(g['i3_blocks']), g['i2_grid']) == (6, 2, (1, 2))


# definition-shaped: what opens the one definition of each piece of the line machinery (a call, a use or a comment does not match)
PIECES = {
    'stockham_pass': r'void stockham_pass\(', 'line_sync': r'void line_sync\(', 'Passes': r'struct Passes \{', 'LineGeo': r'struct LineGeo \{',
    'store_lines_transposed': r'void store_lines_transposed\(', 'TwLds': r'struct TwLds \{', 'stage_twiddles': r'const float2\* stage_twiddles\(',
    'line_fft': r'cf\* line_fft\(', 'line_sum': r'\w+ line_sum\(', 'line_sums': r'void line_sums\(', 'mul_rounded': r'float mul_rounded\(',
    'blocks_for': r'int blocks_for\(',
}
HOST_PIECES = {
    'the twiddle loop': r'-2\.0 \* M_PI \* \(double\)j / \(double\)N', 'the frequency mesh': r'uv\[\(size_t\)x \* ny \+ y\] = u \* u \+ v \* v;',
    'line_side_ok': r'bool line_side_ok\(', 'line_upload_twiddles': r'int line_upload_twiddles\(', 'line_upload_uv2t': r'int line_upload_uv2t\(',
}


def test_the_line_machinery_is_one_header_of_the_three_files():
    from adorym_amd.csrc import build
    assert 'adm_ctf_invert.hip' in build.SRCS and 'adm_line_fft.h' in build.HDRS and 'adm_line_host.h' in build.HDRS
    names = sorted(n for n in os.listdir(os.path.join(ROOT, 'adorym_amd', 'csrc')) if n.endswith(('.hip', '.h')))
    assert set(build.SRCS + [h for h in build.HDRS if os.sep not in h]) <= set(names)
    text = {n: re.sub(r'//[^\n]*', '', _read('adorym_amd', 'csrc', n)) for n in names}
    for hdr in ('adm_line_fft.h', 'adm_line_host.h'):
        users = sorted(n for n in names if '"%s"' % hdr in text[n])
        assert users == ['adm_ctf_invert.hip', 'adm_holo.hip', 'adm_holo_ctf.hip'], (hdr, users)
    for n in ('adm_ctf_invert.hip', 'adm_holo.hip', 'adm_holo_ctf.hip'):
        assert len(re.findall(r'^using namespace linefft;$', text[n], re.M)) == 1, n
    # every piece is defined exactly once under adorym_amd/csrc, in its header
    for table, home in ((PIECES, 'adm_line_fft.h'), (HOST_PIECES, 'adm_line_host.h')):
        for piece, shape in table.items():
            where = {n: len(re.findall(shape, t)) for n, t in text.items() if n != 'adm_api.hip' or table is PIECES}
            assert {n: c for n, c in where.items() if c} == {home: 1}, (piece, where)
    # one size list
    lists = {n: len(re.findall(r'X\(16\) X\(32\) X\(64\) X\(128\) X\(256\) X\(512\) X\(1024\) X\(2048\)', t)) for n, t in text.items()}
    assert {n: c for n, c in lists.items() if c} == {'adm_line_fft.h': 1}, lists
