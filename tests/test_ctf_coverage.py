"""CPU: the tables of tests/ctf_matrix.py against the text of adorym_amd/csrc/adm_holo_ctf.hip and of the line machinery it includes
(adm_line_fft.h, adm_line_host.h).  Fails when a __global__ kernel, an
extern "C" entry point, an accepted size or a class of the mirror lacks a row or a test, or when the mirror's launch arithmetic
no longer restates the source's."""
import os
import re

from tests import ctf_matrix as CM

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _read(*p):
    with open(os.path.join(ROOT, *p)) as f:
        return f.read()


SRC = _read('adorym_amd', 'csrc', 'adm_holo_ctf.hip')
HDR = _read('adorym_amd', 'csrc', 'adm_line_fft.h')
HOST = _read('adorym_amd', 'csrc', 'adm_line_host.h')
CODE = re.sub(r'//[^\n]*', '', SRC)
GPU_TESTS = set(re.findall(r'^def (test_\w+)\(', _read('tests', 'test_gpu_ctf.py'), re.M))


def source_kernels():
    """{family: template parameter list or None} of every __global__ function."""
    out = {}
    for m in re.finditer(r'(?:template\s*<([^>]*)>\s*)?__global__\s+(?:__launch_bounds__\(\d+\)\s+)?void\s+(\w+)\s*\(', CODE):
        out[m.group(2)] = m.group(1)
    return out


def test_every_kernel_has_a_row_and_every_row_a_kernel():
    fams = set()
    for name, tpl in source_kernels().items():
        if tpl is None:
            fams.add(name)
        elif 'bool' in tpl:
            fams |= {'%s<N, true>' % name, '%s<N, false>' % name}
        else:
            fams.add('%s<N>' % name)
    assert fams == set(CM.KERNELS), (fams ^ set(CM.KERNELS))
    assert len(source_kernels()) == len(re.findall(r'__global__', CODE)) == 6


def test_every_row_names_tests_that_exist():
    for table in (CM.KERNELS, CM.ENTRY_POINTS):
        for k, row in table.items():
            tests = row[-1] if table is CM.KERNELS else row
            assert tests and set(tests) <= GPU_TESTS, (k, set(tests) - GPU_TESTS)


def test_every_entry_point_has_a_row():
    defined = set(re.findall(r'^extern "C"\s+[\w \t*]+?\b(adm_\w+)\s*\(', SRC, re.M))
    assert defined == set(CM.ENTRY_POINTS) and len(defined) == 3
    header = re.sub(r'/\*.*?\*/', '', _read('include', 'adm.h'), flags=re.S)
    assert defined == set(re.findall(r'\b(adm_ctf_\w+)\s*\(', header))


def test_every_accepted_size_is_launched_in_both_roles():
    sizes = tuple(int(v) for v in re.findall(r'X\((\d+)\)', re.search(r'#define ADM_LINE_SIZES\(X\)([^\n]*)', HDR).group(1)))
    assert sizes == CM.SIZES
    assert all(CM.pow2_in_range(n) for n in sizes) and not CM.pow2_in_range(sizes[0] // 2) and not CM.pow2_in_range(sizes[-1] * 2)
    assert re.search(r'ADM_LINE_MIN_SIDE = 16, ADM_LINE_MAX_SIDE = 2048;', HOST)
    assert re.search(r'n >= ADM_LINE_MIN_SIDE && n <= ADM_LINE_MAX_SIDE && \(n & \(n - 1\)\) == 0', HOST)
    assert re.search(r'if \(!line_side_ok\(d\.ny\) \|\| !line_side_ok\(d\.nx\)\)', SRC)
    assert re.search(r'#define ADM_CTF_MAX_DISTS 64', SRC) and CM.MAX_DISTS == 64
    want = {(k, n) for k, (axis, _) in CM.KERNELS.items() for n in (sizes if axis else (0,))}
    assert CM.reached() == want, sorted(want - CM.reached())
    # every switch of ctf_run dispatches over the whole list
    assert len(re.findall(r'ADM_LINE_SIZES\(C\w+\)', SRC)) == 6


def test_every_class_is_reached_and_every_field_is_small():
    got = set()
    for f in CM.FIELDS:
        assert f[0] * f[1] <= 32768 and CM.pow2_in_range(f[0]) and CM.pow2_in_range(f[1]) and 1 <= f[2] <= CM.MAX_DISTS
        got |= CM.classes(*f)
    assert got == set(CM.ALL_CLASSES), set(CM.ALL_CLASSES) ^ got
    assert CM.VARIANT_FIELD in CM.FIELDS
    # what the issue names: a block that is not full, a row block over two distances, both orientations, the longest side in each
    # role, one / odd / 64 distances, a ragged last round
    assert 'partial_block' in CM.classes(16, 16, 1) and 'c3_block_spans_distances' in CM.classes(16, 16, 3)
    for f in ((32, 16), (16, 32), (64, 512), (512, 64), (2048, 16), (16, 2048), (256, 16)):
        assert any(g[:2] == f for g in CM.FIELDS), f
    assert 'c4_ragged_last_round' in CM.classes(1024, 16, 3) and 'nd_64' in CM.classes(256, 16, 64)


def test_the_mirror_restates_the_launch_arithmetic():
    assert re.search(r'TPR = N / 8;', HDR) and re.search(r'LPB = 256 / TPR;', HDR)
    assert re.search(r'LP = N \+ \(LPB > 1 \? 32 / \(LPB < 32 \? LPB : 32\) : 0\);', HDR)
    assert re.search(r'USE = \(N <= 1024\);', HDR)
    assert re.search(r'return \(lines \+ LineGeo<N>::LPB - 1\) / LineGeo<N>::LPB;', HDR)
    launches = dict(re.findall(r'#define (C\w+)\(N_\) case N_: hipLaunchKernelGGL\(\(ctf_c\d<N_(?:, \w+)?>\), (dim3\(.*?\)), dim3\(256\)', SRC))
    assert launches == {'C1': 'dim3(blocks_for<N_>(A.ny))', 'C2': 'dim3(blocks_for<N_>(A.nx), A.nd)',
                        'C3G': 'dim3(blocks_for<N_>(A.nd * A.ny))', 'C3N': 'dim3(blocks_for<N_>(A.nd * A.ny))',
                        'C4': 'dim3(A.nx)', 'C5': 'dim3(blocks_for<N_>(A.ny))'}, launches
    assert re.search(r'ctf_sums_kernel, dim3\(A\.nd\), dim3\(64\)', SRC)
    assert re.search(r'for \(int d0 = 0; d0 < A\.nd; d0 \+= LG::LPB\)', SRC)            # C4's rounds
    assert re.search(r'for \(int o = blockIdx\.x; o <= A\.nd; o \+= gridDim\.x\)', SRC)   # the nd + 1 sums over C5's blocks
    g = CM.geometry(1024, 16, 3)
    assert (g['gy']['LPB'], g['c4_rounds'], g['c4_ragged'], len(g['c3_blocks']), len(g['row_blocks'])) == (2, 2, True, 24, 8)
    g = CM.geometry(256, 16, 64)
    assert (g['c4_rounds'], g['n_sums'], len(g['row_blocks']), g['sums_per_block']) == (8, 65, 2, 33)


def test_the_old_line_machinery_is_untouched_and_the_new_file_is_built():
    from adorym_amd.csrc import build
    assert 'adm_holo_ctf.hip' in build.SRCS
    assert 'ctf' not in _read('adorym_amd', 'csrc', 'adm_holo.hip').lower()
