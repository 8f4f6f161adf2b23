"""CPU: the tables of tests/ctf_dist_matrix.py against the sources of the CTF distance gradient.  Fails when the new entry point or
a run-time branch of the feature lacks a row or a test, when a branch's text has left the source, or when a field is not one of
tests/ctf_matrix.FIELDS."""
import os
import re

from tests import ctf_dist_matrix as DM
from tests import ctf_matrix as CM

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _read(*p):
    with open(os.path.join(ROOT, *p)) as f:
        return f.read()


SRC = {n: _read('adorym_amd', 'csrc', n) for n in ('adm_holo_ctf.hip', 'adm_ctf_dist.hip', 'adm_ctf_group.h')}
GPU_TESTS = set()
for mod in ('test_gpu_ctf_dist.py', 'test_gpu_ctf_group_bits.py'):
    GPU_TESTS |= set(re.findall(r'^def (test_\w+)\(', _read('tests', mod), re.M))


def test_the_entry_point_has_a_row_a_declaration_and_a_binding():
    defined = set(re.findall(r'^extern "C"\s+[\w \t*]+?\b(adm_\w+)\s*\(', SRC['adm_ctf_dist.hip'], re.M))
    assert defined == set(DM.ENTRY_POINTS) == {'adm_ctfd_fwd_adj'}
    header = re.sub(r'/\*.*?\*/', '', _read('include', 'adm.h'), flags=re.S)
    assert re.search(r'\badm_ctfd_fwd_adj\s*\(', header)
    assert "'adm_ctfd_fwd_adj'" in _read('adorym_amd', '_lib.py')
    assert 'adm_ctfd_fwd_adj' in _read('INTEGRATION.md')
    # no kernel and no use of the line machinery (adm_line_fft.h) outside adm_holo_ctf.hip
    for n in ('adm_ctf_dist.hip', 'adm_ctf_group.h'):
        assert '__global__' not in SRC[n] and 'line_fft' not in SRC[n] and 'stockham' not in SRC[n], n
    from adorym_amd.csrc import build
    assert 'adm_ctf_dist.hip' in build.SRCS and 'adm_ctf_group.h' in build.HDRS


def test_every_branch_is_in_the_source_and_names_tests_that_exist():
    for name, (src, text, tests) in DM.BRANCHES.items():
        assert text in SRC[src], (name, 'not in', src)
        assert tests and set(tests) <= GPU_TESTS, (name, set(tests) - GPU_TESTS)
    for name, tests in DM.ENTRY_POINTS.items():
        assert tests and set(tests) <= GPU_TESTS, (name, set(tests) - GPU_TESTS)
    assert set(DM.ENGINE_TESTS) <= GPU_TESTS


def test_every_field_is_one_of_the_ctf_matrix_and_every_class_is_reached():
    got = set()
    for f in DM.FIELDS:
        assert f in CM.FIELDS and f[0] * f[1] <= 32768, f
        got |= DM.classes(*f)
    assert got == set(DM.ALL_CLASSES), set(DM.ALL_CLASSES) ^ got
    assert DM.VARIANT_FIELD in DM.FIELDS and DM.PHASE_FIELD in CM.FIELDS and DM.PHASE_RUNG == 3000.
    # what the issue names
    assert {'nd_1', 'c4_idle_slots'} <= DM.classes(16, 16, 1)
    assert {'c4_ragged_last_round', 'line_sum_lds_2_waves'} <= DM.classes(1024, 16, 3)
    assert {'nd_64', 'several_dist_sums_per_block'} <= DM.classes(256, 16, 64)
    assert {'c4_one_slot', 'line_sum_lds_4_waves'} <= DM.classes(2048, 16, 3)
    assert 'many_partials_per_distance' in DM.classes(16, 2048, 2)
    g = CM.geometry(256, 16, 64)
    assert (g['c4_rounds'], len(g['row_blocks'])) == (8, 2)          # 64 distance sums + 65 others over two C5 blocks


def test_the_kernel_file_keeps_its_shape():
    """What tests/test_ctf_coverage.py pins, restated for the feature: six kernels, three entry points, and the distance gradient
    inside them."""
    code = re.sub(r'//[^\n]*', '', SRC['adm_holo_ctf.hip'])
    assert len(re.findall(r'__global__', code)) == 6
    assert len(re.findall(r'^extern "C"', SRC['adm_holo_ctf.hip'], re.M)) == 3
    # the line machinery is the header's, included by the kernel file alone of the three
    assert '#include "adm_line_fft.h"' in SRC['adm_holo_ctf.hip'] and 'stockham' not in code
    assert 'adm_line_fft.h' not in SRC['adm_ctf_dist.hip'] and 'adm_line_fft.h' not in SRC['adm_ctf_group.h']
    assert re.search(r'static_assert\(3 \* LG::LPB \* LG::LP \* sizeof\(cf\) \+ 256 \* sizeof\(double\)', SRC['adm_holo_ctf.hip'])
    assert not re.search(r'\batomic\w*\s*\(', code)          # every sum has a fixed order
