"""CPU-only bookkeeping of adm_ms_multidist.hip (one exit wave to several detector planes on streamed plans): the entry point is
declared, exported and bound; every __global__ kernel in the file is named by a GPU test; ms_streamed_launch reaches the file only
through one more optional pointer; the file is built; its recorded resource usage shows no scratch.  (The column helpers it shares
with the other translation units of the path: tests/test_streamed_matrix_coverage.py.)"""
import ctypes
import os
import re

from tests.test_kernel_matrix_coverage import _function_body

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, 'adorym_amd', 'csrc')

# kernel instantiation: (test module, tests whose docstrings name it); the instantiations with the distance gradient are listed, and
# held to their tests, by tests/test_distgrad_coverage.py
KERNELS = {
    'md_fanout_kernel<false>': ('test_gpu_multidist3d', ['test_kernels_vs_reference', 'test_geometries_vs_restatement']),
    'md_fanin_kernel<false>': ('test_gpu_multidist3d', ['test_kernels_vs_reference', 'test_geometries_vs_restatement']),
}
WITH_GRADIENT = {'md_fanout_kernel<true>', 'md_fanin_kernel<true>'}


def _read(name):
    with open(os.path.join(CSRC, name)) as f:
        return f.read()


def test_the_entry_point_is_declared_exported_and_bound():
    import __graft_entry__ as g
    g.build()
    from adorym_amd import _lib
    hdr = re.sub(r'/\*.*?\*/', '', open(os.path.join(ROOT, 'include', 'adm.h')).read(), flags=re.S)
    assert re.search(r'\bint\s+adm_plan_set_detector_fanout\s*\(\s*adm_plan\*\s*plan,\s*int\s+n,\s*const float\*\s*hfree_re,\s*const float\*\s*hfree_im\)', hdr)
    assert hasattr(ctypes.CDLL(_lib.LIB_PATH), 'adm_plan_set_detector_fanout')
    restype, argtypes = _lib.SIGNATURES['adm_plan_set_detector_fanout']
    assert restype is ctypes.c_int and len(argtypes) == 4 and argtypes[1] is ctypes.c_int
    # the setter that means something else (one sweep per entry) keeps its refusal of n > 1 on streamed plans
    api = _read('adm_api.hip')
    body = _function_body(api, r'extern "C" int adm_plan_set_detector_kernels\s*\(')
    assert 'if (n > 1 && plan->streamed)' in body and 'fan' not in body


def test_every_kernel_is_named_by_a_gpu_test():
    from tests.test_distgrad_coverage import KERNELS as DIST
    md = _read('adm_ms_multidist.hip')
    found = set()
    for m in re.finditer(r'(template\s*<([^>]*)>\s*)?__global__\s+(?:__launch_bounds__\([^)]*\)\s+)?void\s+(\w+)\s*\(', md):
        assert m.group(1) and m.group(2).strip() == 'bool GRAD', 'both kernels are templates on the distance gradient'
        found |= {m.group(3) + '<false>', m.group(3) + '<true>'}
    assert len(re.findall(r'__global__', md)) == 2 and found == set(KERNELS) | WITH_GRADIENT, found ^ set(KERNELS)
    assert WITH_GRADIENT <= set(DIST)
    for k, (module, tests) in KERNELS.items():
        text = open(os.path.join(ROOT, 'tests', module + '.py')).read()
        for t in tests:
            m = re.search(r'^def %s\(.*?\n    """(.*?)"""' % t, text, re.M | re.S)
            assert m and k in m.group(1), (k, t)
    # every instantiation is launched, once: one launch line per template, which picks by the request
    for k in ('md_fanout_kernel', 'md_fanin_kernel'):
        line = 'st_col_launch(fo.grad_dists ? %s<true> : %s<false>, cg, batch * p.n_modes, st, p, fld, q, r);' % (k, k)
        assert md.count(line) == 1 and len(re.findall(r'st_col_launch\(', md)) == 2, k
        assert re.search(r'__launch_bounds__\(ST_COL_NT\)\s+void\s+%s\b' % k, md), k
    assert 'hipLaunchKernelGGL' not in md
    code = re.sub(r'//.*', '', md)
    assert not re.search(r'\batomic\w*\s*\(', code)              # a fixed order of the sum over the distances and of the partials
    assert 'reduce_kernel' not in code
    assert '#include "adm_ms_col.h"' in md and 'st_col_geom(' in md and 'st_col_raise_lds_once(' in md and 'st_block_sum_f64(' in md


def test_the_streamed_launch_reaches_the_file_only_with_its_pointer():
    """Every call into the new translation unit and every launch over the detector entries hang on ``fo``: with fo == nullptr the
    body issues the launches it always did."""
    st = _read('adm_ms_streamed.hip')
    body = _function_body(st, r'hipError_t\s+ms_streamed_launch\s*\([^)]*const StFanoutLaunch\* fo,[^)]*\)')
    assert len(re.findall(r'ms_multidist_fanout_launch\(', st)) == 1 and len(re.findall(r'ms_multidist_fanin_launch\(', st)) == 1
    assert 'e = fo ? ms_multidist_fanout_launch(p, batch, fld, *fo, st) : det_col(false);' in body
    assert 'if (e == hipSuccess) e = fo ? det_row_only(2) : row(0, 0, 2, 0, 0, 0);' in body
    assert 'e = fo ? detect(pd, batch * fo->n, fo->fld) : detect(p, batch, fld);' in body
    assert 'e = fo ? det_row_only(1) : row(0, 0, 1, 0, 0, 0);' in body
    assert 'if (e == hipSuccess) e = fo ? ms_multidist_fanin_launch(p, batch, fld, *fo, st) : det_col(true);' in body
    # the sweep itself runs over `batch` positions whatever fo->n is: its launches do not name fo
    for line in body.split('\n'):
        if re.search(r'\be = (row\(s,|conv\()', line):
            assert 'fo' not in line, line
    host = _read('adm_host.h')
    assert re.search(r'const StFanoutLaunch\* fo = nullptr', host)


def test_the_file_is_built_and_documented():
    build = _read('build.py')
    assert "'adm_ms_multidist.hip'" in re.search(r'^SRCS = \[.*\]$', build, re.M).group(0)
    for doc in ('README.md', 'DESIGN.md'):
        assert 'adm_ms_multidist.hip' in open(os.path.join(ROOT, doc)).read(), doc
    assert os.path.exists(os.path.join(ROOT, 'tools', 'bench_multidist3d.py'))


def test_resource_usage_is_recorded_without_scratch():
    text = open(os.path.join(ROOT, 'profiles', 'multidist3d', 'resource_usage.txt')).read()
    names = re.findall(r'Function Name: (\S+)', text)
    for k in ('md_fanout_kernelILb0E', 'md_fanin_kernelILb0E'):          # (the <false> instantiations as the compiler names them)
        assert any(k in n for n in names), k
    scratch = re.findall(r'ScratchSize \[bytes/lane\]: (\d+)', text)
    assert len(scratch) == len(names) == 2 and set(scratch) == {'0'}
    assert len(re.findall(r'VGPRs: \d+', text)) >= 2 and len(re.findall(r'LDS Size \[bytes/block\]: \d+', text)) == 2
