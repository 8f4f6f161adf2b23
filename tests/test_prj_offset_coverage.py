"""CPU-only bookkeeping of adm_ms_exitshift.hip: every __global__ kernel in it, and the reduction of its partials
(st_shift_reduce_kernel of adm_ms_streamed.hip), is named by a GPU test, every instantiation of its template is launched, and
ms_streamed_launch routes the detector step and the reduction.  (The column helpers it shares with the other translation units of
the path: tests/test_streamed_matrix_coverage.py.)"""
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, 'adorym_amd', 'csrc')

# kernel: (test module, tests whose docstrings name it)
KERNELS = {
    'es_col_conv_kernel<false>': ('test_gpu_prj_offset', ['test_kernels_vs_reference', 'test_geometries_vs_restatement']),
    'es_col_conv_kernel<true>': ('test_gpu_prj_offset', ['test_kernels_vs_reference', 'test_geometries_vs_restatement']),
    'st_shift_reduce_kernel': ('test_gpu_prj_offset', ['test_kernels_vs_reference', 'test_geometries_vs_restatement']),
}


def _read(name):
    with open(os.path.join(CSRC, name)) as f:
        return f.read()


def test_every_kernel_is_named_by_a_gpu_test():
    es = _read('adm_ms_exitshift.hip')
    found = set()
    for m in re.finditer(r'(template\s*<\s*bool\s+\w+\s*>\s*)?__global__\s+(?:__launch_bounds__\([^)]*\)\s+)?void\s+(\w+)\s*\(', es):
        found |= {m.group(2) + '<false>', m.group(2) + '<true>'} if m.group(1) else {m.group(2)}
    assert len(re.findall(r'__global__', es)) == 1 and found | {'st_shift_reduce_kernel'} == set(KERNELS), found ^ set(KERNELS)
    for k, (module, tests) in KERNELS.items():
        text = open(os.path.join(ROOT, 'tests', module + '.py')).read()
        for t in tests:
            m = re.search(r'^def %s\(.*?\n    """(.*?)"""' % t, text, re.M | re.S)
            assert m and k in m.group(1), (k, t)
    # every instantiation is launched, through the one launch line of adm_ms_col.h
    assert re.findall(r'st_col_launch\(conj \? es_col_conv_kernel<(\w+)> : es_col_conv_kernel<(\w+)>,', es) == [('true', 'false')]
    assert 'hipLaunchKernelGGL' not in es
    assert 'reduce_kernel' not in re.sub(r'//.*', '', es)          # the reduction is the streamed file's


def test_the_streamed_launch_routes_the_detector_step():
    """ms_streamed_launch hands the detector step's column launches (and nothing else) to the new translation unit, and the
    reduction runs once, after the adjoint sweep."""
    st = _read('adm_ms_streamed.hip')
    assert len(re.findall(r'ms_exitshift_col_launch\(', st)) == 1
    # the reduction: st_shift_reduce_kernel, once for each kind of shift; this one is the last launch, behind a gradient buffer
    launches = [m.start() for m in re.finditer(r'hipLaunchKernelGGL\(st_shift_reduce_kernel\b', st)]
    assert len(launches) == 2 and max(m.start() for m in re.finditer(r'hipLaunchKernelGGL\(', st)) == launches[1]
    assert st[:launches[1]].rstrip().endswith('if (e == hipSuccess && xs && xs->grad_shifts) {')
    assert 'st, xs->part, batch, M * ncg, xs->index, xs->grad_shifts);' in st[launches[1]:st.index(';', launches[1]) + 1]
    assert 'reduce_launch' not in st + _read('adm_host.h')
    assert len(re.findall(r'det_col\((?:true|false)\)', st)) == 2
    build = open(os.path.join(CSRC, 'build.py')).read()
    assert "'adm_ms_exitshift.hip'" in build
