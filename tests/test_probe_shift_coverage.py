"""CPU-only bookkeeping of adm_ms_probeshift.hip: every __global__ kernel in it, and the reduction of its partials
(st_shift_reduce_kernel of adm_ms_streamed.hip), is named by a GPU test, every instantiation of its template is launched, and
ms_streamed_launch reaches them only through a plan's third optional pointer.  (The column helpers it shares with the other
translation units of the path: tests/test_streamed_matrix_coverage.py.)"""
import os
import re

from tests.test_kernel_matrix_coverage import _function_body

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, 'adorym_amd', 'csrc')

# kernel: (test module, tests whose docstrings name it)
KERNELS = {
    'ps_colfft_kernel': ('test_gpu_streamed_probe_shift', ['test_geometries_vs_oracle']),
    'ps_col_kernel<false>': ('test_gpu_streamed_probe_shift', ['test_geometries_vs_oracle']),
    'ps_col_kernel<true>': ('test_gpu_streamed_probe_shift', ['test_geometries_vs_oracle']),
    'st_shift_reduce_kernel': ('test_gpu_streamed_probe_shift', ['test_geometries_vs_oracle']),
}


def _read(name):
    with open(os.path.join(CSRC, name)) as f:
        return f.read()


def test_every_kernel_is_named_by_a_gpu_test():
    ps = _read('adm_ms_probeshift.hip')
    found = set()
    for m in re.finditer(r'(template\s*<\s*bool\s+\w+\s*>\s*)?__global__\s+(?:__launch_bounds__\([^)]*\)\s+)?void\s+(\w+)\s*\(', ps):
        found |= {m.group(2) + '<false>', m.group(2) + '<true>'} if m.group(1) else {m.group(2)}
    assert len(re.findall(r'__global__', ps)) == 2 and found | {'st_shift_reduce_kernel'} == set(KERNELS), found ^ set(KERNELS)
    for k, (module, tests) in KERNELS.items():
        text = open(os.path.join(ROOT, 'tests', module + '.py')).read()
        for t in tests:
            m = re.search(r'^def %s\(.*?\n    """(.*?)"""' % t, text, re.M | re.S)
            assert m and k in m.group(1), (k, t)
    # every instantiation is launched, through the one launch line of adm_ms_col.h
    assert re.findall(r'st_col_launch\(conj \? ps_col_kernel<(\w+)> : ps_col_kernel<(\w+)>,', ps) == [('true', 'false')]
    assert len(re.findall(r'st_col_launch\(ps_colfft_kernel\b', ps)) == 1 and 'hipLaunchKernelGGL' not in ps
    assert 'reduce_kernel' not in re.sub(r'//.*', '', ps)          # the reduction is the streamed file's
    # no atomics in the file
    assert not re.search(r'\batomic\w*\s*\(', ps)


def test_the_streamed_launch_reaches_the_file_only_with_the_third_pointer():
    """Every call into the new translation unit, the extra row launches and every changed argument of the sweep's row launches
    hang on ``ps``: with ps == nullptr the body issues the launches it always did."""
    st = _read('adm_ms_streamed.hip')
    body = _function_body(st, r'hipError_t\s+ms_streamed_launch\s*\([^)]*const StProbeShiftLaunch\* ps\)')
    assert len(re.findall(r'ms_probeshift_spectrum_launch\(', body)) == 1 and len(re.findall(r'ms_probeshift_col_launch\(', body)) == 2
    assert 'reduce_launch' not in body
    # the sweep's launches: today's arguments when ps is null
    assert 'e = row(s, 1, s > 0 || ps ? 2 : 0, s < S - 1 ? 1 : det_row, s == 0 && !ps, 0);' in body
    assert 'const bool ps_adj = ps && (p.grad_probe || ps->grad_shifts);' in body
    assert 'e = row(s, 2, s == S - 1 ? adj_row : 2, s > 0 || ps_adj ? 1 : 0, 0, s == 0 && !ps_adj);' in body
    # everything else that names the new unit sits inside `if (ps)` / `if (... && ps_adj)`
    for m in re.finditer(r'ms_probeshift_\w+\(', body):
        head = body[:m.start()]
        assert head.rfind('if (ps) {') > head.rfind('// ---------------- forward') or head.rfind('&& ps_adj) {') > head.rfind('// ---------------- adjoint'), m.group(0)
    # the reduction: the first of the two st_shift_reduce_kernel launches, inside the ps_adj block one level down, under
    # ps->grad_shifts; then the sparse reduction, then the exit-shift one
    launches = [m.start() for m in re.finditer(r'hipLaunchKernelGGL\(st_shift_reduce_kernel\b', body)]
    assert len(launches) == 2 == len(re.findall(r'hipLaunchKernelGGL\(st_shift_reduce_kernel\b', st))
    head = body[:launches[0]]
    block = head.rfind('&& ps_adj) {')
    assert block > head.rfind('// ---------------- adjoint') and head[block:].count('{') - head[block:].count('}') == 2
    assert head.rstrip().endswith('if (e == hipSuccess && ps->grad_shifts) {')
    assert 'st, ps->part, batch, M * ncg, ps->index, ps->grad_shifts);' in body[launches[0]:body.index(';', launches[0]) + 1]
    assert launches[0] < body.index('hipLaunchKernelGGL(st_dd_reduce_kernel') < launches[1]
    build = open(os.path.join(CSRC, 'build.py')).read()
    assert "'adm_ms_probeshift.hip'" in build


def test_resource_usage_is_recorded_without_scratch():
    text = open(os.path.join(ROOT, 'profiles', 'probe_shift', 'resource_usage.txt')).read()
    names = re.findall(r'Function Name: (\S+)', text)
    for k in ('ps_colfft_kernel', 'ps_col_kernelILb0', 'ps_col_kernelILb1', 'st_shift_reduce_kernel'):
        assert any(k in n for n in names), k
    scratch = re.findall(r'ScratchSize \[bytes/lane\]: (\d+)', text)
    assert len(scratch) == len(names) == 4 and set(scratch) == {'0'}
