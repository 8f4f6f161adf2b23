"""CPU-only bookkeeping of adm_ms_probeshift.hip: every __global__ kernel in it is named by a GPU test, every instantiation of its
template is launched, the helpers it restates from adm_ms_streamed.hip (the column-launch geometry, the column load / store, the
column transform, fftfreq) are the originals word for word up to their prefix, its reduction is the exit-shift file's, and ms_streamed_launch reaches it only through a plan's third optional pointer."""
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, 'adorym_amd', 'csrc')

# kernel: (test module, tests whose docstrings name it)
KERNELS = {
    'ps_colfft_kernel': ('test_gpu_streamed_probe_shift', ['test_geometries_vs_oracle']),
    'ps_col_kernel<false>': ('test_gpu_streamed_probe_shift', ['test_geometries_vs_oracle']),
    'ps_col_kernel<true>': ('test_gpu_streamed_probe_shift', ['test_geometries_vs_oracle']),
    'ps_reduce_kernel': ('test_gpu_streamed_probe_shift', ['test_geometries_vs_oracle']),
}

# restated helper -> the original in adm_ms_streamed.hip
RESTATED = {
    'ps_cw': 'st_cw', 'ps_col_fft': 'st_col_fft', 'ps_col_ctx': 'st_col_ctx', 'ps_col_load': 'st_col_load', 'ps_col_store': 'st_col_store',
    'ps_freq_index': 'st_freq_index', 'ps_col_threads': 'st_col_threads',
}
# ... -> the original in adm_ms_exitshift.hip
RESTATED_ES = {'ps_freq': 'es_freq', 'ps_reduce_kernel': 'es_reduce_kernel'}


def _read(name):
    with open(os.path.join(CSRC, name)) as f:
        return f.read()


def _function(src, name):
    """The text of function ``name`` from its name to the closing brace of its body, whitespace squeezed."""
    m = re.search(r'\b%s\s*\(' % name, src)
    assert m, name
    i = src.index('{', m.end())
    depth, j = 1, i + 1
    while depth:
        depth += {'{': 1, '}': -1}.get(src[j], 0)
        j += 1
    return re.sub(r'\s+', ' ', src[m.start():j])


def test_every_kernel_is_named_by_a_gpu_test():
    ps = _read('adm_ms_probeshift.hip')
    found = set()
    for m in re.finditer(r'(template\s*<\s*bool\s+\w+\s*>\s*)?__global__\s+(?:__launch_bounds__\([^)]*\)\s+)?void\s+(\w+)\s*\(', ps):
        found |= {m.group(2) + '<false>', m.group(2) + '<true>'} if m.group(1) else {m.group(2)}
    assert len(re.findall(r'__global__', ps)) == 3 and found == set(KERNELS), found ^ set(KERNELS)
    for k, (module, tests) in KERNELS.items():
        text = open(os.path.join(ROOT, 'tests', module + '.py')).read()
        for t in tests:
            m = re.search(r'^def %s\(.*?\n    """(.*?)"""' % t, text, re.M | re.S)
            assert m and k in m.group(1), (k, t)
    assert {v for v in re.findall(r'hipLaunchKernelGGL\(ps_col_kernel<(\w+)>', ps)} == {'true', 'false'}
    assert len(re.findall(r'hipLaunchKernelGGL\(ps_colfft_kernel\b', ps)) == 1
    assert len(re.findall(r'hipLaunchKernelGGL\(ps_reduce_kernel\b', ps)) == 1
    # no atomics in the file
    assert not re.search(r'\batomic\w*\s*\(', ps)


def test_restated_helpers_equal_the_originals():
    ps, st, es = _read('adm_ms_probeshift.hip'), _read('adm_ms_streamed.hip'), _read('adm_ms_exitshift.hip')
    to = lambda s, p, P: re.sub(r'\bps_', p, re.sub(r'\bPS_', P, s))
    for mine, orig in RESTATED.items():
        assert to(_function(ps, mine), 'st_', 'ST_') == _function(st, orig), mine
    for mine, orig in RESTATED_ES.items():
        assert to(_function(ps, mine), 'es_', 'ES_') == _function(es, orig), mine
    val = lambda src, n: re.search(r'constexpr\s+int\s+%s\s*=\s*([^;]+);' % n, src).group(1).strip()
    assert val(ps, 'PS_COL_NT') == val(st, 'ST_COL_NT')
    # the launchers size the workgroup and its LDS as ms_streamed_launch does
    assert len(re.findall(re.escape('((size_t)Py * cw + Py) * sizeof(float2)'), ps)) == 2
    assert 'const size_t clds = ((size_t)Py * st_cw(Py) + Py) * sizeof(float2);' in st
    assert len(re.findall(r'ps_col_threads\(Py\)', ps)) == 2


def test_the_streamed_launch_reaches_the_file_only_with_the_third_pointer():
    """Every call into the new translation unit, the extra row launches and every changed argument of the sweep's row launches
    hang on ``ps``: with ps == nullptr the body issues the launches it always did."""
    st = _read('adm_ms_streamed.hip')
    body = _function(st, 'ms_streamed_launch')
    assert 'const StProbeShiftLaunch* ps)' in body
    assert len(re.findall(r'ms_probeshift_spectrum_launch\(', body)) == 1 and len(re.findall(r'ms_probeshift_col_launch\(', body)) == 2
    assert len(re.findall(r'ms_probeshift_reduce_launch\(', body)) == 1
    # the sweep's launches: today's arguments when ps is null
    assert 'e = row(s, 1, s > 0 || ps ? 2 : 0, s < S - 1 ? 1 : det_row, s == 0 && !ps, 0);' in body
    assert 'const bool ps_adj = ps && (p.grad_probe || ps->grad_shifts);' in body
    assert 'e = row(s, 2, s == S - 1 ? adj_row : 2, s > 0 || ps_adj ? 1 : 0, 0, s == 0 && !ps_adj);' in body
    # everything else that names the new unit sits inside `if (ps)` / `if (... && ps_adj)`
    for m in re.finditer(r'ms_probeshift_\w+\(', body):
        head = body[:m.start()]
        assert head.rfind('if (ps) {') > head.rfind('// ---------------- forward') or head.rfind('&& ps_adj) {') > head.rfind('// ---------------- adjoint'), m.group(0)
    build = open(os.path.join(CSRC, 'build.py')).read()
    assert "'adm_ms_probeshift.hip'" in build


def test_resource_usage_is_recorded_without_scratch():
    text = open(os.path.join(ROOT, 'profiles', 'probe_shift', 'resource_usage.txt')).read()
    names = re.findall(r'Function Name: (\S+)', text)
    for k in ('ps_colfft_kernel', 'ps_col_kernelILb0', 'ps_col_kernelILb1', 'ps_reduce_kernel'):
        assert any(k in n for n in names), k
    scratch = re.findall(r'ScratchSize \[bytes/lane\]: (\d+)', text)
    assert len(scratch) == len(names) == 4 and set(scratch) == {'0'}
