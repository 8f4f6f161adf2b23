"""CPU-only bookkeeping of adm_ms_exitshift.hip: every __global__ kernel in it is named by a GPU test, every instantiation of its
template is launched, and the helpers it restates from adm_ms_streamed.hip (the column-launch geometry, the column load / store,
the column transform, fftfreq) are the originals word for word up to their prefix."""
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, 'adorym_amd', 'csrc')

# kernel: (test module, tests whose docstrings name it)
KERNELS = {
    'es_col_conv_kernel<false>': ('test_gpu_prj_offset', ['test_kernels_vs_reference', 'test_geometries_vs_restatement']),
    'es_col_conv_kernel<true>': ('test_gpu_prj_offset', ['test_kernels_vs_reference', 'test_geometries_vs_restatement']),
    'es_reduce_kernel': ('test_gpu_prj_offset', ['test_kernels_vs_reference', 'test_geometries_vs_restatement']),
}

# restated helper -> the original in adm_ms_streamed.hip
RESTATED = {
    'es_cw': 'st_cw', 'es_col_fft': 'st_col_fft', 'es_col_ctx': 'st_col_ctx', 'es_col_load': 'st_col_load', 'es_col_store': 'st_col_store',
    'es_freq_index': 'st_freq_index', 'es_col_threads': 'st_col_threads',
}


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
    es = _read('adm_ms_exitshift.hip')
    found = set()
    for m in re.finditer(r'(template\s*<\s*bool\s+\w+\s*>\s*)?__global__\s+(?:__launch_bounds__\([^)]*\)\s+)?void\s+(\w+)\s*\(', es):
        found |= {m.group(2) + '<false>', m.group(2) + '<true>'} if m.group(1) else {m.group(2)}
    assert len(re.findall(r'__global__', es)) == 2 and found == set(KERNELS), found ^ set(KERNELS)
    for k, (module, tests) in KERNELS.items():
        text = open(os.path.join(ROOT, 'tests', module + '.py')).read()
        for t in tests:
            m = re.search(r'^def %s\(.*?\n    """(.*?)"""' % t, text, re.M | re.S)
            assert m and k in m.group(1), (k, t)
    assert {v for v in re.findall(r'hipLaunchKernelGGL\(es_col_conv_kernel<(\w+)>', es)} == {'true', 'false'}
    assert len(re.findall(r'hipLaunchKernelGGL\(es_reduce_kernel\b', es)) == 1


def test_restated_helpers_equal_the_originals():
    es, st = _read('adm_ms_exitshift.hip'), _read('adm_ms_streamed.hip')
    back = lambda s: re.sub(r'\bes_', 'st_', re.sub(r'\bES_', 'ST_', s))
    for mine, orig in RESTATED.items():
        assert back(_function(es, mine)) == _function(st, orig), mine
    val = lambda src, n: re.search(r'constexpr\s+int\s+%s\s*=\s*([^;]+);' % n, src).group(1).strip()
    assert val(es, 'ES_COL_NT') == val(st, 'ST_COL_NT')
    # the launcher sizes the workgroup and its LDS as ms_streamed_launch does
    assert '((size_t)Py * cw + Py) * sizeof(float2)' in es and 'const size_t clds = ((size_t)Py * st_cw(Py) + Py) * sizeof(float2);' in st


def test_the_streamed_launch_routes_the_detector_step():
    """ms_streamed_launch hands the detector step's column launches (and nothing else) to the new translation unit, and the
    reduction runs once, after the adjoint sweep."""
    st = _read('adm_ms_streamed.hip')
    assert len(re.findall(r'ms_exitshift_col_launch\(', st)) == 1 and len(re.findall(r'ms_exitshift_reduce_launch\(', st)) == 1
    assert len(re.findall(r'det_col\((?:true|false)\)', st)) == 2
    build = open(os.path.join(CSRC, 'build.py')).read()
    assert "'adm_ms_exitshift.hip'" in build
