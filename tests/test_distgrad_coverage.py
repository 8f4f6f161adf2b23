"""CPU-only bookkeeping of adm_ms_distgrad.hip (the distances of the detector fan-out as parameters on the device): the two entry
points are declared, exported and bound; every __global__ kernel in the file is named by a GPU test; the file is built and
documented; its recorded resource usage shows no scratch; and with no gradient requested ms_streamed_launch does not reach the
file -- read from the sources, as tests/test_multidist3d_coverage.py does."""
import ctypes
import os
import re

from tests.test_kernel_matrix_coverage import _function_body

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, 'adorym_amd', 'csrc')

# kernel: (test module, tests whose docstrings name it)
KERNELS = {
    'dg_table_kernel': ('test_gpu_multidist3d_dist', ['test_kernels_vs_reference', 'test_changed_distances_rebuild_the_table']),
    'dg_fanout_kernel': ('test_gpu_multidist3d_dist', ['test_kernels_vs_reference', 'test_geometries_vs_restatement']),
    'dg_fanin_kernel': ('test_gpu_multidist3d_dist', ['test_kernels_vs_reference', 'test_geometries_vs_restatement']),
    'dg_reduce_kernel': ('test_gpu_multidist3d_dist', ['test_kernels_vs_reference', 'test_geometries_vs_restatement']),
}


def _read(name):
    with open(os.path.join(CSRC, name)) as f:
        return f.read()


def test_the_entry_points_are_declared_exported_and_bound():
    import __graft_entry__ as g
    g.build()
    from adorym_amd import _lib
    hdr = re.sub(r'/\*.*?\*/', '', open(os.path.join(ROOT, 'include', 'adm.h')).read(), flags=re.S)
    assert re.search(r'\bint\s+adm_plan_set_fanout_distances\s*\(\s*adm_plan\*\s*plan,\s*const float\*\s*dists_cm_dev,\s*int\s+n,\s*double\s+lambda_nm,'
                     r'\s*double\s+voxel_nm_y,\s*double\s+voxel_nm_x\)', hdr)
    assert re.search(r'\bint\s+adm_multislice_fwd_adj_fanout_dist\s*\([^)]*size_t\s+workspace_bytes,\s*float\*\s*grad_dists_dev\)', hdr)
    lib = ctypes.CDLL(_lib.LIB_PATH)
    for fn in ('adm_plan_set_fanout_distances', 'adm_multislice_fwd_adj_fanout_dist'):
        assert hasattr(lib, fn), fn
    restype, argtypes = _lib.SIGNATURES['adm_plan_set_fanout_distances']
    assert restype is ctypes.c_int and len(argtypes) == 6 and argtypes[2] is ctypes.c_int and argtypes[3] is ctypes.c_double
    restype, argtypes = _lib.SIGNATURES['adm_multislice_fwd_adj_fanout_dist']
    assert restype is ctypes.c_int and argtypes == _lib.SIGNATURES['adm_multislice_fwd_adj_sparse'][1]
    assert 'adm_plan_set_fanout_distances' in open(os.path.join(ROOT, 'INTEGRATION.md')).read()
    # the same limits and refusals as the host-table setter
    body = _function_body(_read('adm_api.hip'), r'extern "C" int adm_plan_set_fanout_distances\s*\(')
    assert 'if (n < 1 || n > 64)' in body
    for what in ('!plan->streamed', 'ADM_DET_FRESNEL', 'plan->exit_shift', 'plan->probe_shift', 'plan->n_zpos > 0', 'fan_dists_dirty = true'):
        assert what in body, what


def test_every_kernel_is_named_by_a_gpu_test():
    dg = _read('adm_ms_distgrad.hip')
    found = set()
    for m in re.finditer(r'(template\s*<[^>]*>\s*)?__global__\s+(?:__launch_bounds__\([^)]*\)\s+)?void\s+(\w+)\s*\(', dg):
        assert not m.group(1), 'a template: list its instantiations in KERNELS and check that each is launched'
        found.add(m.group(2))
    assert len(re.findall(r'__global__', dg)) == len(KERNELS) and found == set(KERNELS), found ^ set(KERNELS)
    for k, (module, tests) in KERNELS.items():
        text = open(os.path.join(ROOT, 'tests', module + '.py')).read()
        for t in tests:
            m = re.search(r'^def %s\(.*?\n    """(.*?)"""' % t, text, re.M | re.S)
            assert m and k in m.group(1), (k, t)
        assert len(re.findall(r'hipLaunchKernelGGL\(%s\b' % k, dg)) == 1, k
    code = re.sub(r'//.*', '', dg)
    assert not re.search(r'\batomic\w*\s*\(', code)              # fixed orders of all sums
    assert '#include "adm_ms_col.h"' in dg and 'st_col_geom(' in dg and 'st_col_raise_lds(' in dg and 'st_block_sum_f64(' in dg
    for k in ('dg_fanout_kernel', 'dg_fanin_kernel'):
        assert re.search(r'__launch_bounds__\(ST_COL_NT\)\s+void\s+%s\b' % k, dg), k


def test_without_a_request_the_streamed_launch_does_not_reach_the_file():
    """The only ways into adm_ms_distgrad.hip from a launch: the first line of the two fan-out launchers and the sum launch at the
    end of ms_streamed_launch, each behind StFanoutLaunch::grad_dists; and that pointer is set in one place, behind the caller's
    buffer and want_grad."""
    md, st, api = _read('adm_ms_multidist.hip'), _read('adm_ms_streamed.hip'), _read('adm_api.hip')
    calls = re.findall(r'^.*\bms_distgrad_\w+\(.*$', md + st, re.M)
    assert len(calls) == 3, calls
    assert sum('if (fo.grad_dists) return ms_distgrad_fanout_launch(p, batch, fld, fo, st);' in c for c in calls) == 1
    assert sum('if (fo.grad_dists) return ms_distgrad_fanin_launch(p, batch, fld, fo, st);' in c for c in calls) == 1
    assert sum('if (e == hipSuccess && fo && fo->grad_dists) e = ms_distgrad_sum_launch(p, batch, *fo, st);' in c for c in calls) == 1
    assert 'float* grad_dists = nullptr;' in _read('adm_host.h')
    sets = re.findall(r'^.*\bgrad_dists\s*=[^=].*$', api, re.M)
    assert len(sets) == 1 and 'fo.grad_dists = grad_dists;' in sets[0], sets
    body = _function_body(api, r'static int streamed_launch\s*\(')
    assert re.search(r'if \(grad_dists && p\.want_grad\) \{\s*fo\.grad_dists = grad_dists;', body)
    # the table is rebuilt only behind the dirty flag
    assert re.search(r'if \(plan->fan_dists_dirty\) \{[^}]*ms_distgrad_table_launch\(', body, re.S)
    assert len(re.findall(r'ms_distgrad_table_launch\(', api)) == 1


def test_the_workspace_sections_exist_only_on_a_refining_plan():
    api = _read('adm_api.hip')
    body = _function_body(api, r'WsLayout\s+ws_layout\s*\(')
    assert 'const bool refine = fan && plan->fan_dists_dev;' in body
    assert 'w.fan_keep = take(refine ? B * M * fld : 0);' in body
    assert 'w.fan_part = take(refine ? (size_t)plan->n_fan * B * M * cg * sizeof(double) : 0);' in body
    assert body.index('w.fan_pos = take(') < body.index('w.fan_keep = take(') < body.index('w.fan_part = take(') < body.index('w.total = at;')


def test_the_file_is_built_and_documented():
    build = _read('build.py')
    assert "'adm_ms_distgrad.hip'" in re.search(r'^SRCS = \[.*\]$', build, re.M).group(0)
    for doc in ('README.md', 'DESIGN.md'):
        text = open(os.path.join(ROOT, doc)).read()
        assert 'adm_ms_distgrad.hip' in text and 'fanout_free_prop' in text, doc
    assert os.path.exists(os.path.join(ROOT, 'tools', 'bench_multidist3d_dist.py'))


def test_resource_usage_is_recorded_without_scratch():
    text = open(os.path.join(ROOT, 'profiles', 'distgrad', 'resource_usage.txt')).read()
    names = re.findall(r'Function Name: (\S+)', text)
    for k in KERNELS:
        assert any(k in n for n in names), k
    scratch = re.findall(r'ScratchSize \[bytes/lane\]: (\d+)', text)
    assert len(scratch) == len(names) == len(KERNELS) and set(scratch) == {'0'}
    assert len(re.findall(r'VGPRs: \d+', text)) >= len(KERNELS)
