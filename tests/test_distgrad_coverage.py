"""CPU-only bookkeeping of the distance gradient of the detector fan-out (the distances as parameters on the device): the
instantiations md_fanout_kernel<true> / md_fanin_kernel<true> of adm_ms_multidist.hip and the table and reduce kernels they share
with sparse multislice (st_fresnel_table_kernel, st_dd_reduce_kernel of adm_ms_streamed.hip).  The two entry points are declared,
exported and bound; every kernel is named by a GPU test; the code is built and documented; its recorded resource usage shows no
scratch; and with no gradient requested ms_streamed_launch does not reach the gradient code -- read from the sources, as
tests/test_multidist3d_coverage.py does."""
import ctypes
import os
import re

from tests.test_kernel_matrix_coverage import _function_body

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, 'adorym_amd', 'csrc')

# kernel (templates: the instantiation): (source file, test module, tests whose docstrings name it)
KERNELS = {
    'st_fresnel_table_kernel': ('adm_ms_streamed.hip', 'test_gpu_multidist3d_dist', ['test_kernels_vs_reference', 'test_changed_distances_rebuild_the_table']),
    'md_fanout_kernel<true>': ('adm_ms_multidist.hip', 'test_gpu_multidist3d_dist', ['test_kernels_vs_reference', 'test_geometries_vs_restatement']),
    'md_fanin_kernel<true>': ('adm_ms_multidist.hip', 'test_gpu_multidist3d_dist', ['test_kernels_vs_reference', 'test_geometries_vs_restatement']),
    'st_dd_reduce_kernel': ('adm_ms_streamed.hip', 'test_gpu_multidist3d_dist', ['test_kernels_vs_reference', 'test_geometries_vs_restatement']),
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
    api = _read('adm_api.hip')
    body = _function_body(api, r'extern "C" int adm_plan_set_fanout_distances\s*\(')
    assert 'if (n < 1 || n > 64)' in body and 'fan_dists_dirty = true' in body
    # (both ask the one check of the exclusive plan options, as the fan-out, and that check and its table hold the refusals)
    host_setter = _function_body(api, r'extern "C" int adm_plan_set_detector_fanout\s*\(')
    for b, who, on in ((body, 'adm_plan_set_fanout_distances', 'true'), (host_setter, 'adm_plan_set_detector_fanout', 'n != 0')):
        assert 'if (const int rc = plan_option_check(plan, OPT_FANOUT, "%s", %s)) return rc;' % (who, on) in b, who
    check = _function_body(api, r'static int plan_option_check\s*\(')
    for what in ('!plan->streamed', 'opt == OPT_FANOUT && plan->d.det_mode != ADM_DET_FRESNEL', '&other != &me && other.on(plan)'):
        assert what in check, what
    table = api[api.index('PLAN_OPTIONS[] = {'):api.index('static int plan_option_check')]
    for what in ('return p->exit_shift;', 'return p->probe_shift;', 'return p->n_zpos > 0;', 'return p->n_fan > 0;'):
        assert what in table, what


def test_every_kernel_is_named_by_a_gpu_test():
    md, st = _read('adm_ms_multidist.hip'), _read('adm_ms_streamed.hip')
    assert not os.path.exists(os.path.join(CSRC, 'adm_ms_distgrad.hip'))
    # templates are listed by instantiation (tests/test_multidist3d_coverage.py holds the file to exactly these two templates)
    for k, (src, module, tests) in KERNELS.items():
        name, inst = re.match(r'(\w+)(<true>)?$', k).groups()
        head = re.search(r'(template\s*<[^>]*>\s*)?__global__\s+(?:__launch_bounds__\([^)]*\)\s+)?void\s+%s\s*\(' % name, _read(src))
        assert head and bool(head.group(1)) == bool(inst), k
        text = open(os.path.join(ROOT, 'tests', module + '.py')).read()
        for t in tests:
            m = re.search(r'^def %s\(.*?\n    """(.*?)"""' % t, text, re.M | re.S)
            assert m and k in m.group(1), (k, t)
    # each is launched exactly once for the distances: the instantiations by the launch line that picks them, the table by its
    # launcher, the reduce kernel by the one launch with gaps = 0
    for k in ('md_fanout_kernel', 'md_fanin_kernel'):
        assert len(re.findall(r'st_col_launch\(fo\.grad_dists \? %s<true> : %s<false>,' % (k, k), md)) == 1, k
        assert re.search(r'__launch_bounds__\(ST_COL_NT\)\s+void\s+%s\b' % k, md), k
    assert len(re.findall(r'hipLaunchKernelGGL\(st_fresnel_table_kernel\b', st)) == 1
    assert len(re.findall(r'hipLaunchKernelGGL\(st_dd_reduce_kernel, [^;]*, 0, fo->grad_dists\);', st)) == 1
    assert len(re.findall(r'hipLaunchKernelGGL\(st_dd_reduce_kernel\b', st)) == 2          # (the other: the gaps of a sparse plan)
    # fixed orders of all sums: no atomics in the fan-out's file nor in the two shared kernels
    assert not re.search(r'\batomic\w*\s*\(', re.sub(r'//.*', '', md))
    for k in ('st_fresnel_table_kernel', 'st_dd_reduce_kernel'):
        assert not re.search(r'\batomic\w*\s*\(', re.sub(r'//.*', '', _function_body(st, r'void\s+%s\s*\(' % k))), k
    assert '#include "adm_ms_col.h"' in md and 'st_col_geom(' in md and 'st_col_raise_lds_once(' in md and 'st_block_sum_f64(' in md


def test_without_a_request_the_streamed_launch_does_not_reach_the_gradient_code():
    """The only ways into the gradient code from a launch: the <true> instantiations in the launch line of the two fan-out launchers
    and the gaps = 0 reduce launch at the end of ms_streamed_launch, each behind StFanoutLaunch::grad_dists; and that pointer is set
    in one place, behind the caller's buffer and want_grad."""
    md, st, api = _read('adm_ms_multidist.hip'), _read('adm_ms_streamed.hip'), _read('adm_api.hip')
    # <true> is named where the LDS limit is raised and behind `fo.grad_dists ?`, nowhere else in the code
    code = re.sub(r'//.*', '', md)
    for k in ('md_fanout_kernel', 'md_fanin_kernel'):
        uses = [m.start() for m in re.finditer(r'%s<true>' % k, code)]
        assert len(uses) == 2, (k, uses)
        assert code[:uses[0]].rstrip().endswith('st_col_raise_lds_once(raised, %s<false>,' % k)
        assert code[:uses[1]].endswith('st_col_launch(fo.grad_dists ? ')
    body = _function_body(st, r'hipError_t\s+ms_streamed_launch\s*\(')
    assert re.search(r'if \(e == hipSuccess && fo && fo->grad_dists\) \{\s*hipLaunchKernelGGL\(st_dd_reduce_kernel, dim3\(1\), dim3\(256\), 0, st, '
                     r'fo->part, batch \* M \* ncg, fo->n, 0, fo->grad_dists\);', body)
    assert len(re.findall(r'\bgrad_dists\b', re.sub(r'//.*', '', md + st))) == 4          # (two launch lines, the condition, the argument)
    assert 'ms_distgrad_' not in md + st + api + _read('adm_host.h')
    assert 'float* grad_dists = nullptr;' in _read('adm_host.h')
    # (two assignments: the launch record's into the launch, and further down the entry point's caller's buffer into the record)
    sets = re.findall(r'^.*\bgrad_dists\s*=[^=].*$', api, re.M)
    assert len(sets) == 2 and 'fo.grad_dists = c.grad_dists;' in sets[0] and '.grad_dists = grad_dists_dev}' in sets[1], sets
    assert sets[1] in _function_body(api, r'extern "C" int adm_multislice_fwd_adj_fanout_dist\s*\(')
    body = _function_body(api, r'static int streamed_launch\s*\(')
    assert re.search(r'if \(c\.grad_dists && p\.want_grad\) \{\s*fo\.grad_dists = c\.grad_dists;', body)
    # the table is rebuilt only behind the dirty flag, by the launcher it shares with the sparse plan's gaps
    assert re.search(r'if \(plan->fan_dists_dirty\) \{[^}]*q\.gaps = 0;[^}]*ms_fresnel_table_launch\(q, plan->fan_dists_dev,', body, re.S)
    assert len(re.findall(r'ms_fresnel_table_launch\(q, plan->fan_dists_dev', api)) == 1 and len(re.findall(r'ms_fresnel_table_launch\(', api)) == 2


def test_the_workspace_sections_exist_only_on_a_refining_plan():
    api = _read('adm_api.hip')
    body = _function_body(api, r'WsLayout\s+ws_layout\s*\(')
    assert 'const bool refine = fan && plan->fan_dists_dev;' in body
    assert 'w.fan_keep = take(refine ? B * M * fld : 0);' in body
    assert 'w.fan_part = take(refine ? (size_t)plan->n_fan * B * M * cg * sizeof(double) : 0);' in body
    assert body.index('w.fan_pos = take(') < body.index('w.fan_keep = take(') < body.index('w.fan_part = take(') < body.index('w.total = at;')


def test_the_file_is_built_and_documented():
    build = _read('build.py')
    srcs = re.search(r'^SRCS = \[.*\]$', build, re.M).group(0)
    assert "'adm_ms_multidist.hip'" in srcs and "'adm_ms_streamed.hip'" in srcs and 'distgrad' not in srcs
    for doc in ('README.md', 'DESIGN.md'):
        text = open(os.path.join(ROOT, doc)).read()
        assert 'md_fanin_kernel<true>' in text and 'st_dd_reduce_kernel' in text and 'fanout_free_prop' in text, doc
    assert os.path.exists(os.path.join(ROOT, 'tools', 'bench_multidist3d_dist.py'))


def test_resource_usage_is_recorded_without_scratch():
    text = open(os.path.join(ROOT, 'profiles', 'distgrad', 'resource_usage.txt')).read()
    names = re.findall(r'Function Name: (\S+)', text)
    for k in ('st_fresnel_table_kernel', 'md_fanout_kernelILb1E', 'md_fanin_kernelILb1E', 'st_dd_reduce_kernel'):      # (<true> as the compiler names it)
        assert any(k in n for n in names), k
    scratch = re.findall(r'ScratchSize \[bytes/lane\]: (\d+)', text)
    assert len(scratch) == len(names) == len(KERNELS) and set(scratch) == {'0'}
    assert len(re.findall(r'VGPRs: \d+', text)) >= len(KERNELS)
