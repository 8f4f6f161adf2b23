"""CPU-only bookkeeping of adm_register.hip (the affine registration of measured holograms for multi-distance holography of a 3-D
object): every __global__ kernel in the file is named by a GPU test; the four entry points agree between header, library and
ctypes table; the geometry cases of the GPU tests sit on both sides of the constants read from the source; the file is built and
documented, its recorded resource usage shows no scratch; and the multislice translation units were not touched by the change that
brought the file in."""
import ctypes
import os
import re
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, 'adorym_amd', 'csrc')

# kernel: (test module, tests whose docstrings name it)
KERNELS = {
    'reg_sample_kernel': ('test_gpu_multidist3d_affine', ['test_kernels_vs_reference', 'test_geometries_vs_restatement']),
    'reg_grad_kernel': ('test_gpu_multidist3d_affine', ['test_kernels_vs_reference', 'test_geometries_vs_restatement', 'test_identity_matrices']),
    'reg_reduce_kernel': ('test_gpu_multidist3d_affine', ['test_kernels_vs_reference', 'test_geometries_vs_restatement']),
}
ENTRY_POINTS = {
    'adm_register_create': r'\(\s*adm_ctx\*\s*ctx,\s*int\s+n_dists,\s*int\s+ny,\s*int\s+nx,\s*int\s+intensity,\s*adm_register\*\*\s*out\)',
    'adm_register_destroy': r'\(\s*adm_register\*\s*r\)',
    'adm_register_targets': r'\(\s*adm_register\*\s*r,\s*const float\*\s*data,\s*const float\*\s*affine,\s*float\*\s*target\)',
    'adm_register_grad': r'\(\s*adm_register\*\s*r,\s*const float\*\s*data,\s*const float\*\s*affine,\s*const float\*\s*pred,\s*float\s+grad_scale,'
                         r'\s*float\*\s*grad_affine\)',
}


def _read(name):
    with open(os.path.join(CSRC, name)) as f:
        return f.read()


def test_the_entry_points_are_declared_exported_and_bound():
    import __graft_entry__ as g
    g.build()
    from adorym_amd import _lib
    hdr = re.sub(r'/\*.*?\*/', '', open(os.path.join(ROOT, 'include', 'adm.h')).read(), flags=re.S)
    lib = ctypes.CDLL(_lib.LIB_PATH)
    doc = open(os.path.join(ROOT, 'INTEGRATION.md')).read()
    src = _read('adm_register.hip')
    for fn, sig in ENTRY_POINTS.items():
        assert re.search(r'\bint\s+%s\s*%s' % (fn, sig), hdr), fn
        assert re.search(r'extern "C" int %s\s*%s' % (fn, sig), src), fn
        assert hasattr(lib, fn) and fn in _lib.SIGNATURES and '`%s`' % fn in doc, fn
        assert _lib.SIGNATURES[fn][0] is ctypes.c_int
    VP, I, Fl = ctypes.c_void_p, ctypes.c_int, ctypes.c_float
    assert _lib.SIGNATURES['adm_register_create'][1][:5] == [VP, I, I, I, I]
    assert _lib.SIGNATURES['adm_register_destroy'][1] == [VP]
    assert _lib.SIGNATURES['adm_register_targets'][1] == [VP] * 4
    assert _lib.SIGNATURES['adm_register_grad'][1] == [VP, VP, VP, VP, Fl, VP]
    # the refusals name their entry point
    for what in ('"adm_register_create: null argument"', '"adm_register_create: field sizes must be in [2, 2048]"',
                 '"adm_register_create: n_dists must be in [1, 64]"', '"adm_register_targets: null argument"', '"adm_register_grad: null argument"'):
        assert what in src, what
    assert 'if (ny < 2 || ny > 2048 || nx < 2 || nx > 2048)' in src and 'if (n_dists < 1 || n_dists > 64)' in src


def test_every_kernel_is_named_by_a_gpu_test():
    src = _read('adm_register.hip')
    found = set()
    for m in re.finditer(r'(template\s*<[^>]*>\s*)?__global__\s+(?:__launch_bounds__\([^)]*\)\s+)?void\s+(\w+)\s*\(', src):
        assert not m.group(1), 'a template: list its instantiations in KERNELS and check that each is launched'
        found.add(m.group(2))
    assert len(re.findall(r'__global__', src)) == len(KERNELS) and found == set(KERNELS), found ^ set(KERNELS)
    for k, (module, tests) in KERNELS.items():
        text = open(os.path.join(ROOT, 'tests', module + '.py')).read()
        for t in tests:
            m = re.search(r'^def %s\(.*?\n    """(.*?)"""' % t, text, re.M | re.S)
            assert m and k in m.group(1), (k, t)
            assert re.search(r'@gpu\n(?:@pytest\.mark\.parametrize\(.*\)\n)?def %s\(' % t, text), (t, 'is not marked gpu')
        assert len(re.findall(r'hipLaunchKernelGGL\(adm::%s\b' % k, src)) == 1, k
    code = re.sub(r'//.*', '', src)
    assert not re.search(r'\batomic\w*\s*\(', code)              # fixed orders of all sums
    assert not re.search(r'\basm\b|__builtin_amdgcn', code)      # plain C++
    assert 'st_block_sum_f64(' in src and '#include "adm_ms_col.h"' in src
    # the coordinate arithmetic is adm_holo.hip's, statement for statement
    holo = _read('adm_holo.hip')
    for fn_h, fn_r in (('base_coord', 'reg_base_coord'), ('affine_coords', 'reg_affine_coords')):
        body = lambda text, fn: re.sub(r'\s+', ' ', re.search(r'__device__ __forceinline__ \w+ %s\([^\n]*\) \{\n(.*?)\n\}' % fn, text, re.S).group(1))
        assert body(holo, fn_h) == body(src, fn_r), fn_h
    assert '#pragma clang fp contract(off)' in re.search(r'void reg_affine_coords\(.*?\n\}', src, re.S).group(0)


def test_the_geometry_cases_sit_on_both_sides_of_the_constants():
    """Workgroup size and reduce stride are read from the source, not typed twice; the GPU test file's own assertion does the
    arithmetic on its table."""
    import sys
    sys.path.insert(0, os.path.join(ROOT, 'tests', 'golden'))
    from tests import test_gpu_multidist3d_affine as T
    src = _read('adm_register.hip')
    nt, stride = T.kernel_constant('REG_NT'), T.kernel_constant('REG_RED_NT')
    assert '__launch_bounds__(REG_NT)' in src and '__launch_bounds__(REG_RED_NT)' in src and 'i += REG_RED_NT' in src
    assert '(size_t)ny * nx + REG_NT - 1) / REG_NT' in src
    T.test_the_cases_sit_on_both_sides_of_the_constants()
    fields = [c[0] for c in T.REG_CASES.values()]
    assert (2, 2) in fields and (12, 20) in fields and (24, 20) in fields and (33, 70) in fields and (1025, 12) in fields
    blocks = sorted({-(-int(np.prod(f)) // nt) for f in fields})
    assert blocks[0] == 1 and stride - 1 in blocks and stride + 1 in blocks
    assert {c[3] for c in T.REG_CASES.values()} == {'magnitude', 'intensity'} and any(c[4] for c in T.REG_CASES.values())


def test_the_file_is_built_and_documented():
    build = _read('build.py')
    assert "'adm_register.hip'" in re.search(r'^SRCS = \[.*\]$', build, re.M).group(0)
    for doc in ('README.md', 'DESIGN.md'):
        text = open(os.path.join(ROOT, doc)).read()
        assert 'adm_register.hip' in text and 'fanout_prj_affine' in text, doc
    assert os.path.exists(os.path.join(ROOT, 'tools', 'bench_multidist3d_affine.py'))


def test_resource_usage_is_recorded_without_scratch():
    text = open(os.path.join(ROOT, 'profiles', 'multidist3d_affine', 'resource_usage.txt')).read()
    names = re.findall(r'Function Name: (\S+)', text)
    for k in KERNELS:
        assert any(k in n for n in names), k
    scratch = re.findall(r'ScratchSize \[bytes/lane\]: (\d+)', text)
    assert len(scratch) == len(names) == len(KERNELS) and set(scratch) == {'0'}
    assert len(re.findall(r'VGPRs: \d+', text)) >= len(KERNELS)


UNTOUCHED = ('adm_ms_streamed.hip', 'adm_ms_multidist.hip', 'adm_ms_distgrad.hip')


def _git(*args):
    return subprocess.run(('git', '-C', ROOT) + args, capture_output=True, timeout=60)


def test_the_multislice_translation_units_are_untouched():
    """The registration acts on the data, not on the wave: the change that brought adm_register.hip in left the streamed sweep, the
    fan-out and the distance-gradient kernels byte-identical to its parent commit (before that change is committed: to HEAD).
    Compared with `git show` in a checkout; skipped outside one."""
    if _git('rev-parse', '--is-inside-work-tree').returncode != 0:
        pytest.skip('not a git checkout')
    added = _git('log', '--diff-filter=A', '--format=%H', '--', 'adorym_amd/csrc/adm_register.hip').stdout.decode().split()
    if added:
        new, old = added[-1], added[-1] + '~'
    else:
        new, old = None, 'HEAD'
    if _git('rev-parse', '--verify', '--quiet', old + '^{commit}').returncode != 0:
        pytest.skip('the parent commit is not in this checkout (shallow clone)')
    for name in UNTOUCHED:
        path = 'adorym_amd/csrc/' + name
        before = _git('show', '%s:%s' % (old, path))
        assert before.returncode == 0, (name, before.stderr.decode())
        if new is None:
            with open(os.path.join(CSRC, name), 'rb') as f:
                after = f.read()
        else:
            after = _git('show', '%s:%s' % (new, path)).stdout
        assert before.stdout == after, name
