"""The layout of adorym_amd/csrc: every source and header there is one the build knows (a forgotten file fails here and not at link
time on a GPU machine), the pieces the translation units share are defined once, the element-wise kernels sum a workgroup through
block_sum_f32 only, and every function of the C ABI has exactly one definition."""
import os
import re

from adorym_amd.csrc import build

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, 'adorym_amd', 'csrc')


def _sources():
    out = {}
    for name in sorted(os.listdir(CSRC)):
        if name.endswith(('.hip', '.h')):
            with open(os.path.join(CSRC, name)) as f:
                out[name] = f.read()
    return out


def test_the_build_lists_every_file():
    names = set(_sources())
    assert {n for n in names if n.endswith('.hip')} == set(build.SRCS) and len(set(build.SRCS)) == len(build.SRCS)
    hdrs = [os.path.basename(h) for h in build.HDRS]
    assert {n for n in names if n.endswith('.h')} == set(hdrs) - {'adm.h'} and len(set(hdrs)) == len(hdrs)
    assert 'adm.h' in hdrs and os.path.exists(os.path.join(ROOT, 'include', 'adm.h'))
    assert not os.path.exists(os.path.join(CSRC, 'adm_object.hip'))


def test_shared_pieces_are_defined_once():
    """A definition: the name, its parameter list and an opening brace (a call ends in ';' or sits inside an expression)."""
    src = _sources()
    for name in ('stream_grid', 'block_sum_f32', 'reg_stencil', 'reg_rows', 'ri_stats_launch', 'reg_threads'):
        found = [(f, m.group(0)) for f, text in src.items() for m in re.finditer(r'^[\w \t:*&<>]*\b%s\s*\([^;{}]*\)\s*\{' % name, text, re.M)]
        assert len(found) == 1, (name, found)
    assert not any(re.search(r'\bgrid_for\b', text) for text in src.values())


def test_the_elementwise_kernels_do_not_spell_out_the_shuffle_tree():
    src = _sources()
    for name in ('adm_regularize.hip', 'adm_optimize.hip'):
        assert src[name].count('__shfl_down') == 0, name
        assert 'block_sum_f32(' in src[name], name
    assert len(re.findall(r'__shfl_down\s*\(', src['adm_block_sum.h'])) == 1


def test_every_abi_function_is_defined_in_one_file():
    with open(os.path.join(ROOT, 'include', 'adm.h')) as f:
        header = re.sub(r'/\*.*?\*/|//[^\n]*', '', f.read(), flags=re.S)
    declared = set(re.findall(r'\b(adm_\w+)\s*\(', header))
    assert len(declared) > 80, len(declared)
    src = {n: t for n, t in _sources().items() if n.endswith('.hip')}
    defined = {}
    for name, text in src.items():
        for fn in re.findall(r'^extern "C"\s+[\w \t*]+?\b(adm_\w+)\s*\([^;{}]*\)\s*\{', text, re.M):
            defined.setdefault(fn, []).append(name)
    for fn in sorted(declared):
        assert len(defined.get(fn, [])) == 1, (fn, defined.get(fn))
