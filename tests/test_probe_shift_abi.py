"""CPU-only: the entry points of sub-pixel probe positions on streamed plans are declared in include/adm.h and bound in
adorym_amd/_lib.py with as many arguments as the header gives them, of the kinds the header gives them."""
import ctypes
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def header_arguments(name):
    """The argument declarations of ``name`` in include/adm.h (comments stripped), e.g. ['adm_plan* plan', 'int on']."""
    src = open(os.path.join(ROOT, 'include', 'adm.h')).read()
    src = re.sub(r'/\*.*?\*/', '', src, flags=re.S)
    m = re.search(r'\bint\s+%s\s*\(([^)]*)\)\s*;' % re.escape(name), src)
    assert m, '%s is not declared in include/adm.h' % name
    return [' '.join(a.split()) for a in m.group(1).split(',')]


def ctype_of(decl):
    if '*' in decl:
        return ctypes.c_void_p
    return {'int': ctypes.c_int, 'float': ctypes.c_float, 'size_t': ctypes.c_size_t}[decl.split()[0]]


def test_probe_shift_entry_points_are_declared_and_bound():
    from adorym_amd import _lib
    for name in ('adm_plan_set_probe_shift', 'adm_multislice_fwd_adj_probe_shift'):
        args = header_arguments(name)
        assert name in _lib.SIGNATURES, 'ctypes binding missing for %s' % name
        restype, argtypes = _lib.SIGNATURES[name]
        assert restype is ctypes.c_int
        assert len(argtypes) == len(args), (name, len(argtypes), args)
        for i, (decl, t) in enumerate(zip(args, argtypes)):
            assert ctypes.sizeof(t) == ctypes.sizeof(ctype_of(decl)) and (t is ctypes.c_void_p) == ('*' in decl), (name, i, decl, t)
    # the launch is adm_multislice_fwd_adj plus (shifts, index, grad_shifts), like the exit-shift launch
    plain, ps = header_arguments('adm_multislice_fwd_adj'), header_arguments('adm_multislice_fwd_adj_probe_shift')
    assert ps[:len(plain)] == plain
    assert ps[len(plain):] == ['const float* shifts', 'const int32_t* index', 'float* grad_shifts']
    assert _lib.SIGNATURES['adm_multislice_fwd_adj_probe_shift'] == _lib.SIGNATURES['adm_multislice_fwd_adj_exit_shift']
