#!/usr/bin/env python3
"""Build libadm.so (gfx950) in-tree with hipcc.  Usage: python adorym_amd/csrc/build.py [--force] [--safe-sync]"""
import os
import subprocess
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
PKG = os.path.dirname(HERE)
OUT = os.path.join(PKG, 'libadm.so')
SRCS = ['adm_api.hip', 'adm_rotate.hip', 'adm_overlap_add.hip', 'adm_regularize.hip', 'adm_optimize.hip', 'adm_cg.hip', 'adm_kappa_tie.hip', 'adm_multislice.hip', 'adm_ms_generic.hip', 'adm_ms_streamed.hip', 'adm_ms_exitshift.hip', 'adm_ms_probeshift.hip', 'adm_ms_multidist.hip', 'adm_rotcsr.hip', 'adm_project.hip', 'adm_rotate_project.hip', 'adm_comm.hip', 'adm_p2p.hip', 'adm_holo.hip', 'adm_holo_ctf.hip', 'adm_ctf_dist.hip', 'adm_register.hip', 'adm_ctf_invert.hip']
HDRS = ['adm_common.h', 'adm_host.h', 'adm_fft.h', 'adm_ms_math.h', 'adm_ms_gen.h', 'adm_ms_col.h', 'adm_optim.h', 'adm_block_sum.h', 'adm_rot_bilin.h', 'adm_line_fft.h', 'adm_line_host.h', 'adm_ctf_group.h', os.path.join('..', '..', 'include', 'adm.h')]


# Flags that ONE translation unit alone is compiled with (every other file keeps the common line below).
# adm_multislice.hip: the backend's load/store merging pass is off, so the LDS field exchanges of ld_line / st_line stay single
# ds_read_b64 / ds_write_b64 -- the forms the field layouts of adm_ms_math.h were searched for (a merged ds_read2_b64 costs
# twice two single reads and is banked in 16-lane groups over 32 banks).  1.76 -> 1.69 ms per launch of 32 positions, same
# registers, same bits; tools/isa_lds_forms.py prints what is issued.
# (-Xclang reaches the host pass of the file too, which answers "not a recognized feature for this target (ignoring feature)".)
FILE_FLAGS = {'adm_multislice.hip': ['-Xclang', '-target-feature', '-Xclang', '-load-store-opt']}


def _hipcc():
    for c in (os.environ.get('HIPCC'), '/opt/rocm/bin/hipcc', 'hipcc'):
        if c and (os.path.isabs(c) and os.path.exists(c) or not os.path.isabs(c)):
            return c
    raise RuntimeError('hipcc not found')


def compile_cmd(src, obj, flags=(), mode=('-c',)):
    """The hipcc line of one translation unit (tools/isa_lds_forms.py uses it with mode = --cuda-device-only -S)."""
    return [_hipcc(), '--offload-arch=gfx950', '-O3', '-std=c++17', '-fPIC', '-munsafe-fp-atomics',
            '-Wno-unused-result', '-fno-slp-vectorize'] + list(mode) + [os.path.join(HERE, src), '-o', obj] + list(flags)


def needs_build():
    if not os.path.exists(OUT):
        return True
    t = os.path.getmtime(OUT)
    return any(os.path.getmtime(os.path.join(HERE, f)) > t for f in SRCS + HDRS + ['build.py'])


def build(force=False, extra=(), out=None, tag='', only=None, file_flags=None):
    """only = FILE: `extra` and `tag` apply to that translation unit alone, the others are the default build's objects.
    file_flags: stands in for FILE_FLAGS (an empty dict builds every file with the common line)."""
    out = out or OUT
    file_flags = FILE_FLAGS if file_flags is None else file_flags
    if not force and out == OUT and not needs_build():
        return OUT
    objs, cmds = [], []
    hdr_t = max(os.path.getmtime(os.path.join(HERE, f)) for f in HDRS + ['build.py'])
    for s in SRCS:
        mine = only is None or s == only           # does this file take the variant's tag and flags?
        o = os.path.join(HERE, s.replace('.hip', (tag if mine else '') + '.o'))
        objs.append(o)
        fresh = os.path.exists(o) and os.path.getmtime(o) > max(hdr_t, os.path.getmtime(os.path.join(HERE, s)))
        if fresh and (not mine or (not force and not extra)):
            continue          # object is newer than its source and every header
        cmds.append(compile_cmd(s, o, (list(extra) if mine else []) + list((file_flags if mine else FILE_FLAGS).get(s, []))))
    # the translation units are independent: compile them side by side (adm_multislice.hip alone takes ~75 s)
    procs = [subprocess.Popen(c) for c in cmds]
    failed = [c for c, p_ in zip(cmds, procs) if p_.wait() != 0]
    if failed:
        raise subprocess.CalledProcessError(1, failed[0])
    subprocess.check_call([_hipcc(), '--offload-arch=gfx950', '-shared', '-fPIC', '-o', out] + objs + ['-ldl'])
    return out


if __name__ == '__main__':
    # experiment builds: python build.py --variant NAME [--only FILE.hip] [--no-file-flags] -DFLAG ...  -> adorym_amd/libadm_NAME.so
    # --only FILE.hip: the flags go to that translation unit alone, every other object is the default build's.
    # --no-file-flags: without FILE_FLAGS (the build as it was before a per-file flag shipped).
    if '--variant' in sys.argv:
        name = sys.argv[sys.argv.index('--variant') + 1]
        only = sys.argv[sys.argv.index('--only') + 1] if '--only' in sys.argv else None
        flags = [a for i_, a in enumerate(sys.argv[1:]) if a.startswith('-D') or a.startswith('-m') or a.startswith('-f') or a.startswith('-amdgpu')
                 or a == '-Xclang' or sys.argv[i_] in ('-mllvm', '-Xclang')]          # (the value that follows -mllvm / -Xclang)
        print(build(force=True, extra=flags, out=os.path.join(PKG, 'libadm_%s.so' % name), tag='_' + name, only=only,
                    file_flags={} if '--no-file-flags' in sys.argv else None))
    else:
        extra = ['-DADM_SAFE_SYNC'] if '--safe-sync' in sys.argv else []
        print(build(force='--force' in sys.argv or bool(extra), extra=extra))
