#!/usr/bin/env python3
"""Instruction forms of every kernel of one translation unit, from its gfx950 assembly.  CPU only (cross-compiles).

    python tools/isa_lds_forms.py adorym_amd/csrc/adm_multislice.hip [--match SUBSTR] [--totals] [--no-file-flags] [extra hipcc flags ...]

Compiles the file with build.py's own line (its per-file flags included, unless --no-file-flags) plus
`--cuda-device-only -S` and prints, one line per kernel instantiation (--totals: one line per file): the DS read / write forms, the global loads / stores by
width, v_pk_*, s_nop, s_waitcnt, VGPRs, scratch bytes and spills.  `--asm FILE` reads an assembly file instead.
The LDS cost model (tools/lds/lds_layout_search.c) prices ds_read_b64 and ds_read2_b64 differently, so what the backend
merged is part of the kernel's cost: DESIGN.md section 4 and appendix round 9.
"""
import collections
import os
import re
import shutil
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, 'adorym_amd', 'csrc'))
import build as B  # noqa: E402

COLS = ['ds_read_b64', 'ds_read2_b64', 'ds_read_other', 'ds_write_b64', 'ds_write2_b64', 'ds_write_other',
        'global_load_dword', 'global_load_dwordx2', 'global_load_dwordx4', 'global_load_other',
        'global_store_dword', 'global_store_dwordx2', 'global_store_dwordx4', 'global_store_other',
        'v_pk', 's_nop', 's_waitcnt']


def classify(op):
    for fam in ('ds_read', 'ds_write', 'global_load', 'global_store'):
        if op.startswith(fam):
            return op if op in COLS else fam + '_other'
    if op.startswith('v_pk_'):
        return 'v_pk'
    return op if op in ('s_nop', 's_waitcnt') else None


def demangle(names):
    filt = shutil.which('llvm-cxxfilt') or shutil.which('c++filt')
    try:
        if not filt:
            raise OSError('no demangler')
        out = subprocess.run([filt], input='\n'.join(names), capture_output=True, text=True, check=True).stdout.split('\n')
        return dict(zip(names, out))
    except (OSError, subprocess.CalledProcessError):
        return {n: n for n in names}


def parse(text):
    """{kernel symbol: Counter of COLS + vgpr / scratch / spill fields}"""
    kernels = collections.OrderedDict()
    syms = re.findall(r'^\s*\.amdhsa_kernel\s+(\S+)', text, re.M)
    for sym in syms:
        body = re.search(r'^%s:.*?^\.Lfunc_end\d+:' % re.escape(sym), text, re.M | re.S)
        c = collections.Counter()
        for line in (body.group(0).split('\n')[1:] if body else []):
            tok = line.split(';')[0].split()
            if not tok or tok[0].startswith('.') or tok[0].endswith(':'):
                continue
            k = classify(tok[0])
            if k:
                c[k] += 1
        kernels[sym] = c
    # code-object metadata: one "  - " entry per kernel
    meta = text[text.find('amdhsa.kernels:'):]
    for entry in re.split(r'^  - ', meta, flags=re.M)[1:]:
        name = re.search(r'^\s*\.name:\s*(\S+)', entry, re.M)
        if not name or name.group(1) not in kernels:
            continue
        for key, field in (('vgpr', 'vgpr_count'), ('scratch', 'private_segment_fixed_size'),
                           ('vgpr_spill', 'vgpr_spill_count'), ('sgpr_spill', 'sgpr_spill_count')):
            m = re.search(r'^\s*\.%s:\s*(\d+)' % field, entry, re.M)
            kernels[name.group(1)][key] = int(m.group(1)) if m else -1
    return kernels


def assembly(src, flags, file_flags=True):
    name = os.path.basename(src)
    with tempfile.TemporaryDirectory() as d:
        out = os.path.join(d, 'k.s')
        ff = list(B.FILE_FLAGS.get(name, [])) if file_flags else []
        subprocess.check_call(B.compile_cmd(name, out, list(flags) + ff, mode=('--cuda-device-only', '-S')))
        return open(out).read(), ff


HEAD = ('# columns: ds_read b64/read2_b64/other | ds_write b64/write2_b64/other | global_load x1/x2/x4/other | global_store x1/x2/x4/other | '
        'v_pk_* s_nop s_waitcnt | VGPR scratch-bytes spills(vgpr+sgpr)')


def line(c):
    return '%d/%d/%d | %d/%d/%d | %d/%d/%d/%d | %d/%d/%d/%d | %d %d %d | %d %d %d' % (
        c['ds_read_b64'], c['ds_read2_b64'], c['ds_read_other'], c['ds_write_b64'], c['ds_write2_b64'], c['ds_write_other'],
        c['global_load_dword'], c['global_load_dwordx2'], c['global_load_dwordx4'], c['global_load_other'],
        c['global_store_dword'], c['global_store_dwordx2'], c['global_store_dwordx4'], c['global_store_other'],
        c['v_pk'], c['s_nop'], c['s_waitcnt'], c['vgpr'], c['scratch'], c['vgpr_spill'] + c['sgpr_spill'])


def report(kernels, match=None, out=sys.stdout, totals=False):
    """One line per kernel instantiation; totals: one line for the whole file (sums; VGPR = the largest)."""
    if totals:
        t = collections.Counter()
        for c in kernels.values():
            for k, v in c.items():
                t[k] = max(t[k], v) if k == 'vgpr' else t[k] + v
        out.write('%d kernels: %s\n' % (len(kernels), line(t)))
        return
    names = demangle(list(kernels))
    for sym, c in kernels.items():
        dn = re.sub(r'\(.*$', '', re.sub(r'^void ', '', names[sym])).replace('adm::', '').replace(' ', '')
        if match and match not in dn:
            continue
        out.write('%s: %s\n' % (dn, line(c)))


def main(argv):
    args = list(argv)
    match = asm = None
    if '--match' in args:
        i = args.index('--match'); match = args[i + 1]; del args[i:i + 2]
    if '--asm' in args:
        i = args.index('--asm'); asm = args[i + 1]; del args[i:i + 2]
    file_flags, totals = '--no-file-flags' not in args, '--totals' in args
    args = [a for a in args if a not in ('--no-file-flags', '--totals')]
    print(HEAD)
    if asm:
        print('# %s' % asm)
        report(parse(open(asm).read()), match, totals=totals)
        return
    srcs = [a for a in args if a.endswith('.hip')]
    flags = [a for a in args if not a.endswith('.hip')]
    for src in srcs:
        text, ff = assembly(src, flags, file_flags)
        print('# %s  flags beyond the common line: %s' % (os.path.basename(src), ' '.join(flags + ff) or '(none)'))
        report(parse(text), match, totals=totals)
        sys.stdout.flush()


if __name__ == '__main__':
    main(sys.argv[1:])
