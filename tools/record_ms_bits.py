#!/usr/bin/env python3
"""Record (or compare) the digests of a bit-for-bit test module with the library ADM_LIB_PATH names.  Needs the GPU.

    ADM_LIB_PATH=adorym_amd/libadm_parent.so python tools/record_ms_bits.py --commit <hash of the commit that library was built from> --out FILE
    ADM_LIB_PATH=adorym_amd/libadm_X.so python tools/record_ms_bits.py --compare tests/golden/ms_lds_forms_bits.json
    ... --module test_gpu_streamed_col_bits      (the module under tests/ whose CASES, case_id, run_case and FIXTURE are used;
                                                  default test_gpu_ms_lds_forms_bits)

The fixture is recorded with the build BEFORE a change that must keep every bit (how the LDS exchanges are issued, where the
shared pieces of the column kernels are stated); --compare checks an experiment build against it without pytest (exit status 1 and
the differing cases if any bit differs).
"""
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tests'))
MODULE = sys.argv[sys.argv.index('--module') + 1] if '--module' in sys.argv else 'test_gpu_ms_lds_forms_bits'
T = __import__(MODULE)


def rocm_version():
    for f in ('/opt/rocm/.info/version', '/opt/rocm/.info/version-dev'):
        if os.path.exists(f):
            return open(f).read().strip()
    return 'unknown'


def main(argv):
    import adorym_amd as A
    ctx = A.Context(0)
    cases = [c if isinstance(c, tuple) else (c,) for c in T.CASES]
    digests = {T.case_id(*c): T.run_case(A, ctx, *c) for c in cases}
    ctx.close()
    if '--compare' in argv:
        want = json.load(open(argv[argv.index('--compare') + 1]))['digests']
        bad = ['%s: %s' % (c, ', '.join(k for k in sorted(want[c]) if digests[c].get(k) != want[c][k])) for c in sorted(want) if digests.get(c) != want[c]]
        print('%s: %d of %d cases identical' % (A._lib.LIB_PATH, len(want) - len(bad), len(want)))
        for b in bad:
            print('  differs  ' + b)
        return 1 if bad else 0
    commit = argv[argv.index('--commit') + 1]
    out = argv[argv.index('--out') + 1] if '--out' in argv else T.FIXTURE
    doc = {'written_by': {'commit': commit, 'rocm': rocm_version(), 'tool': 'tools/record_ms_bits.py',
                          'note': 'SHA-256 of raw bytes; inputs and cases: tests/%s.py' % MODULE},
           'digests': digests}
    with open(out, 'w') as f:          # one line per case
        f.write('{"written_by": %s,\n "digests": {\n' % json.dumps(doc['written_by'], sort_keys=True))
        f.write(',\n'.join('  %s: %s' % (json.dumps(c), json.dumps(digests[c], sort_keys=True)) for c in sorted(digests)))
        f.write('\n }}\n')
    print('wrote %s (%d cases)' % (out, len(digests)))
    return 0


if __name__ == '__main__':
    sys.exit(main(sys.argv[1:]))
