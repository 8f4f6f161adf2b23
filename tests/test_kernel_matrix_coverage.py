"""The kernel-matrix sweep (tests/test_gpu_kernel_matrix.py) covers what adm_multislice.hip compiles: every probe size of
ADM_FOR_EACH_SIZE, every ADM_LAUNCH branch of launch<> and every size of the probe-shift kernels.  Parsed from the source, so
that a size or a branch added there fails this CPU test until ms_matrix.py's tables name it."""
import os
import re

from tests import ms_matrix as MM

SRC = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), 'adorym_amd', 'csrc', 'adm_multislice.hip')


def _source():
    with open(SRC) as f:
        return f.read()


def _function_body(src, signature):
    """Text of the brace-balanced body of the first function whose head matches ``signature``."""
    m = re.search(signature, src)
    assert m, signature
    i = src.index('{', m.end())
    depth = 0
    for j in range(i, len(src)):
        depth += {'{': 1, '}': -1}.get(src[j], 0)
        if depth == 0:
            return src[i:j + 1]
    raise AssertionError('unbalanced body: ' + signature)


def compiled_sizes(src):
    m = re.search(r'#define\s+ADM_FOR_EACH_SIZE\(X\)(.*)', src)
    assert m, 'ADM_FOR_EACH_SIZE not found'
    sizes = [tuple(int(v) for v in t) for t in re.findall(r'X\(\s*(\d+)\s*,\s*(\d+)\s*,\s*(\d+)\s*\)', m.group(1))]
    assert sizes and all(n == r1 * r2 for n, r1, r2 in sizes), sizes
    return [n for n, _, _ in sizes]


def launch_branches(src):
    body = _function_body(src, r'static\s+hipError_t\s+launch\s*\(')
    body = re.sub(r'#define[^\n]*\n', '', body)            # the macro's own definition is not a launch
    lit = {'true': True, 'false': False}
    calls = re.findall(r'ADM_LAUNCH\(\s*(\w+)\s*,\s*(\w+)\s*,\s*(\d+)\s*,\s*(\w+)\s*\)', body)
    assert calls, 'no ADM_LAUNCH in launch<>'
    return [(lit[b1], lit[mu], int(mode), lit[pp]) for b1, mu, mode, pp in calls]


def shift_sizes(src):
    body = _function_body(src, r'hipError_t\s+shift_launch\s*\(')
    assert 'launch_shift<' in body
    return compiled_sizes(src) if 'ADM_FOR_EACH_SIZE(X)' in body else []


def test_the_parsers_see_the_kernel_matrix():
    src = _source()
    assert len(compiled_sizes(src)) >= 10
    br = launch_branches(src)
    assert len(br) == len(set(br)) >= 14, br
    assert shift_sizes(src) == compiled_sizes(src)


def test_every_compiled_size_and_branch_is_swept():
    src = _source()
    sizes, branches = compiled_sizes(src), set(launch_branches(src))
    assert set(sizes) <= set(MM.SIZES), 'sizes compiled but not swept: %s' % sorted(set(sizes) - set(MM.SIZES))
    assert branches <= set(MM.BRANCHES), 'branches compiled but not swept: %s' % sorted(branches - set(MM.BRANCHES))
    assert set(MM.BRANCHES) <= branches, 'swept branches that launch<> no longer has: %s' % sorted(set(MM.BRANCHES) - branches)
    pairs = set(MM.BRANCH_CASES)
    missing = [(n, b) for n in sizes for b in branches if (n, b) not in pairs]
    assert not missing, 'size x branch pairs not swept: %s' % missing


def test_every_branch_case_reaches_its_branch():
    """The arguments filed under a branch take that branch (the engine's dispatch, mirrored by ms_matrix.dispatch)."""
    for br, kw in MM.BRANCHES.items():
        assert MM.dispatch(kw) == br, (br, kw)


def test_every_shift_kernel_size_is_swept():
    src = _source()
    assert set(shift_sizes(src)) <= set(MM.SHIFT_SIZES), sorted(set(shift_sizes(src)) - set(MM.SHIFT_SIZES))


def test_every_size_runs_every_detector_and_loss_variant():
    assert set(MM.VARIANT_CASES) == {(n, v) for n in compiled_sizes(_source()) for v in MM.VARIANTS}
