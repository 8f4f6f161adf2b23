"""The rotation matrix (tests/test_gpu_rotation_matrix.py, tables in tests/rot_matrix.py) reaches every path it claims: the box
classes of every staged and stacked case from the host table builder, the y_chunk / npl values recomputed from thresholds
parsed out of the kernel source, and every rotation entry point and kernel of the source named by a row of the table.  A
changed constant, a new branch threshold or a new rotation kernel fails here, on the CPU, until the tables are revisited.
Also: bar 1 holds for the oracle's own float32 results and does not hold for an operator that lost or doubled one entry."""
import os
import re

import numpy as np

from tests import rot_matrix as RM

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, 'adorym_amd', 'csrc')


def _read(*parts):
    with open(os.path.join(*parts)) as f:
        return f.read()


def _object_src():
    return _read(CSRC, 'adm_rotate.hip')


def _rotcsr_src():
    return _read(CSRC, 'adm_rotcsr.hip')


def _one(pattern, text, what):
    found = re.findall(pattern, text)
    assert len(found) == 1, '%s: expected one match of %r, found %r' % (what, pattern, found)
    return found[0]


def parsed_constants():
    """The constants and thresholds the tables depend on, from adm_rotate.hip, adm_rotcsr.hip and util.py."""
    src = _object_src()
    k = {}
    k['stage_max'] = int(_one(r'#define\s+ADM_STAGE_MAX\s+(\d+)', src, 'ADM_STAGE_MAX'))
    k['stack_min_blocks'] = int(_one(r'#define\s+ADM_STACK_MIN_BLOCKS\s+(\d+)', src, 'ADM_STACK_MIN_BLOCKS'))
    # the stage of both staged kernels holds 4 planes of ADM_STAGE_MAX, and both take two rim planes per pass when they fit it
    assert len(re.findall(r'__shared__\s+float2\s+stage\[4 \* ADM_STAGE_MAX\]', src)) == 2
    rim = set(re.findall(r'(\d+) \* per <= (\d+) \* ADM_STAGE_MAX', src))
    assert len(rim) == 1 and len(re.findall(r'\d+ \* per <= \d+ \* ADM_STAGE_MAX', src)) == 2, rim
    k['rim2'] = tuple(int(v) for v in rim.pop())
    assert len(re.findall(r'per <= ADM_STAGE_MAX\)', src)) == 2           # the interior test of both staged kernels
    assert len(re.findall(r'if \(bw == 0\)', src)) == 2                   # the no-box test of both
    k['box_limit_device'] = int(_one(r'bw \* bh > (\d+)', _rotcsr_src(), 'box limit of rotcsr_boxes_kernel'))
    k['box_limit_host'] = int(_one(r'bw \* bh > (\d+)', _read(ROOT, 'adorym_amd', 'util.py'), 'box limit of build_rotation_adjoint_csr'))
    fwd = RM.function_body(src, r'extern "C" int adm_rotate_fwd\(')
    k['fwd_chunk'] = int(_one(r'int y_chunk = (\d+);', fwd, 'y_chunk of adm_rotate_fwd'))
    k['fwd_min_blocks'] = int(_one(r'while \(y_chunk > 1 && n_patch \* \(\(y_hi - y_lo \+ y_chunk - 1\) / y_chunk\) < (\d+)\) y_chunk >>= 1;', fwd,
                                   'block threshold of adm_rotate_fwd'))
    adj = RM.function_body(src, r'extern "C" int adm_rotate_adj\(')
    k['adj_chunk'] = int(_one(r'const int y_chunk = (\d+);', adj, 'y_chunk of adm_rotate_adj'))
    st = RM.function_body(src, r'extern "C" int adm_rotate_adj_staged_stack\(')
    k['npl'] = int(_one(r'int npl = (\d+);', st, 'npl of adm_rotate_adj_staged_stack'))
    assert _one(r'\n\s+npl = (\d+);', st, 'npl of the scratch form') == str(k['npl'])
    k['npl_min_blocks'] = int(_one(r'while \(npl > 1 && n_patch \* \(\(Yb \+ npl - 1\) / npl\) < (\d+)\) npl >>= 1;', st, 'sequential threshold'))
    assert len(re.findall(r'while \(npl > 1 && \(size_t\)n_patch \* \(\(Yb \+ npl - 1\) / npl\) \* n_tables < \(size_t\)ADM_STACK_MIN_BLOCKS\) npl >>= 1;',
                          st)) == 1, 'scratch threshold'
    return k


def test_the_restated_constants_are_the_sources():
    k = parsed_constants()
    assert k['stage_max'] == RM.STAGE_MAX and k['rim2'] == RM.RIM2_PLANES
    assert k['box_limit_device'] == k['box_limit_host'] == RM.BOX_LIMIT
    assert RM.BOX_LIMIT <= 4 * RM.STAGE_MAX                       # a one-plane rim box fits the stage
    assert (k['fwd_chunk'], k['fwd_min_blocks'], k['adj_chunk']) == (RM.FWD_CHUNK, RM.FWD_MIN_BLOCKS, RM.ADJ_CHUNK)
    assert (k['npl'], k['npl_min_blocks'], k['stack_min_blocks']) == (RM.NPL, RM.NPL_MIN_BLOCKS, RM.STACK_MIN_BLOCKS)


def _classes(size, theta, k):
    cls, rows, patch = RM.patch_classes(size, theta, stage_max=k['stage_max'], rim2=k['rim2'])
    return cls, rows, patch


def test_every_staged_case_reaches_the_box_classes_it_claims():
    k = parsed_constants()
    reached = set()
    for name in RM.ROTATED:
        size, theta, _, _, claimed = RM.CASES[name]
        cls, rows, patch = _classes(size, theta, k)
        assert set(cls) == set(claimed), (name, sorted(set(cls)), sorted(claimed))
        reached |= set(cls)
        boxes = RM.host_tables(size, theta, True)[4]
        per = boxes[:, 2].astype(int) * boxes[:, 3]
        assert per.max() <= k['box_limit_host'] and ((boxes[:, 2] == 0) == (cls == 'nobox')).all()
    assert reached == set(RM.BOX_CLASSES)
    assert RM.NOBOX_CASES and all('nobox' in RM.CASES[n][4] for n in RM.NOBOX_CASES)
    # the angles asked for: axis-aligned, above pi; a square size with no-box patches; both orientations of a flat object
    thetas = [RM.CASES[n][1] for n in RM.ROTATED]
    for want in (0.0, np.pi / 2, np.pi, 2 * np.pi):
        assert any(abs(t - want) < 1e-12 for t in thetas), want
    assert any(np.pi < t < 2 * np.pi for t in thetas)
    assert any(RM.CASES[n][0][1] == RM.CASES[n][0][2] for n in RM.NOBOX_CASES)
    sizes = {RM.CASES[n][0][1:] for n in RM.ROTATED}
    assert any((z, x) in sizes and x != z for x, z in sizes)


def test_csr_rows_exercise_the_unrolled_loop_and_its_edges():
    """Rows of rim patches (the 8-way unrolled loop) with a length that is no multiple of 8, below 8, above 1024 and empty;
    rows of no-box patches that are empty and not."""
    k = parsed_constants()
    rim_rows, nobox_rows = [], []
    for name in RM.ROTATED:
        size, theta = RM.CASES[name][:2]
        cls, rows, patch = _classes(size, theta, k)
        is_rim = np.isin(cls[patch], ('rim1', 'rim2'))
        rim_rows.append(rows[is_rim])
        nobox_rows.append(rows[cls[patch] == 'nobox'])
    rim_rows, nobox_rows = np.concatenate(rim_rows), np.concatenate(nobox_rows)
    assert (rim_rows % 8 != 0).any() and (rim_rows == 0).any() and (rim_rows > 1024).any() and ((rim_rows > 0) & (rim_rows < 8)).any()
    assert (rim_rows[rim_rows > 0] % 8 == 0).any()                # ... and a row that ends exactly on a group of eight
    assert (nobox_rows == 0).any() and (nobox_rows > 0).any()


def test_patch_tails_and_y_ranges():
    tails = [n for n in RM.ROTATED if RM.CASES[n][0][1] % 16 and RM.CASES[n][0][2] % 16]
    no_tails = [n for n in RM.ROTATED if RM.CASES[n][0][1] % 16 == 0 and RM.CASES[n][0][2] % 16 == 0]
    assert tails and no_tails
    rests = set()
    for name, (size, theta, (lo, hi), _, _) in RM.CASES.items():
        assert 0 < lo < hi <= size[0] and (hi - lo) % 4 != 0, name
        rests.add((hi - lo) % 4)
        (py0, _), (px0, _) = RM.pads_of(size)
        assert py0 > 0 and px0 > 0, name
    assert rests == {1, 2, 3}
    assert any(RM.CASES[n][0][0] > parsed_constants()['adj_chunk'] for n in RM.ROTATED)      # the atomic kernel's second chunk


def test_forward_y_chunks_are_the_claimed_ones():
    k = parsed_constants()
    reached = set()
    for name, (size, theta, (lo, hi), claimed, _) in RM.CASES.items():
        Y, X, Z = size
        if theta is None and Z < 16:
            continue                                               # identity_fwd_kernel: no y_chunk
        full = RM.fwd_y_chunk(X, Z, Y, k['fwd_chunk'], k['fwd_min_blocks'])
        assert full == claimed, (name, full, claimed)
        reached |= {full, RM.fwd_y_chunk(X, Z, hi - lo, k['fwd_chunk'], k['fwd_min_blocks'])}
        if full == k['fwd_chunk']:
            assert Y % full != 0, name                             # the largest chunk with a tail
    assert {k['fwd_chunk'], 1} <= reached and any(1 < v < k['fwd_chunk'] for v in reached), reached
    assert {32, 8, 2, 1} <= reached
    # coords = NULL: the general kernels at Z >= 16, the identity kernels below, Z = 1 among them
    null_z = sorted(RM.CASES[n][0][2] for n in RM.CASES if RM.CASES[n][1] is None)
    assert null_z[0] == 1 and any(1 < z < 16 for z in null_z) and null_z[-1] >= 16
    body = RM.function_body(_object_src(), r'extern "C" int adm_rotate_fwd\(')
    assert 'if (!coords && d.obj_z < 16)' in body
    assert 'if (!coords && d.obj_z < 16)' in RM.function_body(_object_src(), r'extern "C" int adm_rotate_adj\(')


def test_stacked_cases_reach_npl_1_2_4_in_both_forms():
    k = parsed_constants()
    X, Z = RM.STACK_XZ
    R = len(RM.STACK_THETAS)
    reached = set()
    for name, (Yb, scratch, claimed) in RM.STACK_CASES.items():
        npl = RM.stack_npl(X, Z, Yb, R, scratch, k['npl'], k['npl_min_blocks'], k['stack_min_blocks'])
        assert npl == claimed and ('npl%d' % npl) in name and name.startswith('scratch' if scratch else 'sequential'), (name, npl)
        reached.add((scratch, npl))
        assert Z * (R * Yb + 4) * (X + 6) * 8 <= 26e6              # the stacked frame stays around 25 MB
    assert reached == {(s, n) for s in (False, True) for n in (1, 2, 4)}
    for scratch in (False, True):
        assert any(Yb % npl for Yb, s, npl in RM.STACK_CASES.values() if s == scratch and npl > 1)
    # every angle's table holds no-box and both kinds of rim patches (npp = 1 and 2; at npl = 1 rim patches take one plane)
    for th in RM.STACK_THETAS:
        cls, _, _ = _classes((1, X, Z), th, k)
        assert set(cls) == set(RM.BOX_CLASSES), (th, sorted(set(cls)))


def _entry_points(src):
    return re.findall(r'extern "C"\s+[\w ]+?\b(adm_rotat\w+)\s*\(', src)


def _launched(body):
    return set(re.findall(r'hipLaunchKernelGGL\(\s*(\w+(?:<\w+>)?)', body))


def test_every_rotation_entry_point_and_kernel_is_in_the_table():
    import tests.test_gpu_rotation_matrix as G
    table_kernels = set()
    seen = []
    for src in (_object_src(), _rotcsr_src()):
        for name in _entry_points(src):
            seen.append(name)
            assert name in RM.ENTRY_POINTS, 'rotation entry point without a row in rot_matrix.ENTRY_POINTS: ' + name
            kernels, test = RM.ENTRY_POINTS[name]
            launched = _launched(RM.function_body(src, r'extern "C"\s+[\w ]+?\b%s\s*\(' % name))
            assert launched == set(kernels), (name, sorted(launched), sorted(kernels))
            assert callable(getattr(G, test, None)), test
            table_kernels |= {kn.split('<')[0] for kn in kernels}
    assert sorted(seen) == sorted(RM.ENTRY_POINTS), sorted(set(RM.ENTRY_POINTS) ^ set(seen))
    # every __global__ of the two files that rotates, copies for the identity or sums the stack is launched by one of them
    for src in (_object_src(), _rotcsr_src()):
        for kn in re.findall(r'__global__\s+(?:__launch_bounds__\(\d+\)\s+)?void\s+(\w+)\s*\(', src):
            if re.search(r'rot|identity|stack', kn):
                assert kn in table_kernels, 'rotation kernel that no tabulated entry point launches: ' + kn
    assert len(table_kernels) >= 14
    # the exported adjoint that nothing else calls is bound and driven in both lane orders
    from adorym_amd import _lib
    assert all(name in _lib.SIGNATURES for name in RM.ENTRY_POINTS)
    assert {'csr_lanes_z', 'csr_lanes_x', 'staged', 'atomic'} == set(RM.ADJ_PATHS)


def test_bar_1_holds_for_the_float32_oracle_and_catches_one_entry():
    """The reference alone passes bar 1 with room, and an operator with one entry dropped, doubled or moved by one voxel does
    not: the bar is as tight as a per-element bar can be."""
    for name in ('x37z53_t0.3', 'x40z72_t0', 'x64z64_t0.7'):
        c = RM.case_refs(name)
        assert RM.check_bar1(c.fwd_32, c.fwd_S, c.fwd_bound, name) < 1
        zero = np.zeros_like(c.g0)
        for g0 in (zero, c.g0):
            S, bound, f64, f32 = c.adjoint(g0)
            assert RM.check_bar1(f32, S, bound, name) < 1
            RM.check_bar2(f32, f64, f32, name)
        S, bound, _, _ = c.adjoint(zero)
        idx, w = c.op
        p = int(np.argmax(w[1]))                                   # a rotated-frame voxel with a solid second weight
        for mutate in ('drop', 'double', 'shift'):
            w2, idx2 = w.copy(), idx.copy()
            if mutate == 'drop':
                w2[1, p] = 0
            elif mutate == 'double':
                w2[1, p] *= 2
            else:
                idx2[1, p] = idx2[0, p]
            bad_fwd, _ = RM.sharp_forward((idx2, w2), c.obj)
            bad_adj, _, _ = RM.sharp_adjoint_terms((idx2, w2), c.cot)
            for got, ref, bnd in ((bad_fwd, c.fwd_S, c.fwd_bound), (bad_adj, S, bound)):
                try:
                    RM.check_bar1(got.astype(np.float32), ref, bnd, name)
                except AssertionError:
                    continue
                raise AssertionError('%s: bar 1 did not notice the operator with one entry %s' % (name, mutate))
        RM.check_adjointness(c.fwd_32, c.adjoint(zero)[3], c.obj, c.cot, c.fwd_bound, bound, name)
