"""On the CPU: the case table of tests/rotproj_matrix.py reaches the launch branches of adm_rotate_project.hip that its comments
name -- the constants and the launch arithmetic are parsed from the source, not assumed -- and bar 1 of either direction rejects a
dropped and a doubled term.  This looks at launch geometry only; the numbers are judged on the GPU
(tests/test_gpu_rotate_project.py)."""
import os
import re

import numpy as np
import pytest

from tests import rot_matrix as RM
from tests import rotproj_matrix as PM

CSRC = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), 'adorym_amd', 'csrc')


@pytest.fixture(scope='module')
def src():
    with open(os.path.join(CSRC, 'adm_rotate_project.hip')) as f:
        return f.read()


def constant(src, name):
    m = re.search(r'#define\s+%s\s+(\d+)' % name, src)
    assert m, name
    return int(m.group(1))


def test_constants_and_launch_arithmetic_are_the_restated_ones(src):
    assert (constant(src, 'RPJ_TILE'), constant(src, 'RPJ_PLANES'), constant(src, 'RPJ_MIN_BLOCKS')) == (PM.TILE, PM.PLANES, PM.MIN_BLOCKS)
    assert (constant(src, 'RPJ_ADJ_PLANES'), constant(src, 'RPJ_ADJ_VOX')) == (PM.ADJ_PLANES, PM.ADJ_VOX)
    fwd = RM.function_body(src, r'extern "C" int adm_rotate_project_fwd\(')
    assert 'tiles = (d.obj_x + RPJ_TILE - 1) / RPJ_TILE' in fwd
    assert '(size_t)tiles * ((ny + RPJ_PLANES - 1) / RPJ_PLANES) >= RPJ_MIN_BLOCKS' in fwd
    assert 'rotate_project_fwd_kernel<RPJ_PLANES>, dim3(tiles, (ny + RPJ_PLANES - 1) / RPJ_PLANES)' in fwd
    assert 'rotate_project_fwd_kernel<1>, dim3(tiles, ny)' in fwd
    adj = RM.function_body(src, r'extern "C" int adm_rotate_project_adj\(')
    assert 'per_block = (size_t)256 * RPJ_ADJ_VOX' in adj
    assert '((size_t)d.obj_x * d.obj_z + per_block - 1) / per_block' in adj and '(y_hi - y_lo + RPJ_ADJ_PLANES - 1) / RPJ_ADJ_PLANES' in adj
    lanes = RM.function_body(src, r'bool rpj_lanes_along_z\(')
    assert 'coords == nullptr || Z < 2' in lanes and '(X / 2) * Z + (Z - 1) / 2' in lanes and 'fabsf(dz) >= fabsf(dx)' in lanes
    kern = RM.function_body(src, r'void rotate_project_fwd_kernel\(')
    assert 'zr += RPJ_TILE' in kern and 'along_z ? (threadIdx.x >> 4) : (threadIdx.x & 15)' in kern


def test_the_table_reaches_every_launch_branch(src):
    tile, planes, min_blocks = constant(src, 'RPJ_TILE'), constant(src, 'RPJ_PLANES'), constant(src, 'RPJ_MIN_BLOCKS')
    adj_planes, vox = constant(src, 'RPJ_ADJ_PLANES'), constant(src, 'RPJ_ADJ_VOX')
    seen = set()
    for name, (size, theta, ranges, pads) in PM.CASES.items():
        Y, X, Z = size
        along_z = PM.lanes_along_z(size, theta)
        for lo, hi in ranges:
            ny = hi - lo
            pl = PM.fwd_planes(X, ny, tile, planes, min_blocks)
            seen.add('lanes_z' if along_z else 'lanes_x')
            seen.add('fwd_planes_%d' % pl)
            seen.add('fwd_one_workgroup_per_row' if PM.fwd_workgroups_per_row(X, tile) == 1 else 'fwd_several_workgroups_per_row')
            if X % tile:
                seen.add('fwd_ragged_tile')
            if Z % tile:
                seen.add('fwd_ragged_lanes_along_z')
            if Z < tile:
                seen.add('fwd_fewer_slices_than_lanes')
            if pl > 1 and ny % pl:
                seen.add('fwd_short_last_plane_group')
            if theta is None:
                seen.add('null_coords')
            seen.add('adj_one_workgroup_per_plane' if PM.adj_workgroups_per_plane(X, Z, vox) == 1 else 'adj_several_workgroups_per_plane')
            if (X * Z) % (256 * vox):
                seen.add('adj_voxel_tail')
            if (X * Z) % (256 * vox) == 0:
                seen.add('adj_no_voxel_tail')
            if ny % adj_planes:
                seen.add('adj_short_last_plane_group')
            if lo > 0:
                seen.add('partial_range')
    want = {'lanes_z', 'lanes_x', 'fwd_planes_1', 'fwd_planes_%d' % planes, 'fwd_one_workgroup_per_row', 'fwd_several_workgroups_per_row',
            'fwd_ragged_tile', 'fwd_ragged_lanes_along_z', 'fwd_fewer_slices_than_lanes', 'fwd_short_last_plane_group', 'null_coords',
            'adj_one_workgroup_per_plane', 'adj_several_workgroups_per_plane', 'adj_voxel_tail', 'adj_no_voxel_tail',
            'adj_short_last_plane_group', 'partial_range'}
    assert want <= seen, sorted(want - seen)
    # what the table's comments claim, row by row
    assert PM.lanes_along_z(*PM.CASES['x37z53_t0.3'][:2]) and not PM.lanes_along_z(*PM.CASES['x37z53_t1.2'][:2])
    assert PM.fwd_workgroups_per_row(200, tile) > 1 and 120 % 64 and 120 % tile
    assert PM.fwd_workgroups_per_row(16, tile) == 1
    assert PM.fwd_planes(256, 126, tile, planes, min_blocks) == planes and PM.fwd_planes(256, 125, tile, planes, min_blocks) == planes
    assert all(RM.frame(c[0])[2] > 0 and RM.frame(c[0])[3] > 0 for c in PM.CASES.values())          # non-zero pads


def test_bar1_rejects_a_dropped_and_a_doubled_term():
    """A float32 evaluation of the restatement passes bar 1 of either direction; with one term of one element left out, or taken
    twice, it does not."""
    c = PM.case_refs('x37z53_t0.3')
    Y, X, Z = c.size
    idx, w = c.op
    o = c.obj.reshape(Y, X * Z, 2)
    samp = np.zeros((Y, X * Z, 2), np.float32)
    for k in range(4):
        samp = samp + o[:, idx[k], :] * w[k][None, :, None]
    samp = samp.reshape(Y, X, Z, 2)
    good = samp.astype(np.float64).sum(axis=2).astype(np.float32)
    PM.check_fwd_bar1(good, c.fwd_S, c.fwd_bound, 'float32 restatement')
    y, x, z = 1, 17, 29
    for name, factor in (('dropped', -1.), ('doubled', 1.)):
        bad = good.copy()
        bad[y, x] = (good[y, x].astype(np.float64) + factor * samp[y, x, z]).astype(np.float32)
        with pytest.raises(AssertionError, match='bar 1'):
            PM.check_fwd_bar1(bad, c.fwd_S, c.fwd_bound, name)
    g0 = c.g0
    S, bound, _, f32 = c.adjoint(g0)
    RM.check_bar1(f32, S, bound, 'float32 oracle')
    # one entry of one voxel: its weight times the cotangent it reads
    t = x * Z + z
    rows = np.nonzero((idx == t) & (w != 0))
    assert len(rows[0]) > 0
    j = int(np.argmax(np.abs(w[rows])))          # (the voxel's largest entry: a weight at rounding level would hide under the bar)
    k, p = rows[0][j], rows[1][j]
    term = np.float64(w[k, p]) * c.cot[y, p // Z]
    for name, factor in (('dropped', -1.), ('doubled', 1.)):
        bad = f32.copy()
        bad[y, x, z] = (f32[y, x, z].astype(np.float64) + factor * term).astype(np.float32)
        with pytest.raises(AssertionError, match='bar 1'):
            RM.check_bar1(bad, S, bound, name)
