"""The fused rotate-and-project kernels (adm_rotate_project.hip) against the references and bars of tests/rot_matrix.py (test
infrastructure only).  Case table, references and bars; the GPU tests are in tests/test_gpu_rotate_project.py, and
tests/test_rotate_project_coverage.py checks on the CPU -- from the kernel source -- that the table reaches the launch branches
it claims.

References (inputs are rot_matrix's signed float32 fields, so sums cancel)
  S    forward: sum over z' of the four-term sample with the oracle's float32 weights (O.rotation_weights), products and sums in
       float64.  Adjoint: g0 + sum over the voxel's entries of w_j * grad_proj[y][x'_j], in float64.
  f64  O.rotate_fwd / sum over z, and O.rotate_adj of the cotangent repeated along z, in float64 and float32 (the 3x rule).

Bars
  1  forward, per element: |out - S| <= gamma(6) M + Z 2^-52 M, M = sum_z sum_j |w_j| |v_j|.  Every sample obeys rot_matrix bar 1
     with n = 4 (gamma(5) of its magnitude sum); the Z samples are added in double (each addition at most 2^-53 relative, Z - 1 of
     them: below Z 2^-52 of M), and the one rounding to float32 costs u (1 + gamma(5)) <= gamma(6) - gamma(5) of M.
     adjoint, per element: rot_matrix bar 1 with n = the voxel's entries and g0 = the previous grad_obj.
  2  rot_matrix bar 2 (the 3x rule, FLOOR = 2^-24) in relative L2 over the rows / planes written.
  3  adjointness from the GPU's own two results.
  4  canaries, bit for bit.
"""
import functools

import numpy as np

from oracle import adorym_oracle as O
from tests import rot_matrix as RM

PI = np.pi

# --------------------------------------------------------------------------- what the launch code decides, restated
# (defaults = the constants of adm_rotate_project.hip; the coverage test parses them from the source)
TILE, PLANES, MIN_BLOCKS = 16, 4, 512
ADJ_PLANES, ADJ_VOX = 4, 4


def lanes_along_z(size, theta):
    """rpj_lanes_along_z: the difference of two neighbouring entries at the middle of the fp16 table."""
    _, X, Z = size
    if theta is None or Z < 2:
        return True
    c = np.asarray(O.rotation_coords(size, np.float32(theta))).astype(np.float32).reshape(X * Z, 2)
    i = (X // 2) * Z + (Z - 1) // 2
    dx, dz = c[i + 1, 0] - c[i, 0], c[i + 1, 1] - c[i, 1]
    return bool(abs(dz) >= abs(dx))


def fwd_planes(X, ny, tile=TILE, planes=PLANES, min_blocks=MIN_BLOCKS):
    """planes per workgroup of rotate_project_fwd_kernel (adm_rotate_project_fwd)."""
    tiles = (X + tile - 1) // tile
    return planes if tiles * ((ny + planes - 1) // planes) >= min_blocks else 1


def fwd_workgroups_per_row(X, tile=TILE):
    return (X + tile - 1) // tile


def adj_workgroups_per_plane(X, Z, vox=ADJ_VOX):
    return (X * Z + 256 * vox - 1) // (256 * vox)


# name: (Y, X, Z), theta (None: coords = NULL), y ranges, pads ('rm': rot_matrix.positions; 'zero')
CASES = {
    'x37z53_t0.3':     ((3, 37, 53), 0.3, ((0, 3),), 'rm'),             # odd and ragged; lanes along z'
    'x37z53_t1.2':     ((3, 37, 53), 1.2, ((0, 3),), 'rm'),             # lanes along x'
    'x48z80_pi4':      ((2, 48, 80), PI / 4, ((0, 2),), 'rm'),          # the tie
    'x200z120_t0.3':   ((2, 200, 120), 0.3, ((0, 2),), 'rm'),           # several workgroups per row, Z no multiple of a wave
    'x256z256_pi4':    ((2, 256, 256), PI / 4, ((0, 2),), 'rm'),        # the workload's plane
    'x64z64_t0':       ((3, 64, 64), 0.0, ((0, 3),), 'rm'),             # axis angles: unit weights, border clamps
    'x64z64_halfpi':   ((3, 64, 64), PI / 2, ((0, 3),), 'rm'),
    'x64z64_pi':       ((3, 64, 64), PI, ((0, 3),), 'rm'),
    'x16z1_null':      ((3, 16, 1), None, ((0, 3),), 'rm'),             # coords = NULL; one workgroup per row
    'x16z7_null':      ((3, 16, 7), None, ((0, 3),), 'rm'),
    'x64z64_t0.7':     ((5, 64, 64), 0.7, ((0, 5), (1, 4)), 'rm'),      # whole and partial range, non-zero pads
    'y126x256z3_t0.3': ((126, 256, 3), 0.3, ((0, 126), (1, 126)), 'rm'),    # RPJ_PLANES planes per workgroup, a short last group
}


class CaseRefs(object):
    def __init__(self, name):
        self.name = name
        self.size, self.theta, self.ranges, self.pads = CASES[name]
        Y, X, Z = self.size
        self.obj, cot3, self.g0 = RM.fields(name, self.size)
        self.cot = np.ascontiguousarray(cot3[:, :, 0, :])                  # [Y, X, 2]: the cotangent of the projection
        self.coords = RM.coords_of(self.size, self.theta)
        self.op = RM.operator(self.size, self.theta)
        idx, w = self.op
        o = self.obj.reshape(Y, X * Z, 2).astype(np.float64)
        w64 = w.astype(np.float64)
        samp = sum(o[:, idx[k], :] * w64[k][None, :, None] for k in range(4)).reshape(Y, X, Z, 2)
        mag = sum(np.abs(o[:, idx[k], :]) * np.abs(w64[k])[None, :, None] for k in range(4)).reshape(Y, X, Z, 2)
        self.fwd_S = samp.sum(axis=2)
        self.fwd_M = mag.sum(axis=2)
        self.fwd_bound = forward_bound(self.fwd_M, Z)
        vol = np.ascontiguousarray(np.broadcast_to(self.cot[:, :, None, :], self.obj.shape))
        self._adj = RM.sharp_adjoint_terms(self.op, vol)
        o64 = self.obj.astype(np.float64)
        if self.theta is None:
            f64, f32 = o64, self.obj
            self.adj_64, self.adj_32 = vol.astype(np.float64), vol
        else:
            f64, f32 = O.rotate_fwd(o64, self.coords, 'float64'), O.rotate_fwd(self.obj, self.coords, 'float32')
            self.adj_64 = O.rotate_adj(vol.astype(np.float64), self.coords, 'float64')
            self.adj_32 = O.rotate_adj(vol, self.coords, 'float32')
        self.fwd_64 = np.asarray(f64, np.float64).sum(axis=2)
        self.fwd_32 = np.asarray(f32, np.float32).sum(axis=2, dtype=np.float32)

    def adjoint(self, g0):
        S, mag, n = self._adj
        _, X, Z = self.size
        g64 = g0.astype(np.float64)
        return (g64 + S, RM.gamma(n + 1).reshape(1, X, Z, 1) * (np.abs(g64) + mag), g64 + self.adj_64,
                (g0 + np.asarray(self.adj_32, np.float32)).astype(np.float32))


def forward_bound(M, Z):
    return (RM.gamma(6) + Z * 2.0 ** -52) * M


@functools.lru_cache(maxsize=4)
def case_refs(name):
    return CaseRefs(name)


def check_fwd_bar1(got, S, bound, what):
    err = np.abs(got.astype(np.float64) - S)
    bad = err > bound
    if bad.any():
        ratio = np.where(bound > 0, err / np.where(bound > 0, bound, 1), np.where(err > 0, np.inf, 0))
        y, x, c = np.unravel_index(np.argmax(ratio), ratio.shape)
        raise AssertionError('%s: bar 1 violated at %d elements; worst (y, x, c) = (%d, %d, %d): got %r, S %r, |err| / bound = %.3g'
                             % (what, bad.sum(), y, x, c, got[y, x, c], S[y, x, c], ratio[y, x, c]))
    return float(np.max(np.where(bound > 0, err / np.where(bound > 0, bound, 1), 0)))
