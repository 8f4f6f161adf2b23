"""CPU-only: the order in which adm_rotate_adj_staged's blocks take the 16 x 16 patches (adm_patch_order, the host form of the
function the kernel evaluates) is a permutation of the patch grid with the border ring first."""
import ctypes

import numpy as np
import pytest


@pytest.fixture(scope='module')
def lib():
    import __graft_entry__ as g
    g.build()
    from adorym_amd import _lib
    return _lib.load()


@pytest.mark.parametrize('nx,nz', [(1, 1), (1, 5), (3, 3), (16, 16), (13, 8), (5, 1), (2, 7), (3, 4)])
def test_patch_order_is_a_permutation_with_the_border_ring_first(lib, nx, nz):
    order = np.full(nx * nz + 1, -7, np.int32)                        # one canary behind the table
    n_ring = lib.adm_patch_order(nx, nz, order.ctypes.data_as(ctypes.c_void_p))
    assert order[-1] == -7
    order = order[:-1]
    assert sorted(order.tolist()) == list(range(nx * nz))
    px, pz = order % nx, order // nx
    on_ring = (px == 0) | (px == nx - 1) | (pz == 0) | (pz == nz - 1)
    assert n_ring == on_ring.sum() == nx * nz - max(nx - 2, 0) * max(nz - 2, 0)
    assert on_ring[:n_ring].all() and not on_ring[n_ring:].any()


def test_patch_order_refuses_bad_arguments(lib):
    buf = np.zeros(4, np.int32)
    assert lib.adm_patch_order(0, 2, buf.ctypes.data_as(ctypes.c_void_p)) < 0
    assert lib.adm_patch_order(2, 2, None) < 0
