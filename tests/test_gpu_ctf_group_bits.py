"""
adm_ctf_fwd_adj bit for bit against digests recorded with the build before the distance gradient (pytest -m gpu).

The launch group of adm_holo_ctf.hip now takes its distances from the device too and sums dL/dd in C4 / C5, both under run-time
branches that the old entry point never enters (dists_dev = grad_dists = NULL).  Adding them must not change a single bit of what
adm_ctf_fwd_adj computes: every sum of the group has a fixed order and no atomics.  One accumulating launch into zeros per case,
inputs of tests/ctf_matrix.inputs:

  16x16x3      one C3 block over three distances, C4 with 125 idle slots
  1024x16x3    LPB = 2: C4 in two rounds, the second ragged
  16x2048x2    rows of four waves, twiddles from global memory, 2048 C4 blocks

Compared: SHA-256 of the raw bytes of pred, loss_sum, grad_obj and grad_lg_kappa.  No tolerance.  tests/golden/ctf_group_bits.json
is written by tools/record_ms_bits.py --module test_gpu_ctf_group_bits and names the commit and the ROCm version that wrote it.
"""
import ctypes as C
import hashlib
import json
import os

import numpy as np
import pytest

from tests import ctf_matrix as CM

pytestmark = pytest.mark.gpu

CASES = ((16, 16, 3), (1024, 16, 3), (16, 2048, 2))
FIXTURE = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden', 'ctf_group_bits.json')


def case_id(ny, nx, nd):
    return '%dx%dx%d' % (ny, nx, nd)


def _sha(a):
    return hashlib.sha256(np.ascontiguousarray(a).tobytes()).hexdigest()


def run_case(A, ctx, ny, nx, nd, raw=False):
    """One adm_ctf_fwd_adj (want_grad = 1 into zeros); {name: sha256 of the raw bytes}, or the arrays."""
    from adorym_amd._lib import CtfDesc, check
    c = CM.inputs(ny, nx, nd)
    h = C.c_void_p()
    desc = CtfDesc(ny=ny, nx=nx, n_dists=nd, raw_intensity=1, energy_ev=CM.ENERGY_EV, psize_cm=CM.PSIZE_CM)
    check(ctx.lib.adm_ctf_create(ctx.handle, C.byref(desc), C.byref(h)))
    obj, data, lgk = ctx.array(c['obj']), ctx.array(c['data']), ctx.array(np.array([c['lg_kappa']], np.float32))
    g_obj, g_kappa = ctx.zeros((ny, nx, 2)), ctx.zeros((1,))
    pred, loss = ctx.zeros((nd, ny, nx)), ctx.zeros((nd,))
    dists = np.ascontiguousarray(c['dists'], np.float64)
    check(ctx.lib.adm_ctf_fwd_adj(h, obj.ptr, dists.ctypes.data_as(C.POINTER(C.c_double)), lgk.ptr, data.ptr, 1, g_obj.ptr, g_kappa.ptr,
                                  pred.ptr, loss.ptr))
    out = dict(pred=pred.get(), loss_sum=loss.get(), grad_obj=g_obj.get(), grad_lg_kappa=g_kappa.get())
    check(ctx.lib.adm_ctf_destroy(h))
    for k, v in out.items():
        assert np.isfinite(v).all() and np.any(v), (case_id(ny, nx, nd), k, 'not finite, or all zero')
    return out if raw else {k: _sha(v) for k, v in out.items()}


@pytest.fixture(scope='module')
def A():
    import adorym_amd
    return adorym_amd


@pytest.fixture(scope='module')
def ctx(A):
    c = A.Context(0)
    yield c
    c.close()


@pytest.fixture(scope='module')
def recorded():
    with open(FIXTURE) as f:
        return json.load(f)


def test_fixture_names_its_origin_and_every_case(recorded):
    assert recorded['written_by']['commit'] and recorded['written_by']['rocm']
    assert sorted(recorded['digests']) == sorted(case_id(*c) for c in CASES)


@pytest.mark.parametrize('shape', CASES, ids=lambda s: case_id(*s))
def test_the_old_entry_gives_the_recorded_bits(A, ctx, recorded, shape):
    """ctf_c1 ... ctf_c5 through adm_ctf_fwd_adj: the bits of the build the fixture names."""
    got = run_case(A, ctx, *shape)
    want = recorded['digests'][case_id(*shape)]
    assert sorted(got) == sorted(want)
    differ = [k for k in sorted(got) if got[k] != want[k]]
    assert not differ, '%s: bits differ from the recorded build in %s' % (case_id(*shape), ', '.join(differ))
