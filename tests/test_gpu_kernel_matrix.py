"""Every compiled variant of the multislice and probe-shift kernels (adm_multislice.hip) against the fp64 oracle, and the any-size
kernel (adm_ms_generic.hip) at the edges of what it accepts (pytest -m gpu).

The object is not square, positions hang over all four edges and B = 11 (> 8 and not a multiple of 8: the workgroup -> position
map of xcd_position uses slots > 0 and uneven shares).  tests/ms_matrix.py holds the case builder and the tables;
tests/test_kernel_matrix_coverage.py checks on the CPU that the tables cover every size and dispatch branch of the source.
"""
import numpy as np
import pytest

from tests import ms_matrix as MM
from oracle import adorym_oracle as O      # checker only

pytestmark = pytest.mark.gpu


@pytest.fixture(scope='module')
def A():
    import adorym_amd
    return adorym_amd


@pytest.fixture(scope='module')
def ctx(A):
    c = A.Context(0)
    yield c
    c.close()


def _branch_id(br):
    b1, multi, mode, pp = br
    return 'mode%d%s%s%s' % (mode, '' if b1 else '_binned', '_modes' if multi else '', '_pp' if pp else '')


@pytest.mark.parametrize('P,branch', MM.BRANCH_CASES, ids=['%d-%s' % (P, _branch_id(br)) for P, br in MM.BRANCH_CASES])
def test_every_size_and_dispatch_branch_vs_oracle(A, ctx, P, branch):
    """(a) prediction, loss, object gradient, probe gradient (and per mode), per-position probe and shift gradients."""
    MM.check(MM.run_case(A, ctx, P, **MM.BRANCHES[branch]), MM.TUNED)


@pytest.mark.parametrize('P,variant', MM.VARIANT_CASES, ids=['%d-%s' % c for c in MM.VARIANT_CASES])
def test_every_size_detector_and_loss_variants_vs_oracle(A, ctx, P, variant):
    """(b) sign conventions and 'ortho' in the far field, near field, Fresnel to the detector, the exact slice kernel, Poisson on
    magnitude and intensity data, beamstop weights, three detector distances with per-position probes."""
    MM.check(MM.run_case(A, ctx, P, seed=1, **MM.VARIANTS[variant]), MM.TUNED)


@pytest.mark.parametrize('n_modes', [1, 3])
@pytest.mark.parametrize('P', MM.SHIFT_SIZES)
def test_probe_shift_kernel_at_every_size_vs_oracle(A, ctx, P, n_modes):
    """(c) adm_probe_shift: the shifted probe sets of every position, entries reused through the index, shifts of both signs and
    beyond one pixel, against the oracle's Fourier shift in fp64 (bar: the prediction's, and 3x the oracle's own fp32 error)."""
    from adorym_amd._lib import check
    r = np.random.default_rng([P, n_modes, 7])
    B, n_ent = 11, 6
    shifts = r.uniform(-3.5, 3.5, (n_ent, 2))
    shifts[0], shifts[1] = (2.6, -1.3), (-0.4, 3.1)
    idx = np.array([0, 1, 2, 3, 4, 5, 1, 0, 5, 5, 2], np.int32)
    probes = (0.5 + r.uniform(0, 1, (n_modes, P, P))) * np.exp(1j * r.uniform(-np.pi, np.pi, (n_modes, P, P)))
    eng = A.MultisliceEngine(ctx, (P + 4, P + 6, 2), (P, P), np.array([(0, 0)]), MM.ENERGY_EV, MM.PSIZE_CM, n_probe_modes=n_modes)
    out = ctx.zeros((B, n_modes, P, P, 2))
    d_probes, d_shifts, d_idx = ctx.array(MM.c2(probes)), ctx.array(shifts, np.float32), ctx.array(idx)     # alive until read back
    check(ctx.lib.adm_probe_shift(eng.plan.handle, d_probes.ptr, d_shifts.ptr, d_idx.ptr, B, out.ptr))
    got = MM.cplx(out.get())
    ref = np.stack([O.fourier_shift(probes, shifts[e], 'float64') for e in idx])
    r32 = np.stack([O.fourier_shift(probes.astype(np.complex64), shifts[e].astype(np.float32), 'float32') for e in idx])
    for b in range(B):
        for m in range(n_modes):
            e, e32 = MM.rel(got[b, m], ref[b, m]), MM.rel(r32[b, m], ref[b, m])
            assert e < MM.TUNED['pred'] and e <= 3 * e32 + 1e-6, (b, m, e, e32)
    eng.plan.close()


@pytest.mark.parametrize('n_modes', [1, 3])
@pytest.mark.parametrize('P', MM.SHIFT_SIZES)
def test_multislice_through_probe_shifts_at_every_size_vs_oracle(A, ctx, P, n_modes):
    """(c) the shift adjoint (adm_probe_shift_adj) at every size, far field with sign_convention = -1: shift gradients, probe gradient
    through the shifts (whole and per mode) and the per-position probe gradients it consumes."""
    MM.check(MM.run_case(A, ctx, P, n_modes=n_modes, pp='shifts', sign_convention=-1, seed=2), MM.TUNED)


@pytest.mark.parametrize('Py,Px', MM.GENERIC_FIELDS, ids=['%dx%d' % f for f in MM.GENERIC_FIELDS])
def test_generic_kernel_at_its_edges_vs_oracle(A, ctx, Py, Px):
    """(d) the any-size kernel: one large-prime pass, the loop over the remaining primes, 8 x 2048 / 2048 x 8, the largest
    accepted field."""
    MM.check(MM.run_case(A, ctx, (Py, Px), seed=3), MM.GENERIC)


@pytest.mark.parametrize('Py,Px', MM.GENERIC_REFUSED, ids=['%dx%d' % f for f in MM.GENERIC_REFUSED])
def test_generic_kernel_refuses_the_first_field_too_large(A, ctx, Py, Px):
    """(d) one past the acceptance boundary (Py*Px <= 16384, LDS <= 160 KB - 256): refused at plan creation."""
    with pytest.raises(NotImplementedError):
        A.MultisliceEngine(ctx, (Py + 2, Px + 2, 3), (Py, Px), np.array([(0, 0)]), MM.ENERGY_EV, MM.PSIZE_CM)
    assert b'too large' in ctx.lib.adm_last_error()


def test_per_position_probes_with_binning_are_refused_at_the_c_abi(A, ctx):
    """(d) no per-position-probe kernel bins slices: adm_multislice_fwd_adj_pp returns ADM_ERR_UNSUPPORTED for binning > 1."""
    from adorym_amd import _lib
    P, B = 16, 2
    pos = np.array([(0, 0), (3, 5)])
    eng = A.MultisliceEngine(ctx, (P + 5, P + 7, 4), (P, P), pos, MM.ENERGY_EV, MM.PSIZE_CM, binning=2, max_batch=B)
    eng.set_batch(pos, np.ones((B, P, P), np.float32))
    probes = ctx.zeros((B, 1, P, P, 2))
    loss = ctx.zeros((B,))
    rc = ctx.lib.adm_multislice_fwd_adj_pp(eng.plan.handle, eng.obj_rot.ptr, probes.ptr, eng._cur_pos.ptr, B, eng._cur_target.ptr, 1,
                                           None, None, loss.ptr, 1.0, eng._ws.ptr, eng._ws.nbytes)
    assert rc == _lib.ADM_ERR_UNSUPPORTED
    assert b'binning' in ctx.lib.adm_last_error()
    eng.plan.close()


def test_generic_kernel_per_position_probe_gradients_stay_in_their_slots(A, ctx):
    """(d) adm_multislice_fwd_adj_pp on a generic plan (40 x 24) with a grad_probes buffer: every position's probe gradient is
    left in its own slot, and nothing is summed over the slots afterwards.  Slot b equals BIT FOR BIT the grad_probe of a
    batch-of-one adm_multislice_fwd_adj launch of position b into a zeroed buffer with the same grad_scale (same workgroup,
    same arithmetic, 0 + v = v)."""
    from adorym_amd._lib import check
    (Py, Px), B, S, M = (40, 24), 3, 4, 1
    case = MM.oracle_case((Py, Px), S=S, B=4, seed=4)           # (inputs only; edge_positions makes four corners)
    obj, pos, target = case['obj'], case['pos'][:B], case['target'][:B]
    eng = A.MultisliceEngine(ctx, obj.shape[:2] + (S,), (Py, Px), case['pos'], MM.ENERGY_EV, MM.PSIZE_CM, n_probe_modes=M, max_batch=B)
    eng.set_batch(pos, target)
    eng.rotate(ctx.array(obj, np.float32), None)
    probe = MM.c2(case['probes'])                                # [M, Py, Px, 2]
    d_probe = ctx.array(probe)
    d_probes = ctx.array(np.ascontiguousarray(np.broadcast_to(probe, (B,) + probe.shape)))
    d_slots = ctx.zeros((B, M, Py, Px, 2))
    loss = ctx.zeros((B,))
    scale = 2.0 / (B * Py * Px)
    lib, h = ctx.lib, eng.plan.handle
    check(lib.adm_multislice_fwd_adj_pp(h, eng.obj_rot.ptr, d_probes.ptr, eng._cur_pos.ptr, B, eng._cur_target.ptr, 1, d_slots.ptr, None,
                                        loss.ptr, scale, eng._ws.ptr, eng._ws.nbytes))
    slots = d_slots.get()
    for b in range(B):
        d_gp = ctx.zeros((M, Py, Px, 2))
        check(lib.adm_multislice_fwd_adj(h, eng.obj_rot.ptr, d_probe.ptr, eng._cur_pos.ptr + 8 * b, 1, eng._cur_target.ptr + 4 * b * Py * Px,
                                         1, d_gp.ptr, None, loss.ptr, scale, eng._ws.ptr, eng._ws.nbytes))
        one = d_gp.get()
        assert np.abs(one).max() > 0
        differ = int((slots[b].view(np.uint32) != one.view(np.uint32)).sum())
        print('slot %d: %d of %d words differ from the batch-of-one launch' % (b, differ, one.size))
        assert differ == 0, (b, differ)
    eng.plan.close()
