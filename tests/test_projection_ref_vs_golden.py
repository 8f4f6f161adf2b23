"""CPU-only: the NumPy restatement of the projection approximation (tests/projection_ref.py) against the values recorded from the
reference (golden F25, tests/golden/gen_f25_pure_projection.py).  The restatement is the checker of the GPU tests
(tests/test_gpu_projection.py); this file is what ties it to the reference.

Bars: those tests/test_prj_offset_ref_vs_golden.py uses for the same quantities in fp64 (prediction, loss 1e-12; gradients 1e-11).
"""
import ast
import os
import numpy as np
import pytest

from oracle import adorym_oracle as O
from tests import projection_ref as PJ

HERE = os.path.dirname(os.path.abspath(__file__))
ENERGY_EV, PSIZE_CM = 8000., 1e-6
CASES = ['s%d_%s' % (S, k) for S in (7, 1) for k in ('far_field', 'fresnel_m1_modes2', 'exit_wave', 'far_field_poisson')]


@pytest.fixture(scope='module')
def F():
    return np.load(os.path.join(HERE, 'golden', 'F25_pure_projection.npz'))


def rel(a, b):
    a, b = np.asarray(a, np.complex128), np.asarray(b, np.complex128)
    return np.linalg.norm(a - b) / np.linalg.norm(b)


def case_params(F, name):
    names = [str(n) for n in F['kernel_cases']]
    return ast.literal_eval(str(F['kernel_case_params'][names.index(name)]))       # S, free_prop, sign, modes, loss


def run_ref(F, name, dtype='float64'):
    """The restatement on the inputs of fixture case ``name``: loss, pred, object gradient, probe gradient."""
    S, free_prop, sg, M, loss = case_params(F, name)
    obj, pos, probes, meas = [F['%s/%s' % (name, k)] for k in ('obj', 'pos', 'probes', 'meas')]
    phys = O.Physics(probes.shape[-2:], ENERGY_EV, PSIZE_CM, free_prop_cm=free_prop, sign_convention=sg)
    return PJ.forward_adjoint_object(obj.astype(np.float64), None, probes.astype(np.complex128), pos, meas, phys, dtype,
                                     loss_function_type=loss)


def test_fixture_lists_every_case(F):
    assert sorted(str(n) for n in F['kernel_cases']) == sorted(CASES)
    par = [case_params(F, n) for n in CASES]
    assert {p[0] for p in par} == {1, 7} and {p[2] for p in par} == {1, -1} and {p[3] for p in par} == {1, 2}
    assert {p[4] for p in par} == {'lsq', 'poisson'}
    assert {'inf' if p[1] == 'inf' else ('none' if p[1] is None else 'fresnel') for p in par} == {'inf', 'none', 'fresnel'}
    for n in CASES:
        pos = F[n + '/pos']
        assert F[n + '/obj'].shape[:2] == (17, 27) and F[n + '/probes'].shape[1:] == (12, 20) and len(pos) == 5
        # over all four edges of the object
        assert pos[:, 0].min() < 0 and pos[:, 1].min() < 0 and pos[:, 0].max() + 12 > 17 and pos[:, 1].max() + 20 > 27


@pytest.mark.parametrize('name', CASES)
def test_restatement_matches_reference_fp64(F, name):
    loss, pred, g, gp = run_ref(F, name)
    e = rel(pred, F[name + '/pred']), abs(loss / float(F[name + '/loss']) - 1), rel(g, F[name + '/grad']), rel(gp, F[name + '/gprobe'])
    print(name, 'pred %.1e loss %.1e grad %.1e gprobe %.1e' % e)
    assert e[0] < 1e-12 and e[1] <= 1e-12 and e[2] < 1e-11 and e[3] < 1e-11
    # the model's signature: one gradient for all slices
    assert np.array_equal(g, np.broadcast_to(g[:, :, :1], g.shape))


@pytest.mark.parametrize('name', CASES)
def test_restatement_fp32_is_a_fair_yardstick(F, name):
    """The GPU tests use the restatement's fp32 run as the yardstick at sizes the fixture does not hold: it must not be a laxer one
    than the reference's own fp32 run -- at most 3x as far from fp64."""
    l64, p64, g64, gp64 = run_ref(F, name)
    l32, p32, g32, gp32 = run_ref(F, name, 'float32')
    e = F[name + '/err32']
    assert rel(p32, p64) <= 3 * e[0]
    assert rel(g32, g64) <= 3 * e[2]
    assert rel(gp32, gp64) <= 3 * e[3]


def test_one_slice_is_the_pinned_oracle(F):
    """S = 1: the projection of one slice is the slice, and the restatement is the oracle's multislice, bit for bit."""
    name = 's1_fresnel_m1_modes2'
    S, free_prop, sg, M, loss = case_params(F, name)
    obj, pos, probes, meas = [F['%s/%s' % (name, k)] for k in ('obj', 'pos', 'probes', 'meas')]
    phys = O.Physics(probes.shape[-2:], ENERGY_EV, PSIZE_CM, free_prop_cm=free_prop, sign_convention=sg)
    a = PJ.forward_adjoint_object(obj.astype(np.float64), None, probes.astype(np.complex128), pos, meas, phys)
    b = O.forward_adjoint_object(obj.astype(np.float64), None, probes.astype(np.complex128), pos, meas, phys)
    for x, y in zip(a, b):
        assert np.array_equal(x, y)


def test_driver_first_gradient_matches_reference(F):
    """The first minibatch of the recorded driver run (rotation included) through the restatement."""
    par = ast.literal_eval(str(F['drv/params']))
    N, P = par['N'], par['P']
    theta_ls = np.linspace(0, np.pi, par['n_theta'], dtype='float32')
    task = F['drv/tasks_0_0']
    i_theta, ind = int(task[0, 0]), np.sort(task[:, 1])
    obj = np.stack([F['drv/guess_delta'], F['drv/guess_beta']], -1).astype(np.float64)
    probe = F['drv/probe_mag'] * np.exp(1j * F['drv/probe_phase'])
    phys = O.Physics((P, P), par['energy_ev'], par['psize_cm'], free_prop_cm=par['free_prop_cm'])
    pos = np.round(F['drv/pos']).astype(int)
    loss, _, g, _ = PJ.forward_adjoint_object(obj, O.rotation_coords((N, N, N), theta_ls[i_theta], 'float64'), probe, pos[ind],
                                              F['drv/prj'][i_theta, ind].astype(np.float64), phys)
    assert abs(loss / F['drv/fp64/losses'][0] - 1) < 1e-9
    assert rel(g, F['drv/first_grad']) < 1e-9
    assert len(F['drv/fp64/losses']) == par['n_epochs'] * par['n_theta'] * 3
    assert F['drv/voxels_off'][0] <= 1e-3 * F['drv/voxels_off'][1]


def test_the_sum_bar_catches_a_dropped_or_doubled_slice():
    """The bar of tests/test_gpu_projection_kernels.py, on the CPU: the exact sum passes it, float32 accumulation in a different
    order usually does not need to, and a sum that drops or doubles any one slice fails at nearly every element."""
    r = np.random.default_rng(25)
    for Z in (2, 7, 64, 257):
        v = PJ.mixed_values(r, (Z, 5, 37, 2))
        S, bar = PJ.z_sum_and_bar(v)
        good = S.astype(np.float32)
        assert np.all(np.abs(good.astype(np.float64) - S) <= bar)
        for z in (0, Z // 2, Z - 1):
            for sign in (-1., 1.):          # dropped, doubled
                bad = (S + sign * v[z].astype(np.float64)).astype(np.float32)
                miss = np.abs(bad.astype(np.float64) - S) > bar
                # an element passes only where that slice's value is below half an ulp of the sum: magnitudes span six decades
                assert miss.mean() > 0.5, (Z, z, sign, miss.mean())
                big = np.abs(v[z]) > 2. ** -22 * np.abs(S) + 2 * bar
                assert np.all(miss[big])
