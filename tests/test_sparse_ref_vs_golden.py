"""CPU-only: the NumPy restatement of sparse multislice (tests/sparse_ref.py) against the values recorded from the reference
(golden F21, tests/golden/gen_f21_sparse.py), against the pinned oracle where the two models coincide, and against a finite
difference of itself.  The restatement is the checker of the GPU tests (tests/test_gpu_sparse_multislice.py); this file is what
ties it to the reference.

Bars: those tests/test_oracle_vs_golden.py uses for the same quantities in fp64 (prediction, loss 1e-12; gradients 1e-11; driver
losses 1e-9; a final object that went through fp32 mag / phase TIFFs 2e-6).  dL/dz has no sibling: it is a sum of Py*Px*B*M terms
of both signs with phases a*d of up to ~60 rad, which costs three to four digits of the 1e-16 of fp64 -- 1e-10, relative to the
norm of the vector.
"""
import ast
import os
import numpy as np
import pytest

from oracle import adorym_oracle as O
from tests import sparse_ref as SR

HERE = os.path.dirname(os.path.abspath(__file__))
ENERGY_EV, PSIZE_CM = 8000., 1e-6


@pytest.fixture(scope='module')
def F():
    return np.load(os.path.join(HERE, 'golden', 'F21_sparse_multislice.npz'))


def rel(a, b):
    a, b = np.asarray(a, np.complex128), np.asarray(b, np.complex128)
    return np.linalg.norm(a - b) / np.linalg.norm(b)


CASES = ['s2_db_far_p1_m1', 's2_ri_none_m1_m2', 's3_db_fresnel_m1_m2', 's3_ri_far_m1_m1', 's3_db_none_p1_m1', 's3_ri_far_p1_m2',
         's5_ri_fresnel_p1_m1', 's5_db_far_m1_m2']


def case_params(F, name):
    names = [str(n) for n in F['kernel_cases']]
    S, unknown, free_prop, sg, M = ast.literal_eval(str(F['kernel_case_params'][names.index(name)]))
    return S, unknown, free_prop, sg, M


def run_ref(F, name, dtype='float64'):
    """The restatement on the inputs of fixture case ``name``: loss, pred, object gradient, probe gradient, dL/dz."""
    S, unknown, free_prop, sg, M = case_params(F, name)
    obj, pos, probes, z, meas = [F['%s/%s' % (name, k)] for k in ('obj', 'pos', 'probes', 'z', 'meas')]
    phys = O.Physics(probes.shape[-2:], ENERGY_EV, PSIZE_CM, free_prop_cm=free_prop, sign_convention=sg, unknown_type=unknown)
    return SR.forward_adjoint_object(obj.astype(np.float64), None, probes.astype(np.complex128), pos, meas, phys, z.astype(np.float64), dtype)


def test_fixture_lists_every_case(F):
    assert sorted(str(n) for n in F['kernel_cases']) == sorted(CASES)
    par = [case_params(F, n) for n in CASES]
    assert {p[0] for p in par} == {2, 3, 5} and {p[1] for p in par} == {'delta_beta', 'real_imag'}
    assert {p[3] for p in par} == {1, -1} and {p[4] for p in par} == {1, 2}
    assert {'inf' if p[2] == 'inf' else ('none' if p[2] is None else 'fresnel') for p in par} == {'inf', 'none', 'fresnel'}


@pytest.mark.parametrize('name', CASES)
def test_restatement_matches_reference_fp64(F, name):
    loss, pred, g, gp, gz = run_ref(F, name)
    assert rel(pred, F[name + '/pred']) < 1e-12
    assert abs(loss - float(F[name + '/loss'])) <= 1e-12 * abs(float(F[name + '/loss']))
    assert rel(g, F[name + '/grad']) < 1e-11
    assert rel(gp, F[name + '/gprobe']) < 1e-11
    assert rel(gz, F[name + '/gz']) < 1e-10, (gz, F[name + '/gz'])
    assert abs(gz.sum()) < 1e-9 * np.abs(gz).sum()                  # only the gaps matter


@pytest.mark.parametrize('name', CASES)
def test_restatement_fp32_is_a_fair_yardstick(F, name):
    """The GPU tests use the restatement's fp32 run as a floor (and, at sizes the fixture does not hold, as the yardstick): it must
    not be a laxer yardstick than the reference's own fp32 run -- at most 3x as far from fp64, plus the resolution of fp32 itself
    (2^-23 = 1.2e-7)."""
    l64, p64, g64, gp64, gz64 = run_ref(F, name)
    l32, p32, g32, gp32, gz32 = run_ref(F, name, 'float32')
    e = F[name + '/err32']
    eps = 2. ** -23
    assert rel(p32, p64) <= 3 * e[0] + eps
    assert rel(g32, g64) <= 3 * e[2] + eps
    assert rel(gp32, gp64) <= 3 * e[3] + eps
    assert rel(gz32, gz64) <= 3 * e[4] + eps


@pytest.mark.parametrize('unknown_type', ['delta_beta', 'real_imag'])
def test_equal_gaps_of_one_voxel_reproduce_the_pinned_oracle(unknown_type):
    """With z_s = s * voxel every gap's kernel is the dense path's H: loss, prediction, tile and probe gradients of
    O.forward_adjoint_tiles(binning = 1)."""
    r = np.random.default_rng(5)
    B, Py, Px, S, M = 3, 12, 10, 4, 2
    if unknown_type == 'delta_beta':
        tiles = np.stack([2e-3 * r.uniform(size=(B, Py, Px, S)), 2e-4 * r.uniform(size=(B, Py, Px, S))], -1)
    else:
        tiles = np.stack([1 + 0.1 * r.standard_normal((B, Py, Px, S)), 0.1 * r.standard_normal((B, Py, Px, S))], -1)
    probes = r.standard_normal((M, Py, Px)) + 1j * r.standard_normal((M, Py, Px))
    meas = r.uniform(size=(B, Py, Px)) * 20
    for free_prop, sg in (('inf', 1), ('inf', -1), (None, 1), (3e-3, -1)):
        phys = O.Physics((Py, Px), ENERGY_EV, PSIZE_CM, free_prop_cm=free_prop, sign_convention=sg, unknown_type=unknown_type)
        z = np.arange(S) * PSIZE_CM
        loss, pred, gt, gp, gz = SR.forward_adjoint_tiles(tiles, probes, meas, phys, z)
        lo, po, gto, gpo = O.forward_adjoint_tiles(tiles, probes, meas, phys)
        assert rel(pred, po) < 1e-12 and abs(loss - lo) <= 1e-12 * abs(lo)
        assert rel(gt, gto) < 1e-11 and rel(gp, gpo) < 1e-11


@pytest.mark.parametrize('unknown_type', ['delta_beta', 'real_imag'])
def test_slice_position_gradient_matches_finite_difference(unknown_type):
    """Central differences of the restatement's own loss in every z_j (independent of the reference).  The loss depends on z
    through phases a_k d with |a_k| up to PI * lambda * (u^2 + v^2) = 2.4e-3 rad / nm here (intensities: differences of two, 4.9e-3),
    so a step of h = 1e-8 cm = 0.1 nm has a relative truncation error of (4.9e-4)^2 / 6 = 4e-8; the rounding error of the
    difference is 1e-16 * loss / (2 h |dL/dz|) ~ 1e-9.  Both are far below the 1e-6 asked for."""
    r = np.random.default_rng(6)
    B, Py, Px, S, M = 2, 10, 12, 3, 2
    if unknown_type == 'delta_beta':
        tiles = np.stack([2e-2 * r.uniform(size=(B, Py, Px, S)), 2e-3 * r.uniform(size=(B, Py, Px, S))], -1)
    else:
        tiles = np.stack([1 + 0.1 * r.standard_normal((B, Py, Px, S)), 0.1 * r.standard_normal((B, Py, Px, S))], -1)
    probes = r.standard_normal((M, Py, Px)) + 1j * r.standard_normal((M, Py, Px))
    meas = r.uniform(size=(B, Py, Px)) * 20
    z = np.array([0., 10e-4, 35e-4])
    for free_prop, sg in (('inf', 1), (None, -1), (2e-3, 1)):
        phys = O.Physics((Py, Px), ENERGY_EV, PSIZE_CM, free_prop_cm=free_prop, sign_convention=sg, unknown_type=unknown_type)
        gz = SR.forward_adjoint_tiles(tiles, probes, meas, phys, z)[4]
        h = 1e-8
        fd = np.zeros(S)
        for j in range(S):
            zp, zm = z.copy(), z.copy()
            zp[j] += h
            zm[j] -= h
            fd[j] = (SR.forward_adjoint_tiles(tiles, probes, meas, phys, zp, want_grad=False)[0]
                     - SR.forward_adjoint_tiles(tiles, probes, meas, phys, zm, want_grad=False)[0]) / (2 * h)
        assert np.linalg.norm(gz) > 0 and rel(gz, fd) < 1e-6, (gz, fd)


# ------------------------------------------------------------------------------------------------------------ (b) the driver
def driver_inputs(F):
    par = ast.literal_eval(str(F['drv/params']))
    probe = F['drv/probe_mag'] * np.exp(1j * F['drv/probe_phase'])
    gm, gp = F['drv/guess_mag'].astype(np.float64), F['drv/guess_phase'].astype(np.float64)
    guess = [gm * np.cos(gp), gm * np.sin(gp)]
    phys = O.Physics(probe.shape, ENERGY_EV, PSIZE_CM, unknown_type='real_imag')
    return par, probe, guess, phys


@pytest.mark.parametrize('run', ['zfix', 'zopt'])
def test_driver_restatement_matches_reference_fp64(F, run):
    par, probe, guess, phys = driver_inputs(F)
    out = SR.reconstruct(F['drv/prj'].astype(np.float64), guess, probe, F['drv/pos'], phys, par['z0'], n_epochs=par['n_epochs'],
                         minibatch_size=par['minibatch_size'], learning_rate=par['learning_rate'], optimize_probe=True,
                         probe_learning_rate=par['probe_learning_rate'], optimize_slice_pos=run == 'zopt',
                         slice_pos_learning_rate=par['slice_pos_learning_rate'])
    tag = 'drv/%s_fp64/' % run
    assert np.allclose(out['losses'], F[tag + 'losses'], rtol=1e-9, atol=0)
    if run == 'zopt':
        assert out['z_history'].shape == F[tag + 'z_trace'].shape
        assert np.abs(out['z_history'] - F[tag + 'z_trace']).max() < 1e-9 * np.abs(F[tag + 'z_trace']).max()
        assert np.all(out['z_history'][:, 0] == 0)
    else:
        assert np.array_equal(out['z'], np.array(par['z0']))
    ref = F[tag + 'mag'] * np.exp(1j * F[tag + 'phase'])
    x = out['obj'][..., 0] + 1j * out['obj'][..., 1]
    assert np.abs(x - ref).max() < 2e-6                           # (the golden object went through mag / phase TIFFs)
    pref = F[tag + 'probe_mag_ds_1'] * np.exp(1j * F[tag + 'probe_phase_ds_1'])
    assert np.abs(out['probes'] - pref).max() < 2e-6 * np.abs(pref).max()


def test_driver_fixture_records_the_caps(F):
    """The reference's own fp32 run stays inside the caps the GPU tests may use: at most 1e-3 of the voxels more than one Adam
    step from the fp64 run, and no slice position."""
    for t in ('zfix', 'zopt'):
        n_off, n = F['drv/%s_voxels_off' % t]
        assert n_off <= 1e-3 * n
    assert int(F['drv/z_off'][0]) == 0


def test_task_lists_match_the_oracle(F):
    par, _, _, _ = driver_inputs(F)
    for i_epoch in range(par['n_epochs']):
        b = O.epoch_task_list(i_epoch, 1, len(F['drv/pos']), par['minibatch_size'], 1, 'immediate', two_d_mode=True)
        for j, t in enumerate(b):
            assert np.array_equal(t, F['drv/tasks_%d_%d' % (i_epoch, j)])
