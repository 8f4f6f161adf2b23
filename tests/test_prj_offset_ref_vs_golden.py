"""CPU-only: the NumPy restatement of per-angle projection alignment (tests/prj_offset_ref.py) against the values recorded from
the reference (golden F24, tests/golden/gen_f24_prj_offset.py) and against a finite difference of itself.  The restatement is the
checker of the GPU tests (tests/test_gpu_prj_offset.py); this file is what ties it to the reference.

Bars: those tests/test_sparse_ref_vs_golden.py uses for the same quantities in fp64 (prediction, loss 1e-12; gradients, the shift
gradient included, 1e-11; driver losses 1e-9; a final object that went through fp32 TIFFs 2e-6).
"""
import ast
import os
import numpy as np
import pytest

from oracle import adorym_oracle as O
from tests import prj_offset_ref as PR

HERE = os.path.dirname(os.path.abspath(__file__))
ENERGY_EV, PSIZE_CM = 8000., 1e-6


@pytest.fixture(scope='module')
def F():
    return np.load(os.path.join(HERE, 'golden', 'F24_prj_offset.npz'))


def rel(a, b):
    a, b = np.asarray(a, np.complex128), np.asarray(b, np.complex128)
    return np.linalg.norm(a - b) / np.linalg.norm(b)


CASES = ['s3_fresnel_p1', 's3_fresnel_m1_modes2', 's1_fresnel', 's3_exit_wave', 's3_far_field', 's3_fresnel_real_imag']


def case_params(F, name):
    names = [str(n) for n in F['kernel_cases']]
    return ast.literal_eval(str(F['kernel_case_params'][names.index(name)]))       # S, unknown, free_prop, sign, modes


def run_ref(F, name, dtype='float64'):
    """The restatement on the inputs of fixture case ``name``: loss, pred, object gradient, probe gradient, dL/dshifts."""
    S, unknown, free_prop, sg, M = case_params(F, name)
    obj, pos, probes, shifts, index, meas = [F['%s/%s' % (name, k)] for k in ('obj', 'pos', 'probes', 'shifts', 'index', 'meas')]
    phys = O.Physics(probes.shape[-2:], ENERGY_EV, PSIZE_CM, free_prop_cm=free_prop, sign_convention=sg, unknown_type=unknown)
    return PR.forward_adjoint_object(obj.astype(np.float64), None, probes.astype(np.complex128), pos, meas, phys, shifts.astype(np.float64),
                                     index, dtype)


def test_fixture_lists_every_case(F):
    assert sorted(str(n) for n in F['kernel_cases']) == sorted(CASES)
    par = [case_params(F, n) for n in CASES]
    assert {p[0] for p in par} == {1, 3} and {p[1] for p in par} == {'delta_beta', 'real_imag'}
    assert {p[3] for p in par} == {1, -1} and {p[4] for p in par} == {1, 2}
    assert {'inf' if p[2] == 'inf' else ('none' if p[2] is None else 'fresnel') for p in par} == {'inf', 'none', 'fresnel'}
    for n in CASES:
        s, idx = F[n + '/shifts'], F[n + '/index']
        assert F[n + '/obj'].shape[:2] == (17, 27) and F[n + '/probes'].shape[1:] == (12, 20) and len(F[n + '/pos']) == 5
        assert len(set(idx.tolist())) < len(idx) and s.min() < -1 and s.max() > 1            # a shared entry, mixed signs


@pytest.mark.parametrize('name', CASES)
def test_restatement_matches_reference_fp64(F, name):
    loss, pred, g, gp, gs = run_ref(F, name)
    assert rel(pred, F[name + '/pred']) < 1e-12
    assert abs(loss - float(F[name + '/loss'])) <= 1e-12 * abs(float(F[name + '/loss']))
    assert rel(g, F[name + '/grad']) < 1e-11
    assert rel(gp, F[name + '/gprobe']) < 1e-11
    if case_params(F, name)[2] == 'inf':
        # a far-field magnitude does not see the offsets: exactly zero here, rounding noise beside the object gradient there
        assert np.all(gs == 0) and np.abs(F[name + '/gs']).max() < 1e-12 * np.abs(F[name + '/grad']).max()
    else:
        assert rel(gs, F[name + '/gs']) < 1e-11, (gs, F[name + '/gs'])


@pytest.mark.parametrize('name', [c for c in CASES if c != 's3_far_field'])
def test_restatement_fp32_is_a_fair_yardstick(F, name):
    """The GPU tests use the restatement's fp32 run as the yardstick at sizes the fixture does not hold: it must not be a laxer one
    than the reference's own fp32 run -- at most 3x as far from fp64."""
    l64, p64, g64, gp64, gs64 = run_ref(F, name)
    l32, p32, g32, gp32, gs32 = run_ref(F, name, 'float32')
    e = F[name + '/err32']
    assert e[4] < 1e-4                      # (the condition the generator puts on its inputs)
    assert rel(p32, p64) <= 3 * e[0]
    assert rel(g32, g64) <= 3 * e[2]
    assert rel(gp32, gp64) <= 3 * e[3]
    assert rel(gs32, gs64) <= 3 * e[4]


@pytest.mark.parametrize('unknown_type', ['delta_beta', 'real_imag'])
def test_zero_offsets_reproduce_the_pinned_oracle(unknown_type):
    r = np.random.default_rng(5)
    B, Py, Px, S, M = 3, 12, 10, 3, 2
    if unknown_type == 'delta_beta':
        tiles = np.stack([2e-3 * r.uniform(size=(B, Py, Px, S)), 2e-4 * r.uniform(size=(B, Py, Px, S))], -1)
    else:
        tiles = np.stack([1 + 0.1 * r.standard_normal((B, Py, Px, S)), 0.1 * r.standard_normal((B, Py, Px, S))], -1)
    probes = r.standard_normal((M, Py, Px)) + 1j * r.standard_normal((M, Py, Px))
    meas = r.uniform(size=(B, Py, Px)) * 20
    for free_prop, sg in (('inf', 1), (None, 1), (3e-3, -1)):
        phys = O.Physics((Py, Px), ENERGY_EV, PSIZE_CM, free_prop_cm=free_prop, sign_convention=sg, unknown_type=unknown_type)
        loss, pred, gt, gp, gs = PR.forward_adjoint_tiles(tiles, probes, meas, phys, np.zeros((B, 2)))
        lo, po, gto, gpo = O.forward_adjoint_tiles(tiles, probes, meas, phys)
        assert rel(pred, po) < 1e-12 and abs(loss - lo) <= 1e-12 * abs(lo)
        assert rel(gt, gto) < 1e-11 and rel(gp, gpo) < 1e-11


@pytest.mark.parametrize('unknown_type', ['delta_beta', 'real_imag'])
def test_shift_gradient_matches_finite_difference(unknown_type):
    """Central differences of the restatement's own loss in every offset (independent of the reference).  The loss depends on s
    through phases 2 PI f s with |f| <= 1/2: a step of h = 1e-5 px has a relative truncation error of (PI h)^2 / 6 ~ 2e-10, and the
    rounding error of the difference is 1e-16 * loss / (2 h |dL/ds|) ~ 1e-9.  Both are far below the 1e-6 asked for."""
    r = np.random.default_rng(6)
    B, Py, Px, S, M = 3, 10, 12, 2, 2
    if unknown_type == 'delta_beta':
        tiles = np.stack([2e-2 * r.uniform(size=(B, Py, Px, S)), 2e-3 * r.uniform(size=(B, Py, Px, S))], -1)
    else:
        tiles = np.stack([1 + 0.1 * r.standard_normal((B, Py, Px, S)), 0.1 * r.standard_normal((B, Py, Px, S))], -1)
    probes = r.standard_normal((M, Py, Px)) + 1j * r.standard_normal((M, Py, Px))
    meas = r.uniform(size=(B, Py, Px)) * 20
    shifts = np.array([[0.7, -1.3], [-0.2, 0.9]])
    index = np.array([0, 1, 0])
    for free_prop, sg in ((None, -1), (2e-4, 1), (2e-3, -1)):
        phys = O.Physics((Py, Px), ENERGY_EV, PSIZE_CM, free_prop_cm=free_prop, sign_convention=sg, unknown_type=unknown_type)
        gs = PR.forward_adjoint_tiles(tiles, probes, meas, phys, shifts, index)[4]
        h = 1e-5
        fd = np.zeros_like(shifts)
        for j in range(shifts.size):
            sp, sm = shifts.copy(), shifts.copy()
            sp.flat[j] += h
            sm.flat[j] -= h
            fd.flat[j] = (PR.forward_adjoint_tiles(tiles, probes, meas, phys, sp, index)[0]
                          - PR.forward_adjoint_tiles(tiles, probes, meas, phys, sm, index)[0]) / (2 * h)
        assert np.linalg.norm(gs) > 0 and rel(gs, fd) < 1e-6, (gs, fd)
    phys = O.Physics((Py, Px), ENERGY_EV, PSIZE_CM, free_prop_cm='inf', unknown_type=unknown_type)
    l0 = PR.forward_adjoint_tiles(tiles, probes, meas, phys, shifts, index)[0]
    assert PR.forward_adjoint_tiles(tiles, probes, meas, phys, shifts + 0.37, index)[0] == l0             # far field: no dependence


# ------------------------------------------------------------------------------------------------------------ (b) the driver
def driver_inputs(F):
    par = ast.literal_eval(str(F['drv/params']))
    probe = F['drv/probe_mag'] * np.exp(1j * F['drv/probe_phase'])
    guess = [F['drv/guess_delta'].astype(np.float64), F['drv/guess_beta'].astype(np.float64)]
    phys = O.Physics(probe.shape, ENERGY_EV, PSIZE_CM, free_prop_cm=par['free_prop_cm'])
    theta_ls = np.linspace(0, np.pi, par['n_theta'], dtype='float32')
    return par, probe, guess, phys, theta_ls


@pytest.mark.parametrize('run', ['gd', 'adam'])
def test_driver_restatement_matches_reference_fp64(F, run):
    par, probe, guess, phys, theta_ls = driver_inputs(F)
    out = PR.reconstruct(F['drv/prj'].astype(np.float64), guess, probe, np.zeros((1, 2)), phys, theta_ls, n_epochs=par['n_epochs'],
                         minibatch_size=1, learning_rate=par['learning_rate'], offset_optimizer=run,
                         prj_pos_offset_learning_rate=par['prj_pos_offset_learning_rate'] if run == 'gd' else par['adam_step'])
    tag = 'drv/%s_fp64/' % run
    assert np.allclose(out['losses'], F[tag + 'losses'], rtol=1e-9, atol=0)
    tr = F[tag + 'offset_trace']
    assert out['offset_history'].shape == tr.shape == (par['n_epochs'] * par['n_theta'], par['n_theta'], 2)
    assert np.abs(out['offset_history'] - tr).max() < 1e-9 * np.abs(tr).max()
    assert np.linalg.norm(tr[-1], axis=1).min() > 0.01              # every angle's offset has moved
    x = np.stack([F[tag + 'delta'], F[tag + 'beta']], -1)
    assert np.abs(out['obj'] - x).max() < 2e-6 * np.abs(x).max()    # (the golden object went through fp32 TIFFs)


def test_driver_fixture_records_the_caps(F):
    for t in ('gd', 'adam'):
        n_off, n = F['drv/%s_voxels_off' % t]
        assert n_off <= 1e-3 * n


def test_task_lists_match_the_oracle(F):
    par = driver_inputs(F)[0]
    for i_epoch in range(par['n_epochs']):
        b = O.epoch_task_list(i_epoch, par['n_theta'], 1, 1, 1, 'immediate')
        for j, t in enumerate(b):
            assert np.array_equal(t, F['drv/tasks_%d_%d' % (i_epoch, j)])


def test_recovery_step_reaches_the_truth_on_the_cpu():
    """The step of the GPU recovery test (tests/test_gpu_prj_offset_driver.py) is chosen HERE: the restatement's own gradient
    descent, the object held at the truth, comes within 0.02 px of offsets of +-0.5 px in 40 updates."""
    import sys
    sys.path.insert(0, os.path.join(HERE, 'golden'))
    import cases
    R = PR.RECOVERY
    truth, probe, theta_ls, phys, prj = PR.recovery_inputs(cases.smooth_field)
    out = PR.reconstruct(prj, [truth[..., 0], truth[..., 1]], probe, np.zeros((1, 2)), phys, theta_ls, n_epochs=R['n_epochs'], minibatch_size=1,
                         optimize_object=False, prj_pos_offset_learning_rate=R['step'])
    h = out['offset_history']
    assert len(h) == 40 and np.abs(h[-1] - np.array(R['true_offsets'])).max() < 0.02, h[-1]
