"""The NumPy restatement of multi-distance holography of a 3-D object (tests/multidist3d_ref.py) against golden F27, recorded from
the reference (tests/golden/gen_f27_multidist_3d.py).  CPU only.  The GPU tests use the restatement as the checker at launch
geometries the fixture does not hold; this file is what ties it to the reference.

Bars: those tests/test_sparse_ref_vs_golden.py uses for the same quantities in fp64 (prediction, loss 1e-12; gradients 1e-11; driver
losses 1e-9; a final object that went through TIFFs 2e-6).
"""
import ast
import os

import numpy as np
import pytest

from oracle import adorym_oracle as O      # checker only
from tests import multidist3d_ref as MR
from tests.ms_matrix import rel

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENERGY_EV, PSIZE_CM = 8000., 1e-6
CASES = ['m1_m1_intensity', 'm1_p1_magnitude', 'm2_m1_magnitude', 'm2_p1_intensity']


@pytest.fixture(scope='module')
def F():
    return np.load(os.path.join(ROOT, 'tests', 'golden', 'F27_multidist_3d.npz'))


def kernel_case(F, name):
    names = [str(n) for n in F['kernel_cases']]
    sg, M, rdt = ast.literal_eval(str(F['kernel_case_params'][names.index(name)]))
    c = {k: F['%s/%s' % (name, k)] for k in ('obj', 'pos', 'probes', 'meas')}
    c.update(sign_convention=sg, raw_data_type=rdt, dists=[float(d) for d in F['kernel_dists_cm']])
    return c


def run_ref(c, dtype):
    phys = O.Physics(c['probes'].shape[-2:], ENERGY_EV, PSIZE_CM, free_prop_cm=c['dists'][0], sign_convention=c['sign_convention'])
    return MR.forward_adjoint_object(c['obj'].astype(np.float64), None, c['probes'].astype(np.complex128), c['pos'], c['meas'], phys,
                                     c['dists'], dtype, raw_data_type=c['raw_data_type'])


def test_fixture_holds_the_cases():
    F_ = np.load(os.path.join(ROOT, 'tests', 'golden', 'F27_multidist_3d.npz'))
    assert sorted(str(n) for n in F_['kernel_cases']) == CASES
    par = [ast.literal_eval(str(p)) for p in F_['kernel_case_params']]
    assert {p[0] for p in par} == {1, -1} and {p[1] for p in par} == {1, 2} and {p[2] for p in par} == {'magnitude', 'intensity'}
    assert len(F_['kernel_dists_cm']) == 3
    c = kernel_case(F_, CASES[0])
    assert c['obj'].shape[2] == 5 and c['probes'].shape[-2:] == (12, 20) and c['meas'].shape[0] == 3 * len(c['pos'])
    assert os.path.getsize(os.path.join(ROOT, 'tests', 'golden', 'F27_multidist_3d.npz')) < 1 << 19


@pytest.mark.parametrize('name', CASES)
def test_restatement_matches_reference_fp64(F, name):
    loss, pred, g, gp = run_ref(kernel_case(F, name), 'float64')
    assert rel(pred, F[name + '/pred']) < 1e-12
    assert abs(loss - float(F[name + '/loss'])) <= 1e-12 * abs(float(F[name + '/loss']))
    assert rel(g, F[name + '/grad']) < 1e-11
    assert rel(gp, F[name + '/gprobe']) < 1e-11


@pytest.mark.parametrize('name', CASES)
def test_restatement_fp32_is_a_fair_yardstick(F, name):
    """The restatement's fp32 run is no further from fp64 than three times the reference's own fp32 run (plus 2^-24)."""
    c = kernel_case(F, name)
    (_, p64, g64, gp64), (_, p32, g32, gp32) = run_ref(c, 'float64'), run_ref(c, 'float32')
    e, eps = F[name + '/err32'], 2. ** -24
    assert rel(p32, p64) <= 3 * e[0] + eps
    assert rel(g32, g64) <= 3 * e[2] + eps
    assert rel(gp32, gp64) <= 3 * e[3] + eps


def test_fanout_equals_one_launch_per_distance(F):
    """What the restatement states: the D-entry evaluation is the mean of D single-distance evaluations of the oracle."""
    c = kernel_case(F, 'm2_m1_magnitude')
    loss, pred, g, gp = run_ref(c, 'float64')
    D, B = len(c['dists']), len(c['pos'])
    ls, gs, gps = [], [], []
    for d, dist in enumerate(c['dists']):
        phys = O.Physics(c['probes'].shape[-2:], ENERGY_EV, PSIZE_CM, free_prop_cm=dist, sign_convention=c['sign_convention'])
        l, p, gd, gpd = O.forward_adjoint_object(c['obj'].astype(np.float64), None, c['probes'].astype(np.complex128), c['pos'],
                                                 c['meas'][d::D], phys, 'float64')
        assert rel(p, pred[d::D]) < 1e-13
        ls.append(l), gs.append(gd), gps.append(gpd)
    assert abs(np.mean(ls) / loss - 1) < 1e-13
    assert rel(sum(gs) / D, g) < 1e-12 and rel(sum(gps) / D, gp) < 1e-12


# ------------------------------------------------------------------------------------------------------------ (b) the driver
def driver_inputs(F):
    par = ast.literal_eval(str(F['drv/params']))
    probe = F['drv/probe_mag'] * np.exp(1j * F['drv/probe_phase'])
    guess = [F['drv/guess_delta'].astype(np.float64), F['drv/guess_beta'].astype(np.float64)]
    phys = O.Physics(probe.shape, ENERGY_EV, PSIZE_CM, free_prop_cm=par['dists_cm'][0])
    theta_ls = np.linspace(0, np.pi, par['n_theta'], dtype='float32')
    return par, probe, guess, phys, theta_ls


def test_driver_restatement_matches_reference_fp64(F):
    par, probe, guess, phys, theta_ls = driver_inputs(F)
    out = MR.reconstruct(F['drv/prj'].astype(np.float64), guess, probe, phys, par['dists_cm'], theta_ls, n_epochs=par['n_epochs'],
                         learning_rate=par['learning_rate'])
    assert len(out['losses']) == par['n_epochs'] * par['n_theta']
    assert np.allclose(out['losses'], F['drv/fp64/losses'], rtol=1e-9, atol=0)
    x = F['drv/fp64/obj']
    assert np.abs(out['obj'] - x).max() < 2e-6 * np.abs(x).max()    # (the golden object went through TIFFs)


def test_driver_fixture_records_the_caps(F):
    n_off, n = F['drv/voxels_off']
    assert n_off <= 1e-3 * n
    assert 0 < float(F['drv/fp32/obj_err']) < 1e-2           # (in units of the update)
    assert np.allclose(F['drv/fp32/losses'], F['drv/fp64/losses'], rtol=1e-4, atol=0)


def test_task_lists_match_the_oracle(F):
    par = driver_inputs(F)[0]
    for i_epoch in range(par['n_epochs']):
        b = O.epoch_task_list(i_epoch, par['n_theta'], 1, 1, 1, 'immediate')
        for j, t in enumerate(b):
            assert np.array_equal(t, F['drv/tasks_%d_%d' % (i_epoch, j)])
