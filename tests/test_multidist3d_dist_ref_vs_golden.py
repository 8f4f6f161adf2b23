"""The NumPy restatement of multi-distance holography of a 3-D object with the distances as parameters
(tests/multidist3d_dist_ref.py) against golden F28, recorded from the reference with optimize_free_prop
(tests/golden/gen_f28_multidist3d_dist.py).  CPU only.  The GPU tests use the restatement as the checker at launch geometries the
fixture does not hold; this file is what ties it to the reference.

Bars: those of tests/test_multidist3d_ref_vs_golden.py in fp64 (prediction, loss 1e-12; gradients, dL/d free_prop_cm among them,
1e-11); the restatement's fp32 run under the 3x rule against the reference's own fp32 distance.
"""
import ast
import os

import numpy as np
import pytest

from oracle import adorym_oracle as O      # checker only
from tests import multidist3d_ref as MR
from tests import multidist3d_dist_ref as DR
from tests.ms_matrix import rel

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PATH = os.path.join(ROOT, 'tests', 'golden', 'F28_multidist3d_dist.npz')
ENERGY_EV, PSIZE_CM = 8000., 1e-6
CASES = ['m1_m1_intensity', 'm1_p1_magnitude', 'm2_m1_magnitude', 'm2_p1_intensity']


@pytest.fixture(scope='module')
def F():
    return np.load(PATH)


def kernel_case(F, name):
    names = [str(n) for n in F['kernel_cases']]
    sg, M, rdt = ast.literal_eval(str(F['kernel_case_params'][names.index(name)]))
    c = {k: F['%s/%s' % (name, k)] for k in ('obj', 'pos', 'probes', 'meas')}
    c.update(sign_convention=sg, raw_data_type=rdt, dists=[float(d) for d in F['kernel_dists_cm']])
    return c


def physics(c):
    return O.Physics(c['probes'].shape[-2:], ENERGY_EV, PSIZE_CM, free_prop_cm=c['dists'][0], sign_convention=c['sign_convention'])


def run_ref(c, dtype):
    """loss, pred, dL/d free_prop_cm, per-field terms"""
    return DR.forward_dist_grad_object(c['obj'].astype(np.float64), None, c['probes'].astype(np.complex128), c['pos'], c['meas'],
                                       physics(c), c['dists'], dtype, raw_data_type=c['raw_data_type'])


def test_fixture_holds_the_cases(F):
    assert sorted(str(n) for n in F['kernel_cases']) == CASES
    par = [ast.literal_eval(str(p)) for p in F['kernel_case_params']]
    assert {p[0] for p in par} == {1, -1} and {p[1] for p in par} == {1, 2} and {p[2] for p in par} == {'magnitude', 'intensity'}
    d, d0 = F['kernel_dists_cm'], F['kernel_data_dists_cm']
    assert len(d) == 3 and np.array_equal(d, d.astype(np.float32).astype(np.float64))        # float32-representable
    assert np.allclose(d / d0, (1.1, 0.92, 1.05), rtol=1e-6)                                 # the model is off the data's distances
    c = kernel_case(F, CASES[0])
    assert c['obj'].shape[2] == 5 and c['probes'].shape[-2:] == (12, 20) and c['meas'].shape[0] == 3 * len(c['pos'])
    for name in CASES:
        assert F[name + '/gdists'].shape == (3,) and F[name + '/err32'][4] < 1e-2, name     # the yardstick the generator asserted
    assert os.path.getsize(PATH) < 1 << 19


@pytest.mark.parametrize('name', CASES)
def test_restatement_matches_reference_fp64(F, name):
    c = kernel_case(F, name)
    loss, pred, gd, _ = run_ref(c, 'float64')
    assert rel(pred, F[name + '/pred']) < 1e-12
    assert abs(loss - float(F[name + '/loss'])) <= 1e-12 * abs(float(F[name + '/loss']))
    assert rel(gd, F[name + '/gdists']) < 1e-11
    # ... and the restatement it stands on gives the same loss, prediction, object and probe gradients at these distances
    l2, p2, g, gp = MR.forward_adjoint_object(c['obj'].astype(np.float64), None, c['probes'].astype(np.complex128), c['pos'], c['meas'],
                                              physics(c), c['dists'], 'float64', raw_data_type=c['raw_data_type'])
    assert rel(p2, F[name + '/pred']) < 1e-12 and abs(l2 - float(F[name + '/loss'])) <= 1e-12 * abs(float(F[name + '/loss']))
    assert rel(g, F[name + '/grad']) < 1e-11 and rel(gp, F[name + '/gprobe']) < 1e-11


@pytest.mark.parametrize('name', CASES)
def test_restatement_fp32_is_a_fair_yardstick(F, name):
    """The restatement's fp32 run is no further from fp64 than three times the reference's own fp32 run (plus 2^-24)."""
    c = kernel_case(F, name)
    (l64, p64, gd64, _), (l32, p32, gd32, _) = run_ref(c, 'float64'), run_ref(c, 'float32')
    e, eps = F[name + '/err32'], 2. ** -24
    assert rel(p32, p64) <= 3 * e[0] + eps
    assert abs(l32 / l64 - 1) <= 3 * e[1] + eps
    assert rel(gd32, gd64) <= 3 * e[4] + eps


@pytest.mark.parametrize('name', ['m2_m1_magnitude', 'm1_p1_magnitude'])
def test_gradient_is_the_sum_of_the_per_field_terms(F, name):
    """dL/dd of one launch = the sum over positions and modes of the per-field terms -- each of which is the gradient of the same
    launch's loss through that field alone: checked against a central difference of the loss in one distance."""
    c = kernel_case(F, name)
    loss, _, gd, terms = run_ref(c, 'float64')
    B, M, D = len(c['pos']), c['probes'].shape[0], len(c['dists'])
    assert terms.shape == (B, M, D)
    assert np.allclose(terms.sum(axis=(0, 1)), gd, rtol=1e-14, atol=0)
    # (float32-representable steps: the restatement rounds its distances)
    for d in range(D):
        lo, hi = np.array(c['dists'], np.float32), np.array(c['dists'], np.float32)
        for _ in range(64):
            lo[d], hi[d] = np.nextafter(lo[d], np.float32(0)), np.nextafter(hi[d], np.float32(1))
        fd = (run_ref(dict(c, dists=hi), 'float64')[0] - run_ref(dict(c, dists=lo), 'float64')[0]) / (float(hi[d]) - float(lo[d]))
        assert abs(fd / gd[d] - 1) < 1e-4, (d, fd, gd[d])


# ------------------------------------------------------------------------------------------------------------ (b) the driver
def test_driver_fixture(F):
    par = ast.literal_eval(str(F['drv/params']))
    n_up = par['n_epochs'] * par['n_theta']
    true, d0, tr = F['drv/dists_true_cm'], F['drv/dists0_cm'], F['drv/fp64/dists']
    assert par['n_epochs'] == 8 and par['free_prop_learning_rate'] == 2e-6 and par['learning_rate'] == 1e-10
    assert tr.shape == (n_up, 3) and F['drv/fp32/dists_err'].shape == (n_up, 3) and len(F['drv/fp64/losses']) == n_up
    assert np.allclose(d0 / true, (1.10, 0.92, 1.05), rtol=1e-6)
    # the reference ends at 0.14 - 0.17 of the starting errors; its fp32 run gives the same distances to 7 digits
    ratio = np.abs((tr[-1] - true) / (d0 - true))
    assert np.all(ratio > 0.1) and np.all(ratio < 0.2), ratio
    # (a float32 distance is rounded once per update: at most n_up half-ulps apart from the fp64 run if nothing amplifies them)
    assert np.all(F['drv/fp32/dists_err'] < n_up * 2. ** -24 * tr)
    assert np.allclose(F['drv/fp32/losses'], F['drv/fp64/losses'], rtol=1e-3, atol=0)
    # the object started at the truth and hardly moves at this step size
    x0 = np.stack([F['drv/guess_delta'], F['drv/guess_beta']], -1)
    assert np.abs(F['drv/fp64/obj'] - x0).max() <= n_up * par['learning_rate'] * 1.01 + 2e-6 * np.abs(x0).max()


def test_driver_first_step_follows_the_restatement(F):
    """The first update of the reference's run is one Adam step (no pin, no drift guard) on the restatement's dL/d free_prop_cm:
    distance d moves by the step size against the sign of its gradient."""
    par = ast.literal_eval(str(F['drv/params']))
    probe = F['drv/probe_mag'] * np.exp(1j * F['drv/probe_phase'])
    N = probe.shape[0]
    d0 = F['drv/dists0_cm']
    phys = O.Physics(probe.shape, ENERGY_EV, PSIZE_CM, free_prop_cm=d0[0])
    i_theta = int(F['drv/tasks_0_0'][0, 0])
    theta = np.linspace(0, np.pi, par['n_theta'], dtype='float32')[i_theta]
    obj = np.stack([F['drv/guess_delta'], F['drv/guess_beta']], -1).astype(np.float64)
    loss, _, gd, _ = DR.forward_dist_grad_object(obj, O.rotation_coords((N, N, N), theta, 'float64'), probe[None], np.zeros((1, 2), int),
                                                 F['drv/prj'][i_theta].astype(np.float64), phys, d0, 'float64')
    assert abs(loss / F['drv/fp64/losses'][0] - 1) < 1e-9
    x1, _, _ = O.adam_step(d0.copy(), gd, np.zeros(3), np.zeros(3), 0, step_size=par['free_prop_learning_rate'])
    assert np.allclose(x1, F['drv/fp64/dists'][0], rtol=1e-9, atol=0), (x1, F['drv/fp64/dists'][0])
