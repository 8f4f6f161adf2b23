"""The NumPy restatement of multi-distance holography of a 3-D object with the affine registration of the measured holograms
(tests/multidist3d_affine_ref.py) against golden F29, recorded from the reference with the data through w.affine_transform
(tests/golden/gen_f29_multidist3d_affine.py).  CPU only.  The GPU tests use the restatement as the checker at geometries, matrices
and data the fixture does not hold; this file is what ties it to the reference.

Bars: fp64 to 1e-10 (the project's usual pin; prediction, target and loss 1e-12); the restatement's fp32 run under the 3x rule against
the reference's own fp32 distance.  Matrix 0 of the fixture is the identity, where the sampling points sit on pixel centres and the
last bit of a coordinate decides which one-sided derivative is seen.  In float32 oracle.affine_sample reproduces torch's
coordinates to the rounding (its fused multiply-add is emulated exactly in float64) and the restatement is held to the reference's
own FLOAT32 gradient of matrix 0.  In float64 the emulation goes through long double, which is not exact, and on this 12 x 20 field
the restatement and torch land on different sides of some pixel centres: the fp64 gradient of matrix 0 is not pinned.  Nothing reads
it -- the reference pins matrix 0 to the identity, and the GPU computes in float32.
"""
import ast
import os

import numpy as np
import pytest

from oracle import adorym_oracle as O      # checker only
from tests import multidist3d_affine_ref as AR
from tests.ms_matrix import rel

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PATH = os.path.join(ROOT, 'tests', 'golden', 'F29_multidist3d_affine.npz')
ENERGY_EV, PSIZE_CM = 8000., 1e-6
CASES = ['m1_m1_intensity', 'm1_p1_magnitude', 'm2_m1_magnitude', 'm2_p1_intensity']
fro = lambda a: np.sqrt((np.asarray(a, np.float64) ** 2).sum(axis=(-2, -1)))


@pytest.fixture(scope='module')
def F():
    return np.load(PATH)


def kernel_case(F, name):
    names = [str(n) for n in F['kernel_cases']]
    sg, M, rdt = ast.literal_eval(str(F['kernel_case_params'][names.index(name)]))
    c = {k: F['%s/%s' % (name, k)] for k in ('obj', 'pos', 'probes', 'meas')}
    c.update(sign_convention=sg, raw_data_type=rdt, dists=[float(d) for d in F['kernel_dists_cm']], theta=F['kernel_theta'])
    return c


def run_ref(c, dtype):
    phys = O.Physics(c['probes'].shape[-2:], ENERGY_EV, PSIZE_CM, free_prop_cm=c['dists'][0], sign_convention=c['sign_convention'])
    return AR.forward_adjoint_object(c['obj'].astype(np.float64), None, c['probes'].astype(np.complex128), c['pos'], c['meas'], phys,
                                     c['dists'], c['theta'], dtype, raw_data_type=c['raw_data_type'])


def test_fixture_holds_the_cases(F):
    assert sorted(str(n) for n in F['kernel_cases']) == CASES
    par = [ast.literal_eval(str(p)) for p in F['kernel_case_params']]
    assert {p[0] for p in par} == {1, -1} and {p[1] for p in par} == {1, 2} and {p[2] for p in par} == {'magnitude', 'intensity'}
    th = F['kernel_theta']
    assert th.shape == (3, 2, 3) and np.array_equal(th, th.astype(np.float32).astype(np.float64))        # float32-representable
    assert np.array_equal(th[0], AR.IDENTITY) and np.all(fro(th[1:] - AR.IDENTITY) > 0.05)
    c = kernel_case(F, CASES[0])
    assert c['obj'].shape[2] == 5 and c['probes'].shape[-2:] == (12, 20) and c['meas'].shape[0] == 3 * len(c['pos'])
    for name in CASES:
        e = F[name + '/err32']
        assert F[name + '/gtheta'].shape == (3, 2, 3) and e[4] < 1e-2 and np.all(e[7:] < 1e-2), name     # the yardstick the generator asserted
        assert e[6] > 1e-2                  # ... and why matrix 0 has another: the reference's fp32 and fp64 runs disagree at the identity
    assert os.path.getsize(PATH) < 1 << 20


@pytest.mark.parametrize('name', CASES)
def test_restatement_matches_reference_fp64(F, name):
    c = kernel_case(F, name)
    r = run_ref(c, 'float64')
    assert rel(r['pred'], F[name + '/pred']) < 1e-12 and rel(r['target'], F[name + '/target']) < 1e-12
    assert abs(r['loss'] - float(F[name + '/loss'])) <= 1e-12 * abs(float(F[name + '/loss']))
    assert rel(r['grad'], F[name + '/grad']) < 1e-10 and rel(r['gprobe'], F[name + '/gprobe']) < 1e-10
    assert rel(r['gtheta'][1:], F[name + '/gtheta'][1:]) < 1e-10
    for d in (1, 2):
        assert rel(r['gtheta'][d], F[name + '/gtheta'][d]) < 1e-10, d
    # (matrix 0, the identity: pinned in float32 below -- see the module's docstring)


@pytest.mark.parametrize('name', CASES)
def test_restatement_fp32_is_a_fair_yardstick(F, name):
    """The restatement's fp32 run is no further from fp64 than three times the reference's own fp32 run (plus 2^-24); at the identity
    it reproduces the reference's own float32 gradient."""
    c = kernel_case(F, name)
    r64, r32 = run_ref(c, 'float64'), run_ref(c, 'float32')
    e, eps = F[name + '/err32'], 2. ** -24
    assert rel(r32['pred'], r64['pred']) <= 3 * e[0] + eps and rel(r32['target'], r64['target']) <= 3 * e[5] + eps
    assert abs(r32['loss'] / r64['loss'] - 1) <= 3 * e[1] + eps
    assert rel(r32['gtheta'][1:], r64['gtheta'][1:]) <= 3 * e[4] + eps
    assert rel(r32['gtheta'][0], F[name + '/gtheta32'][0]) < 1e-4


def test_matrix_gradient_is_the_derivative_of_the_loss(F):
    """Central differences of the restatement's fp64 loss in every entry of the free matrices (off the pixel centres the loss is
    differentiable)."""
    c = kernel_case(F, 'm1_p1_magnitude')
    g = run_ref(c, 'float64')['gtheta']
    h = 2. ** -23               # (float32-representable steps: the restatement rounds its matrices; small: a sampling point that
    #                             crosses a pixel centre between lo and hi changes its one-sided derivative)
    for d in (1, 2):
        for i in range(2):
            for j in range(3):
                lo, hi = c['theta'].copy(), c['theta'].copy()
                lo[d, i, j] -= h
                hi[d, i, j] += h
                lo, hi = AR.round32(lo), AR.round32(hi)
                fd = (run_ref(dict(c, theta=hi), 'float64')['loss'] - run_ref(dict(c, theta=lo), 'float64')['loss']) / (hi[d, i, j] - lo[d, i, j])
                assert abs(fd / g[d, i, j] - 1) < 2e-3, (d, i, j, fd, g[d, i, j])        # (the error falls with h: 1e-2 at 2^-20, 1.6e-3 at 2^-22)


def test_zero_samples_have_zero_cotangent():
    """Intensity data with a patch of exact zeros: 0/0 in the cotangent counts as 0 and everything stays finite."""
    r = np.random.default_rng(5)
    data = r.uniform(0.2, 1, (2, 12, 20))
    data[:, 3:9, 4:12] = 0
    theta = np.stack([AR.matrix(0.03, 1.04, (0.05, -0.03)), AR.matrix(-0.02, 0.97, (-0.04, 0.06))])
    pred = r.uniform(0.2, 1, data.shape)
    g = AR.affine_grad(data, theta, pred, 'intensity')
    samp, tgt = AR.register(data, theta, 'intensity')
    assert np.count_nonzero(samp == 0) > 20 and np.all(np.isfinite(g)) and np.all(g != 0)


# ------------------------------------------------------------------------------------------------------------ (b), (c) the driver
def test_driver_fixture(F):
    par = ast.literal_eval(str(F['drv/params']))
    n_up = par['n_epochs'] * par['n_theta']
    true, tr = F['drv/theta_true'], F['drv/fp64/theta']
    assert tr.shape == (n_up, 3, 2, 3) and F['drv/fp32/theta_err'].shape == tr.shape and len(F['drv/fp64/losses']) == n_up
    assert np.allclose(true, AR.inverse(F['drv/warp']), rtol=0, atol=1e-7) and np.array_equal(F['drv/warp'][0], AR.IDENTITY)
    assert np.array_equal(tr[:, 0], np.tile(AR.IDENTITY, (n_up, 1, 1)))                      # the pin of matrix 0
    ratio = fro(tr[-1] - true)[1:] / fro(AR.IDENTITY - true)[1:]
    assert np.all(ratio < 0.25), ratio                                                        # what the generator asserted
    assert F['drv/fp32/theta_err'].max() < 1e-5
    assert F['drv/fp64/losses'][-1] < 0.25 * F['drv/fp64/losses'][0]
    assert np.allclose(F['drv/fp32/losses'], F['drv/fp64/losses'], rtol=1e-3, atol=0)
    # the object started at the truth and hardly moves at this step size
    x0 = np.stack([F['drv/guess_delta'], F['drv/guess_beta']], -1)
    assert np.abs(F['drv/fp64/obj'] - x0).max() <= n_up * par['learning_rate'] * 1.01 + 2e-6 * np.abs(x0).max()
    both = ast.literal_eval(str(F['both/params']))
    n_b = both['n_epochs'] * both['n_theta']
    assert F['both/fp64/theta'].shape == (n_b, 3, 2, 3) and F['both/fp64/dists'].shape == (n_b, 3) and len(F['both/fp64/losses']) == n_b
    assert np.allclose(F['both/dists0_cm'] / F['drv/dists_true_cm'], both['dists_off'], rtol=1e-6)


def test_driver_first_step_follows_the_restatement(F):
    """The first update of the reference's run is one Adam step on the restatement's dL/dtheta at the identity -- in float64, where
    the restatement reproduces torch's coordinates to the rounding -- with matrix 0 put back to the identity."""
    par = ast.literal_eval(str(F['drv/params']))
    probe = F['drv/probe_mag'] * np.exp(1j * F['drv/probe_phase'])
    N = probe.shape[0]
    dists = list(par['dists_cm'])
    phys = O.Physics(probe.shape, ENERGY_EV, PSIZE_CM, free_prop_cm=dists[0])
    i_theta = int(F['drv/tasks_0_0'][0, 0])
    theta = np.linspace(0, np.pi, par['n_theta'], dtype='float32')[i_theta]
    obj = np.stack([F['drv/guess_delta'], F['drv/guess_beta']], -1).astype(np.float64)
    ident = np.tile(AR.IDENTITY, (3, 1, 1))
    r = AR.forward_adjoint_object(obj, O.rotation_coords((N, N, N), theta, 'float64'), probe[None], np.zeros((1, 2), int),
                                  F['drv/prj'][i_theta].astype(np.float64), phys, dists, ident, 'float64')
    assert abs(r['loss'] / F['drv/fp64/losses'][0] - 1) < 1e-9
    x1, _, _ = O.adam_step(ident.copy(), r['gtheta'], np.zeros_like(ident), np.zeros_like(ident), 0, step_size=par['prj_affine_learning_rate'])
    x1[0] = AR.IDENTITY
    assert np.allclose(x1, F['drv/fp64/theta'][0], rtol=0, atol=1e-9), (x1, F['drv/fp64/theta'][0])
