"""tests/ctf_tomo_ref.py against golden F30 (the reference's rotation + modulate_and_get_ctf + autograd, fp64 and fp32), on the CPU:
the restatement's fp64 run reproduces the reference's to rounding, its float32 run stays within 3 x the reference's own float32
distance from fp64, and its inputs are the golden's bit for bit."""
import os

import numpy as np
import pytest

from tests import ctf_matrix as CM
from tests import ctf_tomo_ref as TR

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden', 'F30_ctf_tomo.npz')
rel = lambda a, b: float(np.linalg.norm(np.asarray(a, np.float64) - b) / np.linalg.norm(b))


@pytest.fixture(scope='module')
def F():
    return np.load(GOLDEN)


def test_the_golden_holds_every_case(F):
    assert list(F['model_cases']) == list(TR.CASES)
    assert os.path.getsize(GOLDEN) < os.path.getsize(os.path.join(os.path.dirname(GOLDEN), 'F29_multidist3d_affine.npz'))


def test_driver_part_inputs_first_loss_and_first_gradient(F):
    """Part (b), the reference's own driver: its inputs are ctf_tomo_ref.driver_inputs, bit for bit; the loss and the gradient of its
    first minibatch are the restatement's at that minibatch's angle; its own fp32 run is inside check_run's cap."""
    import ast
    from oracle import adorym_oracle as O
    par = ast.literal_eval(str(F['drv/params']))
    N, n_theta, nd = par['N'], par['n_theta'], par['n_dists']
    c = TR.driver_inputs(N, n_theta, nd)
    assert np.array_equal(c['obj'], F['drv/obj']) and np.array_equal(c['dists'], F['drv/dists'])
    assert F['drv/prj'].shape == (n_theta, nd, N, N) and float(F['drv/prj'].min()) >= CM.MIN_I
    it = int(F['drv/batches'][0])
    theta = np.linspace(0, np.pi, n_theta, dtype='float32')[it]
    case = dict(size=(N, N, N), theta=theta, obj=c['obj'], data=F['drv/prj'][it], dists=c['dists'], lg_kappa=np.float32(CM.LG_KAPPA), raw='intensity')
    r = TR.forward_adjoint(case, lg_kappa=float(CM.LG_KAPPA))
    assert abs(r['loss'] / F['drv/fp64/losses'][0] - 1) < 1e-12
    assert rel(r['grad'], F['drv/first_grad']) < 1e-12 and not F['drv/first_grad'][..., 1].any()
    assert len(F['drv/fp64/losses']) == len(F['drv/fp64/lg_kappa_trace']) == par['n_epochs'] * n_theta
    rmse, flipped, eloss, ok = F['drv/fp32_within_cap']
    assert ok == 1. and rmse < 1e-5 and flipped < 1e-3 and eloss < 1e-5
    assert np.array_equal(F['drv/fp64/beta'], c['obj'][..., 1].astype(np.float64))          # the reference leaves beta where it was


@pytest.mark.parametrize('name', list(TR.CASES))
def test_restatement_reproduces_the_reference(F, name):
    c = TR.inputs(name)
    for k in ('obj', 'data', 'dists'):
        assert np.array_equal(c[k], F['%s/%s' % (name, k)]), k
    r = TR.forward_adjoint(c)
    assert r['pred'].shape == (c['nd'],) + c['size'][:2]
    assert float(r['I'].min()) >= CM.MIN_I
    # fp64 against fp64: two evaluation orders of the same arithmetic (the gradient passes through four transforms and a scatter)
    assert rel(r['pred'], F[name + '/pred']) < 1e-14
    assert abs(r['loss'] / float(F[name + '/loss']) - 1) < 1e-13
    assert rel(r['grad'], F[name + '/grad']) < 1e-13
    assert not r['grad'][..., 1].any() and not F[name + '/grad'][..., 1].any()
    assert abs(r['gkappa'] / float(F[name + '/gkappa']) - 1) < 1e-12
    # float32 against the reference's float32: the 3x rule on its own distances from fp64
    s = TR.forward_adjoint(c, 'float32')
    e32 = F[name + '/err32']
    assert rel(s['pred'], F[name + '/pred']) <= 3 * e32[0]
    # (a scalar: the reference's own float32 distance is one draw, 3e-8 to 4e-7 over the cases; the bar the GPU's loss is held to)
    assert abs(s['loss'] / float(F[name + '/loss']) - 1) < CM.BARS['loss']
    assert rel(s['grad'][..., 0], F[name + '/grad'][..., 0]) <= 3 * e32[2]
    assert abs(s['gkappa'] / float(F[name + '/gkappa']) - 1) <= max(CM.BARS['gkappa'], 3 * e32[3])
