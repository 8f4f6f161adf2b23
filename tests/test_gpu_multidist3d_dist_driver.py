"""Refined detector distances of a 3-D object (holotomography with optimize_free_prop) through MultiDistModel and
reconstruct_ptychography(..., fanout_free_prop=True) on the GPU (pytest -m gpu).

Checkers: golden F28 (the reference driver with optimize_free_prop in fp64, its own fp32 run as the yardstick;
tests/golden/gen_f28_multidist3d_dist.py) and the NumPy restatement tests/multidist3d_dist_ref.py.
"""
import ast
import os

import numpy as np
import pytest

from tests import ms_matrix as MM
from tests import multidist3d_dist_ref as DR
from tests.test_gpu_multidist3d_driver import _drv_kw
from oracle import adorym_oracle as O      # checker only
import cases

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENERGY_EV, PSIZE_CM = 8000., 1e-6
BARS = MM.GENERIC
rel = MM.rel


@pytest.fixture(scope='module')
def A():
    import adorym_amd
    return adorym_amd


@pytest.fixture(scope='module')
def F():
    return np.load(os.path.join(ROOT, 'tests', 'golden', 'F28_multidist3d_dist.npz'))


def _drv_inputs(F):
    par = ast.literal_eval(str(F['drv/params']))
    N = par['N']
    kw = dict(fname=F['drv/prj'], obj_size=(N, N, N), probe_pos=np.array([(0., 0.)]), n_theta=par['n_theta'],
              free_prop_cm=np.array(F['drv/dists0_cm']), minibatch_size=1, n_epochs=par['n_epochs'], learning_rate=par['learning_rate'],
              initial_guess=[F['drv/guess_delta'].astype(np.float64), F['drv/guess_beta'].astype(np.float64)], probe_type='supplied',
              probe_initial=[F['drv/probe_mag'], F['drv/probe_phase']], two_d_mode=False, optimize_free_prop=True,
              free_prop_learning_rate=par['free_prop_learning_rate'], fanout_free_prop=True)
    return par, kw


# ------------------------------------------------------------------------------------------------------------ the model
def test_model_returns_the_distance_gradient(A, F):
    """MultiDistModel on a 3-D object with an engine built with refine_distances=True (16^3, D = 3, the rotation of angle 2):
    loss_and_gradients([0, i_fp]) returns dL/d free_prop_cm at that argument's place, the restatement's under the 3x rule with its
    own fp32 run as the yardstick; predict and the loss function read the distances from the device array."""
    par, _ = _drv_inputs(F)
    N, n_theta, dists = par['N'], par['n_theta'], [float(d) for d in F['drv/dists0_cm']]
    ctx = A.Context(0)
    eng = A.MultisliceEngine(ctx, (N, N, N), (N, N), np.zeros((1, 2)), ENERGY_EV, PSIZE_CM, free_prop_cm=dists, max_batch=1, streamed=True,
                             detector_fanout=True, refine_distances=True)
    theta_ls = np.linspace(0, np.pi, n_theta, dtype='float32')
    tables = {}
    cv = dict(engine=eng, holo_engine=None, prj=F['drv/prj'], two_d_mode=False, theta_ls=theta_ls, forward_algorithm='fresnel',
              optimize_free_prop=True, rotation_tables=lambda i: tables.setdefault(i, A.RotationTable(ctx, (N, N, N), theta_ls[i])))
    fm = A.MultiDistModel(device=ctx, common_vars_dict=cv)
    obj = np.stack([F['drv/guess_delta'], F['drv/guess_beta']], -1).astype(np.float32)
    probe = F['drv/probe_mag'] * np.exp(1j * F['drv/probe_phase'])
    i_theta = 2
    i_fp = fm.get_argument_index('free_prop_cm')
    args = (ctx.array(obj), probe.real[None], probe.imag[None], 0., None, i_theta, np.zeros((1, 2), int), None, np.zeros((len(dists), 2)),
            np.array([0]), eng.dists, 0, None, None, None)
    grad = ctx.zeros(obj.shape)
    out = fm.loss_and_gradients([0, i_fp], grad, *args)
    loss = fm.current_loss
    assert out[0] is grad and out[1].shape == (len(dists),)
    gd = out[1].get().astype(np.float64)
    phys = O.Physics((N, N), ENERGY_EV, PSIZE_CM, free_prop_cm=dists[0])
    ref = {dt: DR.forward_dist_grad_object(obj.astype(np.float64), O.rotation_coords((N, N, N), theta_ls[i_theta], dt), probe[None],
                                           np.zeros((1, 2), int), F['drv/prj'][i_theta].astype(np.float64), phys, dists, dt)
           for dt in ('float64', 'float32')}
    l64, p64, gd64, _ = ref['float64']
    e, e32 = rel(gd, gd64), rel(ref['float32'][2], gd64)
    print('model: loss %.2e  dL/dd %.2e (fp32 restatement %.2e)' % (abs(loss / l64 - 1), e, e32), gd, gd64)
    assert abs(loss / l64 - 1) <= BARS['loss']
    assert e < BARS['grad'] and e <= 3 * e32 + BARS['grad_abs'], (e, e32)
    # the distances are read from the device array: after a change (and dists_changed) prediction and loss follow
    pred = fm.predict(*args)
    assert rel(pred, p64) < BARS['pred'] and fm.get_loss_function()(*args) == loss
    true = [float(d) for d in F['drv/dists_true_cm']]
    eng.dists.set(np.asarray(true, np.float32))
    eng.dists_changed()
    p_true = DR.forward_dist_grad_object(obj.astype(np.float64), O.rotation_coords((N, N, N), theta_ls[i_theta], 'float64'), probe[None],
                                         np.zeros((1, 2), int), F['drv/prj'][i_theta].astype(np.float64), phys, true, 'float64')[1]
    assert rel(fm.predict(*args), p_true) < BARS['pred'] and rel(p64, p_true) > 1e-3
    assert fm.get_loss_function()(*args) < 1e-3 * loss          # (the object is the truth: at the true distances the data are met)
    # a foreign device array in the place of free_prop_cm is refused
    with pytest.raises(ValueError, match="must be the engine's own array"):
        fm.predict(*(args[:10] + (ctx.zeros((len(dists),)),) + args[11:]))
    # what stays refused with such an engine
    for extra, what in ((dict(optimize_prj_affine=True), 'optimize_prj_affine'), (dict(optimize_all_probe_pos=True), 'optimize_all_probe_pos'),
                        (dict(rotate_out_of_loop=True), 'rotate_out_of_loop')):
        m = A.MultiDistModel(device=ctx, common_vars_dict=dict(cv, **extra))
        with pytest.raises(NotImplementedError, match='3-D object with %s' % what):
            m._check(0, None, np.zeros((len(dists), 2)))
    eng.plan.close()
    ctx.close()


# ------------------------------------------------------------------------------------------------------------ the driver
def test_driver_vs_reference(A, F, tmp_path):
    """reconstruct_ptychography(optimize_free_prop=True, fanout_free_prop=True) on the F28 driver case (16^3 object started at the
    truth, 4 angles, D = 3 started at truth * (1.10, 0.92, 1.05), 8 epochs, Adam on the distances with step 2e-6).

    Losses: rtol = max(2e-4, 3 * the reference's own fp32 deviation).  The distances after every update against the reference's
    fp64 run: 3 * the largest relative deviation of the reference's own fp32 run over the history, plus one float32 ulp (2^-23) of
    the distance.  Every final distance error is below 1/3 of its starting error (the reference reaches 0.14 - 0.17)."""
    par, kw = _drv_inputs(F)
    st = A.reconstruct_ptychography(**_drv_kw(tmp_path, **kw))
    l64, l32 = F['drv/fp64/losses'], F['drv/fp32/losses']
    n_up = par['n_epochs'] * par['n_theta']
    assert len(st['losses']) == len(l64) == n_up
    e_l = np.abs(np.asarray(st['losses']) / l64 - 1).max()
    print('losses: worst %.2e (fp32 ref %.2e)' % (e_l, np.abs(l32 / l64 - 1).max()))
    assert np.allclose(st['losses'], l64, rtol=max(2e-4, 3 * np.abs(l32 / l64 - 1).max()))
    h64 = F['drv/fp64/dists']
    hist = np.asarray(st['free_prop_cm_history'], np.float64)
    assert hist.shape == h64.shape == (n_up, 3)
    dev32 = (F['drv/fp32/dists_err'] / h64).max()
    e_h = np.abs(hist / h64 - 1).max()
    print('distance history: worst %.2e (fp32 ref %.2e)' % (e_h, dev32), hist[-1], h64[-1])
    assert e_h <= 3 * dev32 + 2. ** -23, (e_h, dev32)
    final = np.asarray(st['free_prop_cm'], np.float64).reshape(-1)
    assert np.array_equal(final.astype(np.float32), hist[-1].astype(np.float32))
    true, d0 = F['drv/dists_true_cm'], F['drv/dists0_cm']
    ratio = np.abs((final - true) / (d0 - true))
    print('final distance errors / starting errors', ratio)
    assert np.all(ratio < 1. / 3), ratio
    assert st['engine_streamed'] is True


def test_checkpoint_resume_gives_the_same_distances(A, F, tmp_path):
    """A run stopped after its first epoch and resumed from its last checkpoint (epoch 0, batch 3) replays that minibatch and the
    second epoch: the distances travel in the checkpoint under the reference's key free_prop_cm (their optimiser's moments beside
    them), the table is rebuilt from them, and the losses of the replayed minibatches and the final distances are the
    uninterrupted run's bit for bit."""
    import pickle
    par, kw = _drv_inputs(F)
    kw = dict(kw, n_epochs=2)
    n = par['n_theta']
    whole = A.reconstruct_ptychography(**_drv_kw(tmp_path, output_folder='whole', **kw))
    common = dict(store_checkpoint=True, n_batch_per_checkpoint=1, output_folder='part')
    A.reconstruct_ptychography(**_drv_kw(tmp_path, **dict(kw, n_epochs=1, **common)))
    ck = os.path.join(str(tmp_path), 'part', 'checkpoint')
    assert [int(v) for v in np.loadtxt(os.path.join(ck, 'checkpoint.txt'))] == [0, n - 1]
    with open(os.path.join(ck, 'params_0'), 'rb') as f:
        saved = pickle.load(f)
    assert np.array_equal(np.asarray(saved['free_prop_cm'], np.float32), whole['free_prop_cm_history'][n - 2].astype(np.float32))
    res = A.reconstruct_ptychography(**_drv_kw(tmp_path, **dict(kw, use_checkpoint=True, **common)))
    assert len(res['losses']) == 1 + n
    assert np.array_equal(res['losses'], whole['losses'][n - 1:])
    assert np.array_equal(res['free_prop_cm'], whole['free_prop_cm'])
    assert np.array_equal(res['free_prop_cm_history'], whole['free_prop_cm_history'][n - 1:])
    assert np.abs(np.asarray(whole['free_prop_cm'], np.float64).reshape(-1) - F['drv/dists0_cm']).max() > 1e-6


def test_driver_refusals(A, tmp_path):
    N, D = 16, 2
    prj = np.ones((2, D, N, N), np.float32)
    guess = [np.zeros((N, N, 4)), np.zeros((N, N, 4))]
    kw = _drv_kw(tmp_path, fname=prj, obj_size=(N, N, 4), probe_pos=np.array([(0., 0.)]), probe_type='plane', initial_guess=guess, n_epochs=1,
                 minibatch_size=1, n_theta=2, free_prop_cm=[1e-4, 2e-4], two_d_mode=False, optimize_free_prop=True)
    what = 'multi-distance holography of a 3-D object with %s'
    # without the keyword: the refusal as it was
    with pytest.raises(NotImplementedError, match=what % 'optimize_free_prop'):
        A.reconstruct_ptychography(**kw)
    # with it, what else a 3-D object refuses stays refused
    for extra, name in ((dict(optimize_prj_affine=True), 'optimize_prj_affine'), (dict(optimize_all_probe_pos=True), 'optimize_all_probe_pos'),
                        (dict(rotate_out_of_loop=True), 'rotate_out_of_loop'), (dict(unknown_type='real_imag'), "unknown_type='real_imag'"),
                        (dict(safe_zone_width=2), 'data divided into sub-tiles or safe_zone_width > 0')):
        with pytest.raises(NotImplementedError, match=what % name):
            A.reconstruct_ptychography(**dict(kw, fanout_free_prop=True, **extra))
    with pytest.raises(NotImplementedError, match="forward_algorithm='ctf' with two_d_mode=False"):
        A.reconstruct_ptychography(**dict(kw, fanout_free_prop=True, forward_algorithm='ctf', ctf_lg_kappa=1.7))
    # the keyword alone (no optimize_free_prop) changes nothing: the host-table engine
    st = A.reconstruct_ptychography(**dict(kw, optimize_free_prop=False, fanout_free_prop=True))
    assert st['free_prop_cm_history'] is None and np.all(np.isfinite(st['losses']))


def test_2d_multidistance_keeps_the_holography_engine(A, tmp_path, monkeypatch):
    """The 2-D multi-distance run of golden F12 (config 5, optimize_free_prop) still takes HolographyEngine, with or without the
    keyword: holo_engine is set, no fan-out plan is built and no distances are handed to a plan."""
    from adorym_amd import ptychography as PT
    from adorym_amd.device import Plan
    from adorym_amd.propagate import MultisliceEngine
    f = np.load(os.path.join(ROOT, 'tests', 'golden', 'F12_multidist.npz'))
    Cc = cases.C5MINI
    inp = cases.c5mini_inputs()
    N = Cc['N']
    seen = {'fanout': 0, 'changed': 0, 'runs': []}
    orig_fan, orig_model, orig_changed = Plan.set_detector_fanout, PT._Run.create_forward_model, MultisliceEngine.dists_changed

    def count_fanout(self, kernels):
        seen['fanout'] += 1
        return orig_fan(self, kernels)

    def count_changed(self):
        seen['changed'] += 1
        return orig_changed(self)

    def spy(self):
        seen['runs'].append((self.holo_engine, self.engine))
        return orig_model(self)
    monkeypatch.setattr(Plan, 'set_detector_fanout', count_fanout)
    monkeypatch.setattr(MultisliceEngine, 'dists_changed', count_changed)
    monkeypatch.setattr(PT._Run, 'create_forward_model', spy)
    st = A.reconstruct_ptychography(
        fname=f['data'][None], obj_size=(N, N, 1), probe_pos=np.array([[0., 0.]]), theta_st=0, theta_end=0, n_theta=1, two_d_mode=True,
        energy_ev=Cc['energy_ev'], psize_cm=Cc['psize_cm'], free_prop_cm=np.array(inp['dists_guess']), minibatch_size=1, n_epochs=4,
        initial_guess=[inp['guess'][0], inp['guess'][1]], probe_type='plane', raw_data_type='intensity', unknown_type='real_imag',
        gamma=0, alpha_d=0, alpha_b=0, optimizer='adam', learning_rate=1e-2, optimize_free_prop=True, free_prop_learning_rate=1e-1,
        optimize_prj_affine=True, prj_affine_learning_rate=1e-3, n_dp_batch=1, randomize_probe_pos=True, save_path=str(tmp_path),
        output_folder='c5', store_checkpoint=False, use_checkpoint=False, return_state=True, fanout_free_prop=True)
    (holo, eng), = seen['runs']
    assert isinstance(holo, A.HolographyEngine) and not eng.detector_fanout and seen['fanout'] == 0 and seen['changed'] == 0
    assert st['free_prop_cm_history'] is None
    assert np.allclose(st['losses'], f['e2e_losses_64'], rtol=2e-3)       # (the bar of tests/test_gpu_edge_cases.py for this run)
