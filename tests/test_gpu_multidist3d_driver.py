"""Multi-distance holography of a 3-D object through MultiDistModel and reconstruct_ptychography on the GPU (pytest -m gpu).

Checkers: golden F27 (the reference driver in fp64, its own fp32 run as the yardstick; tests/golden/gen_f27_multidist_3d.py) and
the NumPy restatement tests/multidist3d_ref.py.  Model level: the bars tests/ms_matrix.py:check applies with GENERIC.  Driver
level, the floors of the 3x rule as in tests/test_gpu_prj_offset_driver.py: losses 2e-4, object 1e-4 of the update.
"""
import ast
import os

import numpy as np
import pytest

from tests import ms_matrix as MM
from tests import multidist3d_ref as MR
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
    return np.load(os.path.join(ROOT, 'tests', 'golden', 'F27_multidist_3d.npz'))


def _drv_kw(tmp_path, **kw):
    base = dict(theta_st=0, theta_end=np.pi, energy_ev=ENERGY_EV, psize_cm=PSIZE_CM, gamma=0, alpha_d=0, alpha_b=0, optimizer='adam',
                save_path=str(tmp_path), output_folder='out', store_checkpoint=False, use_checkpoint=False, return_state=True)
    base.update(kw)
    return base


def _drv_inputs(F):
    par = ast.literal_eval(str(F['drv/params']))
    N = par['N']
    kw = dict(fname=F['drv/prj'], obj_size=(N, N, N), probe_pos=np.array([(0., 0.)]), n_theta=par['n_theta'],
              free_prop_cm=np.array(par['dists_cm']), minibatch_size=1, n_epochs=par['n_epochs'], learning_rate=par['learning_rate'],
              initial_guess=[F['drv/guess_delta'].astype(np.float64), F['drv/guess_beta'].astype(np.float64)], probe_type='supplied',
              probe_initial=[F['drv/probe_mag'], F['drv/probe_phase']], two_d_mode=False)
    return par, kw


# ------------------------------------------------------------------------------------------------------------ the model
def test_model_vs_restatement(A, F):
    """MultiDistModel on a 3-D object (16^3, D = 3, the rotation of angle 2): predict returns [D, Y, X] distance-major, and the loss,
    the object gradient and the probe gradient are the restatement's (3x rule on the object gradient)."""
    par, _ = _drv_inputs(F)
    N, n_theta, dists = par['N'], par['n_theta'], list(par['dists_cm'])
    ctx = A.Context(0)
    eng = A.MultisliceEngine(ctx, (N, N, N), (N, N), np.zeros((1, 2)), ENERGY_EV, PSIZE_CM, free_prop_cm=dists, max_batch=1, streamed=True,
                             detector_fanout=True)
    theta_ls = np.linspace(0, np.pi, n_theta, dtype='float32')
    tables = {}
    cv = dict(engine=eng, holo_engine=None, prj=F['drv/prj'], two_d_mode=False, theta_ls=theta_ls, forward_algorithm='fresnel',
              rotation_tables=lambda i: tables.setdefault(i, A.RotationTable(ctx, (N, N, N), theta_ls[i])))
    fm = A.MultiDistModel(device=ctx, common_vars_dict=cv)
    obj = np.stack([F['drv/guess_delta'], F['drv/guess_beta']], -1).astype(np.float32)
    probe = F['drv/probe_mag'] * np.exp(1j * F['drv/probe_phase'])
    i_theta = 2
    i_pr, i_pi = fm.get_argument_index('probe_real'), fm.get_argument_index('probe_imag')
    args = (ctx.array(obj), probe.real[None], probe.imag[None], 0., None, i_theta, np.zeros((1, 2), int), None, np.zeros((len(dists), 2)),
            np.array([0]), np.array(dists), 0, None, None, None)
    grad = ctx.zeros(obj.shape)
    out = fm.loss_and_gradients([0, i_pr, i_pi], grad, *args)
    loss = fm.current_loss
    assert out[0] is grad and out[1] is out[2]
    gp = MM.cplx(out[1].get())
    pred = fm.predict(*args)
    loss_fn = fm.get_loss_function()(*args)
    phys = O.Physics((N, N), ENERGY_EV, PSIZE_CM, free_prop_cm=dists[0])
    ref = {dt: MR.forward_adjoint_object(obj.astype(np.float64), O.rotation_coords((N, N, N), theta_ls[i_theta], dt), probe[None],
                                         np.zeros((1, 2), int), F['drv/prj'][i_theta].astype(np.float64), phys, dists, dt)
           for dt in ('float64', 'float32')}
    l64, p64, g64, gp64 = ref['float64']
    assert pred.shape == (len(dists), N, N)
    e = [rel(pred, p64), abs(loss / l64 - 1), rel(grad.get(), g64), rel(gp, gp64)]
    e32 = rel(ref['float32'][2], g64)
    print('model: pred %.2e loss %.2e grad %.2e (fp32 ref %.2e) gprobe %.2e' % (e[0], e[1], e[2], e32, e[3]))
    assert max(rel(p, po) for p, po in zip(pred, p64)) < BARS['pred']            # every distance at its place
    assert e[0] < BARS['pred'] and e[1] <= BARS['loss'] and loss_fn == loss
    assert e[2] < BARS['grad'] and e[2] <= 3 * e32 + BARS['grad_abs']
    assert e[3] < BARS['grad']
    # what the model refuses on a 3-D object, by name
    for extra, what in ((dict(optimize_free_prop=True), 'optimize_free_prop'), (dict(optimize_prj_affine=True), 'optimize_prj_affine'),
                        (dict(optimize_all_probe_pos=True), 'optimize_all_probe_pos'), (dict(rotate_out_of_loop=True), 'rotate_out_of_loop'),
                        (dict(unknown_type='real_imag'), "unknown_type='real_imag'"), (dict(safe_zone_width=2), 'data divided into sub-tiles or safe_zone_width > 0')):
        m = A.MultiDistModel(device=ctx, common_vars_dict=dict(cv, **extra))
        with pytest.raises(NotImplementedError, match='3-D object with %s' % what):
            m._check(0, None, np.zeros((len(dists), 2)))
    i_fp = fm.get_argument_index('free_prop_cm')
    with pytest.raises(NotImplementedError, match="gradient w.r.t. 'free_prop_cm'"):
        fm.loss_and_gradients([0, i_fp], grad, *args)
    m = A.MultiDistModel(device=ctx, common_vars_dict=dict(cv, engine=None))
    with pytest.raises(ValueError, match='detector_fanout=True'):
        m._check(0, None, None)
    eng.plan.close()
    ctx.close()


# ------------------------------------------------------------------------------------------------------------ the driver
def test_driver_vs_reference(A, F, tmp_path):
    """reconstruct_ptychography on the F27 driver case (16^3 object, 4 angles, D = 3, 2 epochs, Adam, minibatch 1): every loss and
    the final object under the 3x rule against the reference's fp64 run; return_state hands the object back; the output files and
    a checkpoint are written as for any other run."""
    par, kw = _drv_inputs(F)
    st = A.reconstruct_ptychography(**_drv_kw(tmp_path, **dict(kw, store_checkpoint=True)))
    l64, l32 = F['drv/fp64/losses'], F['drv/fp32/losses']
    assert len(st['losses']) == len(l64) == par['n_epochs'] * par['n_theta']
    print('losses', st['losses'], l64)
    assert np.allclose(st['losses'], l64, rtol=max(2e-4, 3 * np.abs(l32 / l64 - 1).max()))
    x64 = F['drv/fp64/obj']
    x0 = np.stack([F['drv/guess_delta'], F['drv/guess_beta']], -1).astype(np.float64)
    x = np.stack([st['delta'], st['beta']], -1).astype(np.float64)
    assert x.shape == x64.shape
    upd = np.linalg.norm(x64 - x0)
    e, e_ref = np.linalg.norm(x - x64) / upd, float(F['drv/fp32/obj_err'])
    print('object', e, e_ref)
    assert upd > 0 and e <= 3 * e_ref + 1e-4, (e, e_ref)
    assert st['engine_streamed'] is True
    out = st['output_folder']
    assert os.path.exists(os.path.join(out, 'convergence', 'loss_rank_0.txt')) and os.path.isdir(os.path.join(out, 'checkpoint'))
    assert any(f.startswith('delta') for f in os.listdir(out))


def test_driver_optimizes_the_probe(A, F, tmp_path):
    """optimize_probe on a 3-D object: the probe moves through the small-parameter table, the losses stay finite and fall."""
    par, kw = _drv_inputs(F)
    st = A.reconstruct_ptychography(**_drv_kw(tmp_path, **dict(kw, optimize_probe=True, probe_learning_rate=1e-3, learning_rate=1e-5, n_epochs=3)))
    p0 = F['drv/probe_mag'] * np.exp(1j * F['drv/probe_phase'])
    p = (st['probe_real'] + 1j * st['probe_imag'])[0]
    assert np.all(np.isfinite(st['losses'])) and np.abs(p - p0).max() > 1e-4
    n = par['n_theta']
    assert np.mean(st['losses'][-n:]) < np.mean(st['losses'][:n])


def test_checkpoint_resume_gives_the_same_object(A, F, tmp_path):
    """A run stopped after its first epoch and resumed from its last checkpoint (epoch 0, batch 3) replays that minibatch and the
    second epoch.  With one minibatch per angle the resumed optimiser step counter is the uninterrupted run's, the object's moments
    travel in the checkpoint and every kernel on the way sums in a fixed order: the losses of the replayed minibatches and the
    final object are the uninterrupted run's bit for bit."""
    par, kw = _drv_inputs(F)
    n = par['n_theta']
    whole = A.reconstruct_ptychography(**_drv_kw(tmp_path, output_folder='whole', **kw))
    common = dict(store_checkpoint=True, n_batch_per_checkpoint=1, output_folder='part')
    A.reconstruct_ptychography(**_drv_kw(tmp_path, **dict(kw, n_epochs=1, **common)))
    ck = os.path.join(str(tmp_path), 'part', 'checkpoint')
    assert [int(v) for v in np.loadtxt(os.path.join(ck, 'checkpoint.txt'))] == [0, n - 1]
    assert np.load(os.path.join(ck, 'obj_checkpoint.npy')).shape == (par['N'],) * 3 + (2,)
    res = A.reconstruct_ptychography(**_drv_kw(tmp_path, **dict(kw, use_checkpoint=True, **common)))
    assert len(res['losses']) == 1 + n
    assert np.array_equal(res['losses'], whole['losses'][n - 1:])
    assert np.array_equal(res['delta'], whole['delta']) and np.array_equal(res['beta'], whole['beta'])
    assert np.abs(whole['delta'] - F['drv/guess_delta']).max() > 0


def test_driver_refusals(A, tmp_path):
    N, D = 16, 2
    prj = np.ones((2, D, N, N), np.float32)
    guess = [np.zeros((N, N, 4)), np.zeros((N, N, 4))]
    kw = _drv_kw(tmp_path, fname=prj, obj_size=(N, N, 4), probe_pos=np.array([(0., 0.)]), probe_type='plane', initial_guess=guess, n_epochs=1,
                 minibatch_size=1, n_theta=2, free_prop_cm=[1e-4, 2e-4], two_d_mode=False)
    what = 'multi-distance holography of a 3-D object with %s'
    for extra, name in ((dict(optimize_free_prop=True), 'optimize_free_prop'), (dict(optimize_prj_affine=True), 'optimize_prj_affine'),
                        (dict(optimize_all_probe_pos=True), 'optimize_all_probe_pos'), (dict(rotate_out_of_loop=True), 'rotate_out_of_loop'),
                        (dict(unknown_type='real_imag'), "unknown_type='real_imag'"),
                        (dict(safe_zone_width=2), 'data divided into sub-tiles or safe_zone_width > 0'),
                        (dict(fname=np.ones((2, 2 * D, 8, 8), np.float32), probe_pos=np.array([(0., 0.), (0., 8.)])),
                         'data divided into sub-tiles or safe_zone_width > 0')):
        with pytest.raises(NotImplementedError, match=what % name):
            A.reconstruct_ptychography(**dict(kw, **extra))
    with pytest.raises(NotImplementedError, match="forward_algorithm='ctf' with two_d_mode=False"):
        A.reconstruct_ptychography(**dict(kw, forward_algorithm='ctf', ctf_lg_kappa=1.7))


def test_more_than_one_rank_is_refused(A, tmp_path):
    """The refusal is raised where the data are read, before any engine exists: a communicator that reports two ranks is enough."""
    from adorym_amd.comm import LocalComm

    class TwoRanks(LocalComm):
        size = 2

    N = 16
    kw = _drv_kw(tmp_path, fname=np.ones((2, 2, N, N), np.float32), obj_size=(N, N, 4), probe_pos=np.array([(0., 0.)]), probe_type='plane',
                 initial_guess=[np.zeros((N, N, 4)), np.zeros((N, N, 4))], n_epochs=1, minibatch_size=1, n_theta=2, free_prop_cm=[1e-4, 2e-4],
                 two_d_mode=False, comm=TwoRanks())
    with pytest.raises(NotImplementedError, match='multi-distance holography of a 3-D object with more than one rank'):
        A.reconstruct_ptychography(**kw)


def test_2d_multidistance_keeps_the_holography_engine(A, tmp_path, monkeypatch):
    """The 2-D multi-distance run of golden F12 still takes HolographyEngine: holo_engine is set and no fan-out plan is built."""
    from adorym_amd import ptychography as PT
    from adorym_amd.device import Plan
    f = np.load(os.path.join(ROOT, 'tests', 'golden', 'F12_multidist.npz'))
    Cc = cases.C5MINI
    inp = cases.c5mini_inputs()
    N = Cc['N']
    seen = {'fanout': 0, 'runs': []}
    orig_fan, orig_model = Plan.set_detector_fanout, PT._Run.create_forward_model

    def count_fanout(self, kernels):
        seen['fanout'] += 1
        return orig_fan(self, kernels)

    def spy(self):
        seen['runs'].append((self.holo_engine, self.engine))
        return orig_model(self)
    monkeypatch.setattr(Plan, 'set_detector_fanout', count_fanout)
    monkeypatch.setattr(PT._Run, 'create_forward_model', spy)
    st = A.reconstruct_ptychography(
        fname=f['data'][None], obj_size=(N, N, 1), probe_pos=np.array([[0., 0.]]), theta_st=0, theta_end=0, n_theta=1, two_d_mode=True,
        energy_ev=Cc['energy_ev'], psize_cm=Cc['psize_cm'], free_prop_cm=np.array(inp['dists_guess']), minibatch_size=1, n_epochs=4,
        initial_guess=[inp['guess'][0], inp['guess'][1]], probe_type='plane', raw_data_type='intensity', unknown_type='real_imag',
        gamma=0, alpha_d=0, alpha_b=0, optimizer='adam', learning_rate=1e-2, optimize_free_prop=True, free_prop_learning_rate=1e-1,
        optimize_prj_affine=True, prj_affine_learning_rate=1e-3, n_dp_batch=1, randomize_probe_pos=True, save_path=str(tmp_path),
        output_folder='c5', store_checkpoint=False, use_checkpoint=False, return_state=True)
    (holo, eng), = seen['runs']
    assert isinstance(holo, A.HolographyEngine) and not eng.detector_fanout and seen['fanout'] == 0
    assert np.allclose(st['losses'], f['e2e_losses_64'], rtol=2e-3)       # (the bar of tests/test_gpu_edge_cases.py for this run)
