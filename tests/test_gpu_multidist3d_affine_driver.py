"""Affine hologram registration of a 3-D object (holotomography with optimize_prj_affine) through MultiDistModel and
reconstruct_ptychography(..., fanout_prj_affine=True) on the GPU (pytest -m gpu).

Checkers: golden F29 (the reference driver with optimize_prj_affine in fp64, its own fp32 run as the yardstick;
tests/golden/gen_f29_multidist3d_affine.py) and the NumPy restatement tests/multidist3d_affine_ref.py.
"""
import ast
import os

import numpy as np
import pytest

from tests import ms_matrix as MM
from tests import multidist3d_affine_ref as AR
from tests.test_gpu_multidist3d_driver import _drv_kw
from oracle import adorym_oracle as O      # checker only
import cases

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENERGY_EV, PSIZE_CM = 8000., 1e-6
BARS = MM.GENERIC
rel = MM.rel
fro = lambda a: np.sqrt((np.asarray(a, np.float64) ** 2).sum(axis=(-2, -1)))


@pytest.fixture(scope='module')
def A():
    import adorym_amd
    return adorym_amd


@pytest.fixture(scope='module')
def F():
    return np.load(os.path.join(ROOT, 'tests', 'golden', 'F29_multidist3d_affine.npz'))


def _drv_inputs(F, tag='drv'):
    par = ast.literal_eval(str(F[tag + '/params']))
    N = par['N']
    kw = dict(fname=F['drv/prj'], obj_size=(N, N, N), probe_pos=np.array([(0., 0.)]), n_theta=par['n_theta'],
              free_prop_cm=np.array(par['dists_cm']), minibatch_size=1, n_epochs=par['n_epochs'], learning_rate=par['learning_rate'],
              initial_guess=[F['drv/guess_delta'].astype(np.float64), F['drv/guess_beta'].astype(np.float64)], probe_type='supplied',
              probe_initial=[F['drv/probe_mag'], F['drv/probe_phase']], two_d_mode=False, optimize_prj_affine=True,
              prj_affine_learning_rate=par['prj_affine_learning_rate'], fanout_prj_affine=True)
    if tag == 'both':
        kw.update(free_prop_cm=np.array(F['both/dists0_cm']), optimize_free_prop=True, free_prop_learning_rate=par['free_prop_learning_rate'],
                  fanout_free_prop=True)
    return par, kw


# ------------------------------------------------------------------------------------------------------------ the model
def _model(A, ctx, F, registration=True, refine=False, **extra):
    par, _ = _drv_inputs(F)
    N, n_theta, dists = par['N'], par['n_theta'], list(par['dists_cm'])
    eng = A.MultisliceEngine(ctx, (N, N, N), (N, N), np.zeros((1, 2)), ENERGY_EV, PSIZE_CM, free_prop_cm=dists, max_batch=1, streamed=True,
                             detector_fanout=True, refine_distances=refine)
    theta_ls = np.linspace(0, np.pi, n_theta, dtype='float32')
    tables = {}
    cv = dict(engine=eng, holo_engine=None, prj=F['drv/prj'], two_d_mode=False, theta_ls=theta_ls, forward_algorithm='fresnel',
              optimize_prj_affine=True, optimize_free_prop=refine,
              rotation_tables=lambda i: tables.setdefault(i, A.RotationTable(ctx, (N, N, N), theta_ls[i])), **extra)
    if registration:
        cv['hologram_registration'] = A.HologramRegistration(ctx, len(dists), (N, N), 'magnitude')
    return A.MultiDistModel(device=ctx, common_vars_dict=cv), eng, theta_ls, dists


@pytest.mark.parametrize('refine', [False, True])
def test_model_returns_the_matrix_gradient(A, F, refine):
    """MultiDistModel on a 3-D object with common_vars_dict['hologram_registration'] (16^3, D = 3, the rotation of angle 2, the
    warped holograms of golden F29, matrices half way between the identity and the truth): loss_and_gradients returns dL/dtheta
    [D, 2, 3] at that argument's place -- with and without refine_distances, together with the probe gradient -- under the 3x rule
    with the restatement's own fp32 run as the yardstick; the loss function registers too; predict never sees the data."""
    ctx = A.Context(0)
    fm, eng, theta_ls, dists = _model(A, ctx, F, refine=refine)
    N = eng.probe_size[0]
    theta = AR.round32(0.5 * (np.tile(AR.IDENTITY, (3, 1, 1)) + F['drv/theta_true']))
    obj = np.stack([F['drv/guess_delta'], F['drv/guess_beta']], -1).astype(np.float32)
    probe = F['drv/probe_mag'] * np.exp(1j * F['drv/probe_phase'])
    i_theta = 2
    i_af, i_fp = fm.get_argument_index('prj_affine_ls'), fm.get_argument_index('free_prop_cm')
    i_pr, i_pi = fm.get_argument_index('probe_real'), fm.get_argument_index('probe_imag')
    d_theta = ctx.array(np.ascontiguousarray(theta, np.float32))
    args = (ctx.array(obj), probe.real[None], probe.imag[None], 0., None, i_theta, np.zeros((1, 2), int), None, np.zeros((len(dists), 2)),
            np.array([0]), eng.dists if refine else np.array(dists), 0, d_theta, None, None)
    grad = ctx.zeros(obj.shape)
    want = [0, i_pr, i_pi, i_af] + ([i_fp] if refine else [])
    out = fm.loss_and_gradients(want, grad, *args)
    loss = fm.current_loss
    assert out[0] is grad and out[1] is out[2] and out[3].shape == (3, 2, 3) and (not refine or out[4].shape == (3,))
    g = out[3].get().astype(np.float64)
    phys = O.Physics((N, N), ENERGY_EV, PSIZE_CM, free_prop_cm=dists[0])
    ref = {dt: AR.forward_adjoint_object(obj.astype(np.float64), O.rotation_coords((N, N, N), theta_ls[i_theta], dt), probe[None],
                                         np.zeros((1, 2), int), F['drv/prj'][i_theta].astype(np.float64), phys, dists, theta, dt)
           for dt in ('float64', 'float32')}
    r64, r32 = ref['float64'], ref['float32']
    e, e32 = rel(g, r64['gtheta']), rel(r32['gtheta'], r64['gtheta'])
    print('model: loss %.2e  dL/dtheta %.2e (fp32 restatement %.2e)' % (abs(loss / r64['loss'] - 1), e, e32))
    assert e32 < 1e-2
    assert abs(loss / r64['loss'] - 1) <= BARS['loss']
    assert e < BARS['grad'] and e <= 3 * e32 + BARS['grad_abs'], (e, e32)
    for k, got in (('grad', grad.get()), ('gprobe', MM.cplx(out[1].get()))):
        e, e32 = rel(got, r64[k]), rel(r32[k], r64[k])
        assert e < BARS['grad'] and e <= 3 * e32 + BARS['grad_abs'], (k, e, e32)
    # the accumulated gradient is zeroed per evaluation: a second one returns the same bits
    again = fm.loss_and_gradients(want, ctx.zeros(obj.shape), *args)[3].get()
    assert np.array_equal(again.astype(np.float64), g)
    # the loss function registers with the same matrices; predict is the fan-out's prediction, data or no data
    assert fm.get_loss_function()(*args) == loss
    assert rel(fm.predict(*args), r64['pred']) < BARS['pred']
    ident = ctx.array(np.ascontiguousarray(np.tile(AR.IDENTITY, (3, 1, 1)), np.float32))
    assert fm.get_loss_function()(*(args[:12] + (ident,) + args[13:])) > 1.5 * loss      # (unregistered: the warped data do not fit)
    eng.plan.close()
    ctx.close()


def test_model_refusals_without_the_registration_engine(A, F):
    """Without common_vars_dict['hologram_registration'] every refusal stays; with it, what else a 3-D object refuses stays
    refused by name, and an engine built for another field or data type is refused."""
    ctx = A.Context(0)
    fm, eng, _, dists = _model(A, ctx, F, registration=False)
    assert not fm.register_3d
    with pytest.raises(NotImplementedError, match='3-D object with optimize_prj_affine is outside the accelerated path'):
        fm._check(0, None, np.zeros((3, 2)))
    fm.common_vars['optimize_prj_affine'] = False
    i_af = fm.get_argument_index('prj_affine_ls')
    obj = ctx.zeros((16, 16, 16, 2))
    args = (obj, np.ones((1, 16, 16)), np.zeros((1, 16, 16)), 0., None, 0, np.zeros((1, 2), int), None, np.zeros((3, 2)), np.array([0]),
            np.array(dists), 0, None, None, None)
    with pytest.raises(NotImplementedError, match="the gradient w.r.t. 'prj_affine_ls' is outside the accelerated path"):
        fm.loss_and_gradients([0, i_af], ctx.zeros((16, 16, 16, 2)), *args)
    eng.plan.close()
    for extra, what in ((dict(optimize_all_probe_pos=True), 'optimize_all_probe_pos together with optimize_prj_affine'),
                        (dict(rotate_out_of_loop=True), '3-D object with rotate_out_of_loop'),
                        (dict(optimize_free_prop=True), '3-D object with optimize_free_prop'),
                        (dict(unknown_type='real_imag'), "3-D object with unknown_type='real_imag'"),
                        (dict(safe_zone_width=2), '3-D object with data divided into sub-tiles or safe_zone_width > 0')):
        m, e, _, _ = _model(A, ctx, F, **{k: v for k, v in extra.items() if k != 'optimize_free_prop'})
        m.common_vars.update(extra)
        with pytest.raises(NotImplementedError, match=what):
            m._check(0, None, np.zeros((3, 2)))
        e.plan.close()
    m, e, _, _ = _model(A, ctx, F)
    m.registration = m.common_vars['hologram_registration'] = A.HologramRegistration(ctx, 3, (16, 16), 'intensity')
    with pytest.raises(ValueError, match='hologram_registration was built for another field'):
        m._check(0, None, np.zeros((3, 2)))
    e.plan.close()
    ctx.close()


# ------------------------------------------------------------------------------------------------------------ the driver
def check_history(st, F, tag, par):
    l64, l32 = F[tag + '/fp64/losses'], F[tag + '/fp32/losses']
    n_up = par['n_epochs'] * par['n_theta']
    assert len(st['losses']) == len(l64) == n_up
    e_l = np.abs(np.asarray(st['losses']) / l64 - 1).max()
    print(tag, 'losses: worst %.2e (fp32 ref %.2e)' % (e_l, np.abs(l32 / l64 - 1).max()))
    assert np.allclose(st['losses'], l64, rtol=max(2e-4, 3 * np.abs(l32 / l64 - 1).max()), atol=0)
    h64 = F[tag + '/fp64/theta']
    hist = np.asarray(st['prj_affine_history'], np.float64)
    assert hist.shape == h64.shape == (n_up, 3, 2, 3)
    dev32 = F[tag + '/fp32/theta_err'].max()
    e_h = np.abs(hist - h64).max()
    print(tag, 'matrix history: worst entry %.2e (fp32 ref %.2e)' % (e_h, dev32))
    assert e_h <= 3 * dev32 + 2. ** -23, (e_h, dev32)
    assert np.array_equal(hist[:, 0], np.tile(AR.IDENTITY, (n_up, 1, 1)))             # matrix 0 is pinned, exactly
    assert np.array_equal(np.asarray(st['prj_affine_ls'], np.float32), hist[-1].astype(np.float32))
    return hist


def test_driver_vs_reference(A, F, tmp_path):
    """reconstruct_ptychography(optimize_prj_affine=True, fanout_prj_affine=True) on the F29 driver case (16^3 object started at the
    truth, 4 angles, D = 3, holograms 1 and 2 warped by known matrices, the run started at the identity, 20 epochs, Adam on the
    matrices with step 1e-2).

    Losses: rtol = max(2e-4, 3 * the reference's own fp32 deviation).  The matrices after every update against the reference's
    fp64 run, per entry: 3 * the largest deviation of the reference's own fp32 run over the history, plus one float32 ulp of 1
    (2^-23).  Matrix 0 is exactly the identity after every update.  Every free matrix's final Frobenius distance from the truth
    (the inverse of the warp) is below 1/3 of its starting one (the reference reaches 0.13 and 0.08)."""
    par, kw = _drv_inputs(F)
    st = A.reconstruct_ptychography(**_drv_kw(tmp_path, **kw))
    hist = check_history(st, F, 'drv', par)
    true = F['drv/theta_true']
    ratio = fro(hist[-1] - true)[1:] / fro(AR.IDENTITY - true)[1:]
    print('final Frobenius errors / starting errors', ratio)
    assert np.all(ratio < 1. / 3), ratio
    assert st['engine_streamed'] is True and st['free_prop_cm_history'] is None


def test_driver_refines_distances_and_matrices_together(A, F, tmp_path):
    """fanout_free_prop + fanout_prj_affine (the reference demo's feature set) against its record, 8 epochs from F28's starting
    distances: losses and matrix history by the rules above, the distance history by test_gpu_multidist3d_dist_driver.py's rule."""
    par, kw = _drv_inputs(F, 'both')
    st = A.reconstruct_ptychography(**_drv_kw(tmp_path, **kw))
    check_history(st, F, 'both', par)
    h64 = F['both/fp64/dists']
    hist = np.asarray(st['free_prop_cm_history'], np.float64)
    assert hist.shape == h64.shape
    dev32 = (F['both/fp32/dists_err'] / h64).max()
    e_h = np.abs(hist / h64 - 1).max()
    print('distance history: worst %.2e (fp32 ref %.2e)' % (e_h, dev32))
    assert e_h <= 3 * dev32 + 2. ** -23, (e_h, dev32)


def test_checkpoint_resume_gives_the_same_matrices(A, F, tmp_path):
    """A run stopped after its first epoch and resumed from its last checkpoint (epoch 0, batch 3) replays that minibatch and the
    second epoch: the matrices travel in the checkpoint under the reference's key prj_affine_ls (their optimiser's moments beside
    them), and the losses of the replayed minibatches and the matrices are the uninterrupted run's bit for bit."""
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
    assert np.array_equal(np.asarray(saved['prj_affine_ls'], np.float32), whole['prj_affine_history'][n - 2].astype(np.float32))
    res = A.reconstruct_ptychography(**_drv_kw(tmp_path, **dict(kw, use_checkpoint=True, **common)))
    assert len(res['losses']) == 1 + n
    assert np.array_equal(res['losses'], whole['losses'][n - 1:])
    assert np.array_equal(res['prj_affine_ls'], whole['prj_affine_ls'])
    assert np.array_equal(res['prj_affine_history'], whole['prj_affine_history'][n - 1:])
    assert np.abs(np.asarray(whole['prj_affine_ls'], np.float64)[1:] - AR.IDENTITY).max() > 1e-3


def test_driver_refusals(A, tmp_path):
    N, D = 16, 2
    prj = np.ones((2, D, N, N), np.float32)
    guess = [np.zeros((N, N, 4)), np.zeros((N, N, 4))]
    kw = _drv_kw(tmp_path, fname=prj, obj_size=(N, N, 4), probe_pos=np.array([(0., 0.)]), probe_type='plane', initial_guess=guess, n_epochs=1,
                 minibatch_size=1, n_theta=2, free_prop_cm=[1e-4, 2e-4], two_d_mode=False, optimize_prj_affine=True)
    what = 'multi-distance holography of a 3-D object with %s'
    # without the keyword: the refusal as it was, with and without the other opt-in
    for extra in ({}, dict(fanout_free_prop=True)):
        with pytest.raises(NotImplementedError, match=what % 'optimize_prj_affine'):
            A.reconstruct_ptychography(**dict(kw, **extra))
    # with it, what else a 3-D object refuses stays refused by name
    for extra, name in ((dict(optimize_all_probe_pos=True), 'optimize_all_probe_pos'), (dict(rotate_out_of_loop=True), 'rotate_out_of_loop'),
                        (dict(unknown_type='real_imag'), "unknown_type='real_imag'"),
                        (dict(safe_zone_width=2), 'data divided into sub-tiles or safe_zone_width > 0'),
                        (dict(optimize_free_prop=True), 'optimize_free_prop')):
        with pytest.raises(NotImplementedError, match=what % name):
            A.reconstruct_ptychography(**dict(kw, fanout_prj_affine=True, **extra))
    with pytest.raises(NotImplementedError, match="forward_algorithm='ctf' with two_d_mode=False"):
        A.reconstruct_ptychography(**dict(kw, fanout_prj_affine=True, forward_algorithm='ctf', ctf_lg_kappa=1.7))
    # the keyword alone (no optimize_prj_affine) changes nothing: no registration engine, no history
    st = A.reconstruct_ptychography(**dict(kw, optimize_prj_affine=False, fanout_prj_affine=True))
    assert st['prj_affine_history'] is None and np.all(np.isfinite(st['losses']))


def test_2d_multidistance_keeps_the_holography_engine(A, tmp_path, monkeypatch):
    """The 2-D multi-distance run of golden F12 (config 5, optimize_prj_affine) still takes HolographyEngine, with the keyword too:
    holo_engine is set and no registration engine is built."""
    from adorym_amd import ptychography as PT
    from adorym_amd import holography as H
    f = np.load(os.path.join(ROOT, 'tests', 'golden', 'F12_multidist.npz'))
    Cc = cases.C5MINI
    inp = cases.c5mini_inputs()
    N = Cc['N']
    seen = {'built': 0, 'runs': []}
    orig_init, orig_model = H.HologramRegistration.__init__, PT._Run.create_forward_model

    def count_init(self, *a, **k):
        seen['built'] += 1
        return orig_init(self, *a, **k)

    def spy(self):
        seen['runs'].append((self.holo_engine, self.engine, self.registration))
        return orig_model(self)
    monkeypatch.setattr(H.HologramRegistration, '__init__', count_init)
    monkeypatch.setattr(PT._Run, 'create_forward_model', spy)
    st = A.reconstruct_ptychography(
        fname=f['data'][None], obj_size=(N, N, 1), probe_pos=np.array([[0., 0.]]), theta_st=0, theta_end=0, n_theta=1, two_d_mode=True,
        energy_ev=Cc['energy_ev'], psize_cm=Cc['psize_cm'], free_prop_cm=np.array(inp['dists_guess']), minibatch_size=1, n_epochs=4,
        initial_guess=[inp['guess'][0], inp['guess'][1]], probe_type='plane', raw_data_type='intensity', unknown_type='real_imag',
        gamma=0, alpha_d=0, alpha_b=0, optimizer='adam', learning_rate=1e-2, optimize_free_prop=True, free_prop_learning_rate=1e-1,
        optimize_prj_affine=True, prj_affine_learning_rate=1e-3, n_dp_batch=1, randomize_probe_pos=True, save_path=str(tmp_path),
        output_folder='c5', store_checkpoint=False, use_checkpoint=False, return_state=True, fanout_prj_affine=True)
    (holo, eng, reg), = seen['runs']
    assert isinstance(holo, A.HolographyEngine) and not eng.detector_fanout and reg is None and seen['built'] == 0
    assert st['prj_affine_history'] is None
    assert np.allclose(st['losses'], f['e2e_losses_64'], rtol=2e-3)       # (the bar of tests/test_gpu_edge_cases.py for this run)
