"""reconstruct_ptychography(forward_algorithm='ctf') and MultiDistModel's CTF route on the GPU (pytest -m gpu).

Checker: golden F26 (b) -- the reference driver in fp64, its own fp32 run as the yardstick (tests/golden/gen_f26_ctf.py) -- and
tests/ctf_ref.py's loop (held to that golden by tests/test_ctf_ref_vs_golden.py) for what the reference driver cannot run.
16 x 16 x 1 object, three distances, one minibatch per epoch, four epochs, Adam on the object and on ctf_lg_kappa.
"""
import ast
import os
import pickle

import numpy as np
import pytest

from tests import ctf_matrix as CM
from tests import ctf_ref as R

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ULP = 2. ** -23          # one fp32 spacing in [1, 2): ctf_lg_kappa lives in fp32 here and in float64 in the reference


@pytest.fixture(scope='module')
def A():
    import adorym_amd
    return adorym_amd


@pytest.fixture(scope='module')
def F():
    return np.load(os.path.join(ROOT, 'tests', 'golden', 'F26_ctf.npz'))


def drv_kw(F, tmp_path, **over):
    par = ast.literal_eval(str(F['drv/params']))
    ny, nx, nd = par['field']
    obj = F['drv/obj'].astype(np.float64)
    kw = dict(fname=F['drv/data'][None], obj_size=(ny, nx, 1), probe_pos=np.array([[0., 0.]]), theta_st=0, theta_end=0, n_theta=1, two_d_mode=True,
              energy_ev=CM.ENERGY_EV, psize_cm=CM.PSIZE_CM, free_prop_cm=np.array(F['drv/dists']), minibatch_size=1, n_epochs=par['n_epochs'],
              initial_guess=[obj[:, :, None, 0], obj[:, :, None, 1]], probe_type='plane', raw_data_type='intensity', unknown_type='delta_beta',
              gamma=0, alpha_d=0, alpha_b=0, optimizer='adam', learning_rate=par['learning_rate'], forward_algorithm='ctf', ctf_lg_kappa=CM.LG_KAPPA,
              optimize_ctf_lg_kappa=True, ctf_lg_kappa_learning_rate=par['ctf_lg_kappa_learning_rate'], n_dp_batch=1, randomize_probe_pos=True,
              safe_zone_width=0, save_path=str(tmp_path), output_folder='out', store_checkpoint=False, use_checkpoint=False, return_state=True)
    kw.update(over)
    return par, kw


def ref_loop(F, dtype=np.float64, **over):
    par = ast.literal_eval(str(F['drv/params']))
    obj = F['drv/obj']
    kw = dict(n_epochs=par['n_epochs'], learning_rate=par['learning_rate'], optimize_ctf_lg_kappa=True,
              ctf_lg_kappa_learning_rate=par['ctf_lg_kappa_learning_rate'], dtype=dtype)
    kw.update(over)
    return R.reconstruct(F['drv/data'], obj[..., 0], obj[..., 1], F['drv/dists'], CM.LG_KAPPA, CM.ENERGY_EV, CM.PSIZE_CM, **kw)


def check_run(st, l64, x64, x32, lr, what):
    """Losses within 1e-5 of the fp64 run; final object: RMSE < 1e-5 and |x - x64| <= 3 |x32 - x64| outside the voxels Adam pushed the
    other way (a voxel whose gradient is at rounding level moves by a step of either sign in any fp32 run: tests/test_gpu_variants.py)."""
    e = np.abs(np.asarray(st['losses']) / l64 - 1).max()
    print('%s: losses %r (fp64 %r): %.2e' % (what, st['losses'], list(l64), e))
    assert len(st['losses']) == len(l64) and e < 1e-5, (what, e)
    x = np.stack([st['delta'], st['beta']], -1).astype(np.float64).reshape(x64.shape)
    d = np.abs(x - x64)
    rmse = np.sqrt(np.mean(d ** 2))
    flipped = d > 0.5 * lr
    e_us, e_ref = np.linalg.norm((x - x64)[~flipped]), np.linalg.norm((x32 - x64)[~flipped])
    print('%s: object RMSE %.2e, |x - x64| %.2e (fp32 reference %.2e), voxels set aside %d' % (what, rmse, e_us, e_ref, flipped.sum()))
    assert rmse < 1e-5 and flipped.mean() < 1e-3 and e_us <= 3 * e_ref, (what, rmse, e_us, e_ref)


def test_driver_vs_reference(A, F, tmp_path):
    """The run of golden F26 (b): losses, final object, ctf_lg_kappa after every update (return_state carries value and history)."""
    par, kw = drv_kw(F, tmp_path)
    st = A.reconstruct_ptychography(**kw)
    x64 = np.stack([F['drv/fp64/delta'], F['drv/fp64/beta']], -1).astype(np.float64)
    x32 = np.stack([F['drv/fp32/delta'], F['drv/fp32/beta']], -1).astype(np.float64)
    check_run(st, F['drv/fp64/losses'], x64, x32, par['learning_rate'], 'driver')
    assert np.array_equal(st['beta'].reshape(16, 16), F['drv/obj'][..., 1])          # dL/dbeta = 0: Adam leaves beta where it was
    t64, t32 = F['drv/fp64/lg_kappa_trace'], F['drv/fp32/lg_kappa_trace']
    hist = np.asarray(st['ctf_lg_kappa_history'], np.float64)
    assert hist.shape == t64.shape and st['ctf_lg_kappa'].shape == (1,) and st['ctf_lg_kappa'][0] == np.float32(hist[-1])
    bound = 3 * np.abs(t32 - t64) + np.arange(1, len(t64) + 1) * ULP
    print('ctf_lg_kappa', hist, 'fp64', t64, 'off by', np.abs(hist - t64), 'bound', bound)
    assert (np.abs(hist - t64) <= bound).all()
    assert abs(t64[-1] - CM.LG_KAPPA) > 100 * bound[-1]                              # (a bound the parameter's own movement exceeds)
    assert st['free_prop_cm'] is not None and np.allclose(st['free_prop_cm'], F['drv/dists'])
    assert not os.path.exists(os.path.join(str(tmp_path), 'out', 'intermediate'))


def test_fixed_kappa_vs_the_restatement(A, F, tmp_path):
    """optimize_ctf_lg_kappa=False (the reference driver raises TypeError there, golden 'drv/flag_off'): the fixed ctf_lg_kappa,
    against ctf_ref's loop in fp64 with its fp32 loop as the yardstick."""
    par, kw = drv_kw(F, tmp_path, optimize_ctf_lg_kappa=False)
    st = A.reconstruct_ptychography(**kw)
    r64, r32 = ref_loop(F, optimize_ctf_lg_kappa=False), ref_loop(F, np.float32, optimize_ctf_lg_kappa=False)
    check_run(st, np.array(r64['losses']), r64['obj'], r32['obj'].astype(np.float64), par['learning_rate'], 'fixed kappa')
    assert st['ctf_lg_kappa'][0] == np.float32(CM.LG_KAPPA) and st['ctf_lg_kappa_history'] is None


def test_callers_optimizer_and_update_delay(A, F, tmp_path):
    """optimizer_ctf_lg_kappa supplied by the caller (its step size counts, not ctf_lg_kappa_learning_rate), and
    other_params_update_delay = 2 holding kappa still for the first two updates."""
    par, kw = drv_kw(F, tmp_path, output_folder='own', ctf_lg_kappa_learning_rate=1e-9,
                     optimizer_ctf_lg_kappa=None)
    kw['optimizer_ctf_lg_kappa'] = A.AdamOptimizer('mine', output_folder=str(tmp_path), options_dict={'step_size': 4e-3})
    st = A.reconstruct_ptychography(**kw)
    r = ref_loop(F, ctf_lg_kappa_learning_rate=4e-3)
    hist = np.asarray(st['ctf_lg_kappa_history'], np.float64)
    print('own optimiser', hist, r['lg_kappa_trace'])
    assert np.abs(hist - r['lg_kappa_trace']).max() <= 1e-7 + len(hist) * ULP and abs(hist[-1] - CM.LG_KAPPA) > 5e-3
    par, kw = drv_kw(F, tmp_path, output_folder='delay', other_params_update_delay=2)
    st = A.reconstruct_ptychography(**kw)
    r = ref_loop(F, other_params_update_delay=2)
    hist = np.asarray(st['ctf_lg_kappa_history'], np.float64)
    print('delay', hist, r['lg_kappa_trace'], st['losses'], r['losses'])
    assert r['lg_kappa_trace'][:2] == [float(np.float64(CM.LG_KAPPA))] * 2
    assert hist.shape == (2,) and np.abs(hist - r['lg_kappa_trace'][2:]).max() <= 1e-7 + 2 * ULP
    assert np.abs(np.asarray(st['losses']) / r['losses'] - 1).max() < 1e-5


def test_checkpoint_carries_kappa_and_resume_ends_where_the_whole_run_ends(A, F, tmp_path):
    """params_0 holds ctf_lg_kappa under the reference's key; a run stopped after two epochs and resumed from its last checkpoint
    (epoch 1) replays that minibatch from the stored object, moments and kappa: its loss is the uninterrupted run's, bit for bit.
    Not bit-identical afterwards by design of the reference (tests/test_gpu_projection_driver.py): on resume the Adam step counter
    of every later epoch is starting_epoch * n_batch + starting_batch = 1 where the uninterrupted run counts 0, so each of the three
    remaining object steps is up to a quarter shorter (bias corrections 1 / 0.19 and 1 / 0.002 against 1 / 0.1 and 1 / 0.001), and
    the moments of the small parameters are not part of the reference's checkpoint, so kappa's Adam restarts them: object and
    kappa end within two of their steps of the uninterrupted run (ctf_ref's arithmetic with those counters on the host: 1.2 and
    1.4 steps), with the loss still falling."""
    par, kw = drv_kw(F, tmp_path, output_folder='whole')
    whole = A.reconstruct_ptychography(**kw)
    common = dict(store_checkpoint=True, n_batch_per_checkpoint=1, output_folder='part')
    part = A.reconstruct_ptychography(**drv_kw(F, tmp_path, n_epochs=2, **common)[1])
    ck = os.path.join(str(tmp_path), 'part', 'checkpoint')
    with open(os.path.join(ck, 'params_0'), 'rb') as f:
        saved = np.asarray(pickle.load(f)['ctf_lg_kappa'], np.float64).reshape(-1)
    assert [int(v) for v in np.loadtxt(os.path.join(ck, 'checkpoint.txt'))] == [1, 0]
    o_ck = np.load(os.path.join(ck, 'obj_checkpoint.npy')).astype(np.float64).reshape(16, 16, 2)      # (the resumed run writes its own)
    hist_part = np.asarray(part['ctf_lg_kappa_history'], np.float64)
    print('checkpoint kappa', saved, 'history of the stopped run', hist_part)
    assert saved.shape == (1,) and np.float32(saved[0]) == np.float32(hist_part[0]) != np.float32(CM.LG_KAPPA)
    res = A.reconstruct_ptychography(**drv_kw(F, tmp_path, use_checkpoint=True, **common)[1])
    lr = par['ctf_lg_kappa_learning_rate']
    hist = np.asarray(res['ctf_lg_kappa_history'], np.float64)
    print('resumed', hist, res['losses'], 'whole', whole['ctf_lg_kappa_history'], whole['losses'])
    assert len(res['losses']) == 3 and res['losses'][0] == whole['losses'][1]               # the replayed minibatch: same state, same bits
    # kappa started from the checkpoint's value: its first resumed value is one Adam step with fresh moments and step counter 1 from
    # it, on the gradient at the checkpointed object (ctf_ref on the host)
    from oracle.adorym_oracle import adam_step
    g_ck = R.forward_adjoint(o_ck[..., 0], F['drv/dists'], saved[0], F['drv/data'], CM.ENERGY_EV, CM.PSIZE_CM, 'intensity')['grad_lg_kappa']
    want = adam_step(saved.copy(), np.array([g_ck]), np.zeros(1), np.zeros(1), 1, step_size=lr)[0][0]
    print('first resumed kappa', hist[0], 'a fresh Adam step from the saved value', want)
    assert abs(hist[0] - want) <= 1e-7 + ULP and abs(want - saved[0]) > 100 * (1e-7 + ULP)
    assert np.all(np.diff(res['losses']) < 0) and res['losses'][-1] < whole['losses'][2]
    assert abs(res['ctf_lg_kappa'][0] - whole['ctf_lg_kappa'][0]) <= 2 * lr
    assert np.abs(res['delta'] - whole['delta']).max() <= 2 * par['learning_rate']
    assert np.abs(whole['delta'].reshape(16, 16) - F['drv/obj'][..., 0]).max() > 4 * par['learning_rate']  # (a bound the run's own movement exceeds)


def test_intermediate_folder_is_created_and_left_empty(A, F, tmp_path):
    par, kw = drv_kw(F, tmp_path, n_epochs=1, save_intermediate=True)
    A.reconstruct_ptychography(**kw)
    d = os.path.join(str(tmp_path), 'out', 'intermediate', 'ctf_lg_kappa')
    assert os.path.isdir(d) and os.listdir(d) == []


def test_plugin_route(A, F, tmp_path):
    """forward_model=adorym_amd.MultiDistModel gives the 'auto' run, bit for bit."""
    par, kw = drv_kw(F, tmp_path, output_folder='auto', n_epochs=2)
    a = A.reconstruct_ptychography(**kw)
    b = A.reconstruct_ptychography(**dict(kw, output_folder='plugin', forward_model=A.MultiDistModel))
    assert a['losses'] == b['losses'] and np.array_equal(a['delta'], b['delta']) and np.array_equal(a['ctf_lg_kappa_history'], b['ctf_lg_kappa_history'])


def test_model_level_predict_loss_and_gradients(A, F):
    """MultiDistModel.predict / the loss function / loss_and_gradients route to the CTF engine; the kappa gradient sits at that
    argument's place in the tuple; an object regulariser is added as on the undivided Fresnel path."""
    ctx = A.Context(0)
    c = CM.case(16, 16, 3)
    eng = A.CTFEngine(ctx, (16, 16), 3, CM.ENERGY_EV, CM.PSIZE_CM, raw_data_type='intensity')
    ms = A.MultisliceEngine(ctx, (16, 16, 1), (8, 8), np.zeros((1, 2), int), CM.ENERGY_EV, CM.PSIZE_CM, free_prop_cm=0, max_batch=1)
    cv = dict(engine=ms, ctf_engine=eng, forward_algorithm='ctf', two_d_mode=True, unknown_type='delta_beta', optimize_ctf_lg_kappa=True,
              prj=c['data'][None], n_probe_modes=1, safe_zone_width=0)
    fm = A.MultiDistModel(device=ctx, common_vars_dict=cv, raw_data_type='intensity')
    obj = ctx.array(c['obj'][:, :, None, :])
    args = dict(probe_real=None, probe_imag=None, probe_defocus_mm=0., probe_pos_offset=None, this_i_theta=0, this_pos_batch=np.zeros((1, 2)),
                prj=c['data'][None], probe_pos_correction=None, this_ind_batch=np.array([0]), free_prop_cm=c['dists'], safe_zone_width=0,
                prj_affine_ls=None, ctf_lg_kappa=np.array([CM.LG_KAPPA]), prj_pos_offset=None)
    o = c['o64']
    assert CM.rel(fm.predict(obj, **args), o['pred']) < CM.BARS['pred']
    assert abs(fm.get_loss_function()(obj, **args) / o['loss'] - 1) < CM.BARS['loss']
    g = ctx.zeros((16, 16, 1, 2))
    i_k = fm.get_argument_index('ctf_lg_kappa')
    out = fm.loss_and_gradients([0, i_k], g, obj, **args)
    assert out[0] is g and CM.rel(g.get()[:, :, 0, 0], o['grad_delta']) < CM.BARS['grad'] and not g.get()[..., 1].any()
    assert abs(out[1].get()[0] / o['grad_lg_kappa'] - 1) < CM.BARS['gkappa']
    assert abs(fm.current_loss / o['loss'] - 1) < CM.BARS['loss']
    # a regulariser on the object: value and gradient are added
    fm.add_regularizers([A.L1Regularizer(1e-3, 1e-3, unknown_type='delta_beta')])
    g2 = ctx.zeros((16, 16, 1, 2))
    fm.loss_and_gradients([0], g2, obj, **args)
    l1 = 1e-3 * np.abs(c['obj'].astype(np.float64)).mean(axis=(0, 1)).sum()
    assert abs(fm.current_loss - (o['loss'] + l1)) < 1e-4 * l1
    assert np.abs(g2.get() - g.get()).max() > 0 and g2.get()[..., 1].any()
    ms.plan.close()
    ctx.close()


def test_refusals(A, F, tmp_path):
    """Everything the CTF model does not serve is refused by name, by the driver and by the model."""
    par, kw = drv_kw(F, tmp_path)
    run = lambda **over: A.reconstruct_ptychography(**dict(kw, **over))
    ny = 16
    ri = [np.ones((ny, ny, 1)), np.zeros((ny, ny, 1))]
    for over, what in ((dict(unknown_type='real_imag', initial_guess=ri), "forward_algorithm='ctf' with unknown_type='real_imag'"),
                       (dict(n_probe_modes=2), "forward_algorithm='ctf' with n_probe_modes != 1"),
                       (dict(optimize_probe=True), "forward_algorithm='ctf' with optimize_probe"),
                       (dict(optimize_free_prop=True), "forward_algorithm='ctf' with optimize_free_prop"),
                       (dict(optimize_prj_affine=True), "forward_algorithm='ctf' with optimize_prj_affine"),
                       (dict(optimize_all_probe_pos=True), "forward_algorithm='ctf' with optimize_all_probe_pos"),
                       (dict(safe_zone_width=2), "forward_algorithm='ctf' with data divided into sub-tiles or safe_zone_width > 0"),
                       (dict(two_d_mode=False, obj_size=(ny, ny, 2), initial_guess=[np.zeros((ny, ny, 2))] * 2), "forward_algorithm='ctf' with two_d_mode=False"),
                       (dict(loss_function_type='poisson'), "forward_algorithm='ctf' with loss_function_type='poisson'"),
                       (dict(forward_algorithm='fresnel'), "optimize_ctf_lg_kappa with forward_algorithm='fresnel'"),
                       (dict(pure_projection=True), "forward_algorithm='ctf'"),
                       (dict(free_prop_cm=1e-3, fname=F['drv/data'][None, :1]), "forward_algorithm='ctf'"),
                       (dict(forward_algorithm='born'), "forward_algorithm='born'"),
                       (dict(update_using_external_algorithm='ctf'), 'update_using_external_algorithm')):
        with pytest.raises(NotImplementedError, match=what.replace('(', r'\(').replace(')', r'\)')):
            run(**over)
    ctx = A.Context(0)
    eng = A.CTFEngine(ctx, (16, 16), 3, CM.ENERGY_EV, CM.PSIZE_CM)
    base = dict(engine=None, ctf_engine=eng, forward_algorithm='ctf', two_d_mode=True, unknown_type='delta_beta', n_probe_modes=1)
    for cv, what in ((dict(unknown_type='real_imag'), 'real_imag'), (dict(n_probe_modes=3), 'n_probe_modes != 1'), (dict(two_d_mode=False), 'two_d_mode=False'),
                     (dict(optimize_probe=True), 'optimize_probe'), (dict(optimize_free_prop=True), 'optimize_free_prop'),
                     (dict(optimize_prj_affine=True), 'optimize_prj_affine'), (dict(optimize_all_probe_pos=True), 'optimize_all_probe_pos'),
                     (dict(safe_zone_width=3), 'safe_zone_width > 0')):
        fm = A.MultiDistModel(device=ctx, common_vars_dict=dict(base, **cv), raw_data_type='intensity')
        with pytest.raises(NotImplementedError, match="forward_algorithm='ctf' with .*" + what):
            fm._check(cv.get('safe_zone_width', 0), np.array([1.7]), None)
    fm = A.MultiDistModel(device=ctx, common_vars_dict=dict(engine=None, holo_engine=None, two_d_mode=True, optimize_ctf_lg_kappa=True))
    with pytest.raises(NotImplementedError, match="optimize_ctf_lg_kappa with forward_algorithm='fresnel'"):
        fm._check(0, np.array([1.7]), None)
    with pytest.raises(ValueError, match='ctf_engine'):
        A.MultiDistModel(device=ctx, common_vars_dict=dict(engine=None, forward_algorithm='ctf'))
    with pytest.raises(NotImplementedError, match='LSQ'):
        A.MultiDistModel(loss_function_type='poisson', device=ctx, common_vars_dict=dict(base))
    ctx.close()
