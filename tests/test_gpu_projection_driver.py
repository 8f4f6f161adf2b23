"""reconstruct_ptychography(pure_projection=True) and PtychographyModel on the GPU (pytest -m gpu).

Checker: golden F25 (b) (the reference driver in fp64, its own fp32 run as the yardstick; tests/golden/gen_f25_pure_projection.py).
Floors of the 3x rule as tests/test_gpu_prj_offset_driver.py has them: losses 2e-4, object 1e-4 of the update.
"""
import ast
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope='module')
def A():
    import adorym_amd
    return adorym_amd


@pytest.fixture(scope='module')
def F():
    return np.load(os.path.join(ROOT, 'tests', 'golden', 'F25_pure_projection.npz'))


def _drv_kw(tmp_path, **kw):
    base = dict(theta_st=0, theta_end=np.pi, gamma=0, alpha_d=0, alpha_b=0, optimizer='adam', save_path=str(tmp_path), output_folder='out',
                store_checkpoint=False, use_checkpoint=False, return_state=True)
    base.update(kw)
    return base


def _drv_inputs(F):
    par = ast.literal_eval(str(F['drv/params']))
    N = par['N']
    kw = dict(fname=F['drv/prj'], obj_size=(N, N, N), probe_pos=F['drv/pos'], n_theta=par['n_theta'], free_prop_cm=par['free_prop_cm'],
              energy_ev=par['energy_ev'], psize_cm=par['psize_cm'], minibatch_size=par['minibatch_size'], n_epochs=par['n_epochs'],
              learning_rate=par['learning_rate'], initial_guess=[F['drv/guess_delta'].astype(np.float64), F['drv/guess_beta'].astype(np.float64)],
              probe_type='supplied', probe_initial=[F['drv/probe_mag'], F['drv/probe_phase']], pure_projection=True)
    return par, kw


def _check_driver(st, F, losses64=None, losses32=None):
    l64 = F['drv/fp64/losses'] if losses64 is None else losses64
    l32 = F['drv/fp32/losses'] if losses32 is None else losses32
    assert len(st['losses']) == len(l64)
    print('losses', st['losses'], l64)
    assert np.allclose(st['losses'], l64, rtol=max(2e-4, 3 * np.abs(l32 / l64 - 1).max()))
    x64 = np.stack([F['drv/fp64/delta'], F['drv/fp64/beta']], -1).astype(np.float64)
    x32 = np.stack([F['drv/fp32/delta'], F['drv/fp32/beta']], -1).astype(np.float64)
    x0 = np.stack([F['drv/guess_delta'], F['drv/guess_beta']], -1).astype(np.float64)
    x = np.stack([st['delta'], st['beta']], -1).astype(np.float64)
    upd = np.linalg.norm(x64 - x0)
    e, e_ref = np.linalg.norm(x - x64) / upd, np.linalg.norm(x32 - x64) / upd
    print('object', e, e_ref)
    assert upd > 0 and e <= 3 * e_ref + 1e-4, (e, e_ref)


def test_driver_immediate_vs_reference(A, F, tmp_path):
    par, kw = _drv_inputs(F)
    st = A.reconstruct_ptychography(**_drv_kw(tmp_path, **kw))
    _check_driver(st, F)


def test_driver_accepts_and_ignores_binning(A, F, tmp_path):
    """``binning`` has no effect on the projection model in the reference: the run with binning = 3 is the run without, bit for bit."""
    par, kw = _drv_inputs(F)
    a = A.reconstruct_ptychography(**_drv_kw(tmp_path, output_folder='a', **dict(kw, n_epochs=1)))
    b = A.reconstruct_ptychography(**_drv_kw(tmp_path, output_folder='b', **dict(kw, n_epochs=1, binning=3)))
    assert np.array_equal(a['delta'], b['delta']) and np.array_equal(a['beta'], b['beta']) and a['losses'] == b['losses']


def test_driver_per_angle_gives_the_unfused_sums(A, F, tmp_path):
    """'per angle': the three minibatches of an angle in one fused launch against the same run minibatch by minibatch
    (fuse_per_angle=False): the same sums in another order."""
    par, kw = _drv_inputs(F)
    kw = dict(kw, update_scheme='per angle', n_epochs=1)
    a = A.reconstruct_ptychography(**_drv_kw(tmp_path, output_folder='fused', **kw))
    b = A.reconstruct_ptychography(**_drv_kw(tmp_path, output_folder='unfused', fuse_per_angle=False, **kw))
    assert len(a['losses']) == len(b['losses']) == par['n_theta']
    assert np.allclose(a['losses'], b['losses'], rtol=2e-4)
    x0 = np.stack([F['drv/guess_delta'], F['drv/guess_beta']], -1).astype(np.float64)
    xa, xb = [np.stack([s['delta'], s['beta']], -1).astype(np.float64) for s in (a, b)]
    upd = np.linalg.norm(xb - x0)
    assert upd > 0 and np.linalg.norm(xa - xb) / upd < 5e-3


def test_checkpoint_resume_ends_where_the_whole_run_ends(A, F, tmp_path):
    """A run stopped after its first epoch and resumed from its last checkpoint (epoch 0, batch 11) replays that minibatch and the
    second epoch.  Not bit-identical by design of the reference (tests/test_gpu_e2e.py:test_checkpoint_files_and_resume): on resume
    the Adam step counter restarts at a minibatch index, 11, where the uninterrupted run counts angles, 3; the bias corrections
    then differ by a quarter over the 13 updates that follow: at most 13 * 0.25 steps of 1e-6, bounded here by 1e-5."""
    par, kw = _drv_inputs(F)
    whole = A.reconstruct_ptychography(**_drv_kw(tmp_path, output_folder='whole', **kw))
    common = dict(store_checkpoint=True, n_batch_per_checkpoint=1, output_folder='part')
    A.reconstruct_ptychography(**_drv_kw(tmp_path, **dict(kw, n_epochs=1, **common)))
    ck = os.path.join(str(tmp_path), 'part', 'checkpoint')
    assert [int(v) for v in np.loadtxt(os.path.join(ck, 'checkpoint.txt'))] == [0, 11]
    assert np.load(os.path.join(ck, 'obj_checkpoint.npy')).shape == (par['N'],) * 3 + (2,)
    res = A.reconstruct_ptychography(**_drv_kw(tmp_path, **dict(kw, use_checkpoint=True, **common)))
    assert len(res['losses']) == 1 + 12
    assert np.allclose(res['losses'][-12:], whole['losses'][-12:], rtol=3e-2)
    assert max(np.abs(res['delta'] - whole['delta']).max(), np.abs(res['beta'] - whole['beta']).max()) < 1e-5
    assert np.abs(whole['delta'] - F['drv/guess_delta']).max() > 1e-5          # (a bound that the run's own movement exceeds)


def test_probe_refinement_and_single_slice_run(A, F, tmp_path):
    """optimize_probe with the projection model moves the probe and lowers the loss; an object with ONE slice takes the ordinary
    engine and gives the run without the flag, bit for bit."""
    par, kw = _drv_inputs(F)
    st = A.reconstruct_ptychography(**_drv_kw(tmp_path, output_folder='probe', optimize_probe=True, probe_learning_rate=1e-3, **kw))
    p0 = F['drv/probe_mag'] * np.exp(1j * F['drv/probe_phase'])
    assert np.abs(st['probe_real'][0] + 1j * st['probe_imag'][0] - p0).max() > 1e-4 and np.all(np.isfinite(st['losses']))
    N = par['N']
    one = dict(kw, obj_size=(N, N, 1), n_theta=1, fname=F['drv/prj'][:1], n_epochs=1,
               initial_guess=[F['drv/guess_delta'][:, :, :1].astype(np.float64), F['drv/guess_beta'][:, :, :1].astype(np.float64)])
    a = A.reconstruct_ptychography(**_drv_kw(tmp_path, output_folder='one_pp', **one))
    b = A.reconstruct_ptychography(**_drv_kw(tmp_path, output_folder='one', **dict(one, pure_projection=False)))
    assert np.array_equal(a['delta'], b['delta']) and a['losses'] == b['losses']


def test_refusals(A, F, tmp_path):
    par, kw = _drv_inputs(F)
    N = par['N']
    run = lambda **over: A.reconstruct_ptychography(**_drv_kw(tmp_path, **dict(kw, **over)))
    with pytest.raises(NotImplementedError, match="pure_projection with unknown_type='real_imag'"):
        run(unknown_type='real_imag')
    with pytest.raises(NotImplementedError, match='pure_projection with is_minus_logged'):
        run(is_minus_logged=True)
    with pytest.raises(NotImplementedError, match="forward_algorithm='ctf'"):
        run(forward_algorithm='ctf')
    with pytest.raises(NotImplementedError, match='pure_projection with sparse multislice'):
        run(obj_size=(N, N, 2), slice_pos_cm_ls=[0, 10e-4], initial_guess=[np.zeros((N, N, 2)), np.zeros((N, N, 2))])
    with pytest.raises(NotImplementedError, match='pure_projection with multi-distance'):
        run(fname=np.ones((1, 2, N, N), np.float32), obj_size=(N, N, 1), two_d_mode=True, n_theta=1, probe_pos=np.array([(0., 0.)]),
            free_prop_cm=[1e-3, 2e-3], initial_guess=[np.zeros((N, N, 1)), np.zeros((N, N, 1))])
    with pytest.raises(NotImplementedError, match='pure_projection with optimize_prj_pos_offset'):
        run(optimize_prj_pos_offset=True, free_prop_cm=2e-4)
    with pytest.raises(NotImplementedError, match='pure_projection with rotate_out_of_loop'):
        run(rotate_out_of_loop=True)
    # the model refuses the same combinations by name, and an engine that does not project a volume
    ctx = A.Context(0)
    eng = A.MultisliceEngine(ctx, (N, N, 4), (8, 8), np.zeros((1, 2)), par['energy_ev'], par['psize_cm'], max_batch=1)
    for cv, what in ((dict(unknown_type='real_imag'), 'real_imag'), (dict(is_minus_logged=True), 'is_minus_logged'),
                     (dict(optimize_prj_pos_offset=True), 'optimize_prj_pos_offset'), (dict(rotate_out_of_loop=True), 'rotate_out_of_loop')):
        with pytest.raises(NotImplementedError, match='pure_projection with .*' + what):
            A.PtychographyModel(device=ctx, common_vars_dict=dict(engine=eng, pure_projection=True, **cv))
    with pytest.raises(NotImplementedError, match='pure_projection with multi-distance'):
        A.MultiDistModel(device=ctx, common_vars_dict=dict(engine=eng, pure_projection=True, holo_engine=None))
    with pytest.raises(ValueError, match='ProjectionEngine'):
        A.PtychographyModel(device=ctx, common_vars_dict=dict(engine=eng, pure_projection=True))
    eng.plan.close()
    ctx.close()
