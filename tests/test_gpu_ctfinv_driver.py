"""reconstruct_ptychography(update_using_external_algorithm='ctf', ctf_direct_update=True) on the GPU (pytest -m gpu): the delta
channel overwritten by the direct CTF inversion in every minibatch, kappa refined by the gradient of the data misfit.

Checker: tests/ctfinv_ref.drive in fp64 (the reference's own driver raises TypeError on this combination: golden F31,
'drv/external_ctf'), its float32 run as the yardstick: the bars are tests/ctfinv_matrix.DRV_BARS, 3 x the float32 restatement's
distances, held to those by tests/test_ctfinv_ref_vs_golden.py.  16 x 16 x 1 object, three distances, data made at lg_kappa 1.5,
kappa from 1.7, one minibatch per epoch, ten epochs."""
import os

import numpy as np
import pytest

from tests import ctfinv_matrix as M

pytestmark = pytest.mark.gpu


@pytest.fixture(scope='module')
def A():
    import adorym_amd
    return adorym_amd


def drv_kw(tmp_path, **over):
    c = M.drv_inputs()
    ny, nx, nd = M.DRV['field']
    obj = c['obj'].astype(np.float64)
    kw = dict(fname=c['data'][None], obj_size=(ny, nx, 1), probe_pos=np.array([[0., 0.]]), theta_st=0, theta_end=0, n_theta=1, two_d_mode=True,
              energy_ev=M.ENERGY_EV, psize_cm=M.PSIZE_CM, free_prop_cm=np.array(c['dists']), minibatch_size=1, n_epochs=M.DRV['n_epochs'],
              initial_guess=[obj[:, :, None, 0], obj[:, :, None, 1]], probe_type='plane', raw_data_type='intensity', unknown_type='delta_beta',
              gamma=0, alpha_d=0, alpha_b=0, optimizer='adam', learning_rate=M.DRV['learning_rate'], forward_algorithm='ctf', ctf_lg_kappa=M.LG_KAPPA,
              optimize_ctf_lg_kappa=True, ctf_lg_kappa_learning_rate=M.DRV['ctf_lg_kappa_learning_rate'], n_dp_batch=1, randomize_probe_pos=True,
              safe_zone_width=0, save_path=str(tmp_path), output_folder='out', store_checkpoint=False, use_checkpoint=False, return_state=True,
              update_using_external_algorithm='ctf', ctf_direct_update=True)
    kw.update(over)
    return c, kw


def same_bits(a, b, what):
    a, b = M.bits(np.asarray(a).reshape(-1)), M.bits(np.asarray(b).reshape(-1))
    assert a.shape == b.shape, what
    assert not (a != b).any(), (what, '%d of %d elements differ' % (int((a != b).sum()), a.size))


def test_driver_vs_restatement(A, tmp_path):
    """lg_kappa after every update, the final delta and the losses of at least 1e-9 against drive() in fp64; beta is where it was."""
    c, kw = drv_kw(tmp_path)
    st = A.reconstruct_ptychography(**kw)
    hist = np.asarray(st['ctf_lg_kappa_history'], np.float64)
    ref = M.drv_ref('float64')
    e = M.drv_errors(hist, st['delta'], st['losses'])
    print('lg_kappa', hist, 'fp64', ref['lg_kappa_trace'])
    print('losses', st['losses'], 'fp64', ref['losses'])
    print('distances from drive() in fp64: %r;  bars %r' % (e, M.DRV_BARS))
    for k, v in e.items():
        assert v <= M.DRV_BARS[k], (k, v, M.DRV_BARS[k])
    assert st['ctf_lg_kappa'][0] == np.float32(hist[-1])
    same_bits(st['beta'], c['obj'][..., 1], 'beta')
    # the first loss is the plain CTF run's: the hook acts behind the first gradient
    assert abs(st['losses'][0] / ref['losses'][0] - 1) < 1e-5


def test_first_update_is_the_inversion_at_the_starting_kappa(A, tmp_path):
    """After one minibatch the delta channel is CTFInversion.retrieve(holograms of angle 0, free_prop_cm, lg_kappa = 1.7) bit for bit
    -- kappa as it was BEFORE that minibatch's kappa step, which has moved it since -- and beta is untouched."""
    c, kw = drv_kw(tmp_path, n_epochs=1)
    st = A.reconstruct_ptychography(**kw)
    assert st['ctf_lg_kappa'][0] != np.float32(M.LG_KAPPA)
    ctx = A.Context(0)
    eng = A.CTFInversion(ctx, M.DRV['field'][:2], M.DRV['field'][2], M.ENERGY_EV, M.PSIZE_CM)
    want = eng.retrieve(ctx.array(c['data']), c['dists'], ctx.array(np.array([M.LG_KAPPA], np.float32))).get()[0]
    moved = eng.retrieve(ctx.array(c['data']), c['dists'], ctx.array(np.asarray(st['ctf_lg_kappa'], np.float32))).get()[0]
    del eng
    ctx.close()
    same_bits(st['delta'], want, 'delta after the first minibatch')
    assert (M.bits(moved) != M.bits(want)).any()
    same_bits(st['beta'], c['obj'][..., 1], 'beta')
    # without optimize_object the hook still writes delta
    st2 = A.reconstruct_ptychography(**drv_kw(tmp_path, n_epochs=1, output_folder='fixed_object', optimize_object=False)[1])
    same_bits(st2['delta'], want, 'delta with optimize_object=False')


def test_checkpoint_resume(A, tmp_path):
    """A run stopped after two epochs and resumed from its last checkpoint (taken in front of epoch 1) replays that minibatch from the
    stored object, moments and kappa.  Bit for bit the uninterrupted run's: the replayed loss, the delta the replayed minibatch leaves
    (the inversion at the checkpoint's kappa) and beta.  (kappa itself restarts Adam's moments on resume, as
    tests/test_gpu_ctf_driver.py records for the plain CTF run: the reference's checkpoint does not hold them.)"""
    common = dict(store_checkpoint=True, n_batch_per_checkpoint=1, output_folder='part', n_epochs=2)
    c, kw = drv_kw(tmp_path, **common)
    part = A.reconstruct_ptychography(**kw)
    ck = os.path.join(str(tmp_path), 'part', 'checkpoint')
    assert [int(v) for v in np.loadtxt(os.path.join(ck, 'checkpoint.txt'))] == [1, 0]
    res = A.reconstruct_ptychography(**drv_kw(tmp_path, use_checkpoint=True, **common)[1])
    assert len(part['losses']) == 2 and len(res['losses']) == 1 and res['losses'][0] == part['losses'][1]
    same_bits(res['delta'], part['delta'], 'delta of the resumed run')
    same_bits(res['beta'], part['beta'], 'beta of the resumed run')
    same_bits(res['beta'], c['obj'][..., 1], 'beta')
    assert np.abs(part['delta'].reshape(16, 16) - c['obj'][..., 0]).max() > 1e-3        # (the hook has replaced the starting delta)


def test_refusals(A, tmp_path):
    """What the direct update does not serve is refused by name."""
    c, kw = drv_kw(tmp_path)
    run = lambda **over: A.reconstruct_ptychography(**dict(kw, **over))
    ny = 16
    mask = np.ones((ny, ny, 1))
    for over, what in ((dict(update_using_external_algorithm='tie'), "update_using_external_algorithm='tie'"),
                       (dict(ctf_tomography=True), "update_using_external_algorithm='ctf' with ctf_tomography"),
                       (dict(forward_algorithm='fresnel', optimize_ctf_lg_kappa=False), "update_using_external_algorithm='ctf' with forward_algorithm='fresnel'"),
                       (dict(two_d_mode=False, obj_size=(ny, ny, 2), initial_guess=[np.zeros((ny, ny, 2))] * 2, ctf_tomography=True),
                        "update_using_external_algorithm='ctf' with ctf_tomography"),
                       (dict(two_d_mode=False, obj_size=(ny, ny, 2), initial_guess=[np.zeros((ny, ny, 2))] * 2),
                        "update_using_external_algorithm='ctf' with two_d_mode=False"),
                       (dict(free_prop_cm=1e-3, fname=c['data'][None, :1]), "forward_algorithm='ctf'"),
                       (dict(finite_support_mask_path=mask), "update_using_external_algorithm='ctf' with a finite support mask"),
                       (dict(ctf_direct_update=False), 'update_using_external_algorithm')):
        with pytest.raises(NotImplementedError, match=what.replace('(', r'\(').replace(')', r'\)')):
            run(**over)
    # the keyword alone changes nothing: bit for bit the plain CTF run
    a = run(update_using_external_algorithm=None, n_epochs=2, output_folder='kw')
    b = run(update_using_external_algorithm=None, ctf_direct_update=False, n_epochs=2, output_folder='plain')
    assert a['losses'] == b['losses'] and np.array_equal(a['delta'], b['delta']) and np.array_equal(a['ctf_lg_kappa_history'], b['ctf_lg_kappa_history'])
