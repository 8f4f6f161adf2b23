"""reconstruct_ptychography(optimize_ctf_lg_kappa=True, forward_algorithm='fresnel', fresnel_kappa=True) on the GPU (pytest -m gpu):
the single-material constraint around the 2-D field path and the 3-D fan-out path of multi-distance holography.

Checker: golden F34 (b), the reference driver's fp64 run with its own fp32 run as the yardstick (tests/golden/gen_f34_fresnel_kappa.py).
Losses: rtol = max(2e-4, 3 x the reference's own fp32 deviation), the rule of tests/test_gpu_multidist3d_driver.py; final object:
3 x the fp32 run's distance in units of the whole update, + 1e-4 of it, the same test's rule; ctf_lg_kappa after update k: 3 x the
fp32 run's deviation + k float32 spacings of [1, 2) -- the parameter lives in float32 here and in float64 in either run of the
reference, and every update rounds it once (tests/test_gpu_ctf_driver.py's rule).
"""
import ast
import os
import pickle

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENERGY_EV, PSIZE_CM = 8000., 1e-6
ULP = 2. ** -23


@pytest.fixture(scope='module')
def A():
    import adorym_amd
    return adorym_amd


@pytest.fixture(scope='module')
def F():
    return np.load(os.path.join(ROOT, 'tests', 'golden', 'F34_fresnel_kappa.npz'))


def drv_kw(F, tag, tmp_path, **over):
    par = ast.literal_eval(str(F[tag + '/params']))
    N, S = par['N'], par['S']
    two_d = S == 1
    kw = dict(fname=F[tag + '/prj'], obj_size=(N, N, S), probe_pos=np.array([(0., 0.)]), theta_st=0, theta_end=0 if two_d else np.pi,
              n_theta=par['n_theta'], two_d_mode=two_d, energy_ev=ENERGY_EV, psize_cm=PSIZE_CM, free_prop_cm=np.array(par['dists_cm']),
              minibatch_size=1, n_epochs=par['n_epochs'], optimizer='adam', learning_rate=par['learning_rate'],
              initial_guess=[F[tag + '/guess_delta'].astype(np.float64), F[tag + '/guess_beta'].astype(np.float64)], probe_type='supplied',
              probe_initial=[F[tag + '/probe_mag'], F[tag + '/probe_phase']], raw_data_type=par['raw_data_type'], unknown_type='delta_beta',
              gamma=0, alpha_d=0, alpha_b=0, forward_algorithm='fresnel', ctf_lg_kappa=par['lg_kappa'], optimize_ctf_lg_kappa=True,
              ctf_lg_kappa_learning_rate=par['ctf_lg_kappa_learning_rate'], fresnel_kappa=True, n_dp_batch=1, safe_zone_width=0,
              save_path=str(tmp_path), output_folder='out', store_checkpoint=False, use_checkpoint=False, return_state=True)
    kw.update(over)
    return par, kw


@pytest.mark.parametrize('tag', ['drv2d', 'drv3d'])
def test_driver_vs_reference(A, F, tmp_path, tag):
    """The runs of golden F34 (b): every loss, the final object and ctf_lg_kappa after every update (return_state carries value and
    history, one entry per update); beta does not move; the 2-D run takes the separate launches, not the fused Adam path."""
    par, kw = drv_kw(F, tag, tmp_path)
    fused = []
    if tag == 'drv2d':
        orig = A.HolographyEngine.forward_adjoint_adam
        A.HolographyEngine.forward_adjoint_adam = lambda self, *a, **k: fused.append(1) or orig(self, *a, **k)
    try:
        st = A.reconstruct_ptychography(**kw)
    finally:
        if tag == 'drv2d':
            A.HolographyEngine.forward_adjoint_adam = orig
    assert not fused
    n_up = par['n_epochs'] * par['n_theta']
    l64, l32 = F[tag + '/fp64/losses'], F[tag + '/fp32/losses']
    e_l, dev = np.abs(np.asarray(st['losses']) / l64 - 1).max(), np.abs(l32 / l64 - 1).max()
    print(tag, 'losses', st['losses'], list(l64), 'worst %.2e (fp32 ref %.2e)' % (e_l, dev))
    assert len(st['losses']) == len(l64) == n_up
    assert np.allclose(st['losses'], l64, rtol=max(2e-4, 3 * dev), atol=0)
    x64 = F[tag + '/fp64/obj']
    x0 = np.stack([F[tag + '/guess_delta'], F[tag + '/guess_beta']], -1).astype(np.float64)
    x = np.stack([st['delta'], st['beta']], -1).astype(np.float64).reshape(x64.shape)
    upd = np.linalg.norm(x64 - x0)
    e, e_ref = np.linalg.norm(x - x64) / upd, float(F[tag + '/fp32/obj_err'])
    print(tag, 'object %.2e of the update (fp32 ref %.2e)' % (e, e_ref))
    assert upd > 0 and e <= 3 * e_ref + 1e-4, (e, e_ref)
    assert np.array_equal(x[..., 1], x0[..., 1].astype(np.float32).astype(np.float64))          # dL/dbeta = 0: Adam leaves beta where it was
    t64 = F[tag + '/fp64/lg_kappa_trace']
    hist = np.asarray(st['ctf_lg_kappa_history'], np.float64)
    assert hist.shape == t64.shape == (n_up,) and st['ctf_lg_kappa'].shape == (1,) and st['ctf_lg_kappa'][0] == np.float32(hist[-1])
    bound = 3 * F[tag + '/fp32/lg_kappa_err'] + np.arange(1, n_up + 1) * ULP
    print(tag, 'ctf_lg_kappa', hist, 'fp64', t64, 'off by', np.abs(hist - t64), 'bound', bound)
    assert (np.abs(hist - t64) <= bound).all()
    assert abs(t64[-1] - par['lg_kappa']) > 100 * bound[-1]                                     # (a bound the parameter's own movement exceeds)


@pytest.mark.parametrize('tag', ['drv2d', 'drv3d'])
def test_resumed_run_continues_bit_for_bit(A, F, tmp_path, tag):
    """A run stopped after its first epoch and resumed from its last checkpoint replays that minibatch and the rest: ctf_lg_kappa and
    its Adam moments travel in params_0 under the keys of the CTF runs, so losses, object and kappa are the uninterrupted run's."""
    par, kw = drv_kw(F, tag, tmp_path)
    n = par['n_theta']
    whole = A.reconstruct_ptychography(**dict(kw, output_folder='whole'))
    common = dict(store_checkpoint=True, n_batch_per_checkpoint=1, output_folder='part')
    A.reconstruct_ptychography(**dict(kw, n_epochs=1, **common))
    ck = os.path.join(str(tmp_path), 'part', 'checkpoint')
    assert [int(v) for v in np.loadtxt(os.path.join(ck, 'checkpoint.txt'))] == [0, n - 1]
    with open(os.path.join(ck, 'params_0'), 'rb') as f:
        params = pickle.load(f)
    assert np.asarray(params['ctf_lg_kappa']).shape == (1,) and len(params['ctf_lg_kappa_moments']) == 2
    res = A.reconstruct_ptychography(**dict(kw, use_checkpoint=True, **common))
    k = len(res['losses'])
    assert k == (par['n_epochs'] - 1) * n + 1
    assert np.array_equal(res['losses'], whole['losses'][-k:])
    assert np.array_equal(res['delta'], whole['delta']) and np.array_equal(res['beta'], whole['beta'])
    assert res['ctf_lg_kappa'][0] == whole['ctf_lg_kappa'][0] != np.float32(par['lg_kappa'])
    assert np.array_equal(res['ctf_lg_kappa_history'], whole['ctf_lg_kappa_history'][-k:])


@pytest.mark.parametrize('extra', [dict(optimize_free_prop=True, fanout_free_prop=True, free_prop_learning_rate=1e-6),
                                   dict(optimize_probe=True, probe_learning_rate=1e-3),
                                   dict(optimizer='cg', device_cg=True)], ids=['free_prop', 'probe', 'cg'])
def test_it_composes(A, F, tmp_path, extra):
    """One short 3-D run each with fanout_free_prop, with optimize_probe and with the conjugate-gradient optimiser (whose trial losses
    run on the tied object): it completes, kappa moves and the loss of every angle falls from the first epoch to the last."""
    par, kw = drv_kw(F, 'drv3d', tmp_path, n_epochs=3, learning_rate=1e-5, **extra)
    st = A.reconstruct_ptychography(**kw)
    n = par['n_theta']
    losses = np.asarray(st['losses'])
    print(extra, losses, st['ctf_lg_kappa'])
    assert len(losses) == 3 * n and np.all(np.isfinite(losses))
    assert np.mean(losses[-n:]) < np.mean(losses[:n])
    assert len(st['ctf_lg_kappa_history']) == 3 * n and st['ctf_lg_kappa'][0] != np.float32(par['lg_kappa'])
    if 'optimize_probe' in extra:
        p0 = F['drv3d/probe_mag'] * np.exp(1j * F['drv3d/probe_phase'])
        assert np.abs((st['probe_real'] + 1j * st['probe_imag'])[0] - p0).max() > 1e-4
    if 'optimize_free_prop' in extra:
        assert st['free_prop_cm_history'] is not None and len(st['free_prop_cm_history']) == 3 * n


def test_it_composes_with_registration(A, F, tmp_path):
    """... and with fanout_prj_affine (the holograms registered in front of the launch on the tied object)."""
    par, kw = drv_kw(F, 'drv3d', tmp_path, n_epochs=2, optimize_prj_affine=True, fanout_prj_affine=True, prj_affine_learning_rate=1e-4)
    st = A.reconstruct_ptychography(**kw)
    assert np.all(np.isfinite(st['losses'])) and len(st['prj_affine_history']) == 2 * par['n_theta']
    assert st['ctf_lg_kappa'][0] != np.float32(par['lg_kappa'])


def test_refusals(A, F, tmp_path):
    """fresnel_kappa=True alone is a ValueError; without the keyword the old message; what the constraint does not serve is refused
    by name."""
    par, kw = drv_kw(F, 'drv2d', tmp_path)
    with pytest.raises(ValueError, match='fresnel_kappa=True needs optimize_ctf_lg_kappa=True'):
        A.reconstruct_ptychography(**dict(kw, optimize_ctf_lg_kappa=False))
    off = dict(kw)
    off.pop('fresnel_kappa')
    with pytest.raises(NotImplementedError, match="optimize_ctf_lg_kappa with forward_algorithm='fresnel'"):
        A.reconstruct_ptychography(**off)
    with pytest.raises(ValueError, match="fresnel_kappa=True needs forward_algorithm='fresnel'"):
        A.reconstruct_ptychography(**dict(kw, forward_algorithm='ctf'))
    what = "optimize_ctf_lg_kappa with forward_algorithm='fresnel' and %s"
    for extra, name in ((dict(unknown_type='real_imag'), "unknown_type='real_imag'"), (dict(optimize_all_probe_pos=True), 'optimize_all_probe_pos'),
                        (dict(safe_zone_width=2), 'data divided into sub-tiles or safe_zone_width > 0')):
        with pytest.raises(NotImplementedError, match=what % name):
            A.reconstruct_ptychography(**dict(kw, **extra))
