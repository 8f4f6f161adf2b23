"""Per-angle projection alignment through PtychographyModel and reconstruct_ptychography (optimize_prj_pos_offset) on the GPU
(pytest -m gpu).

Checkers: golden F24 (the reference driver in fp64, its own fp32 run as the yardstick; tests/golden/gen_f24_prj_offset.py) and
the NumPy restatement tests/prj_offset_ref.py.  Floors of the 3x rule: losses 2e-4 and object 1e-4 of the update as in
tests/test_gpu_e2e.py; offsets 32 * 2^-24 of the distance they have moved -- they live in fp32 and each of the 8 updates
rounds about four times (the gradient as it is stored, the step, the subtraction, the value kept).
"""
import ast
import os
import pickle
import socket
import sys

import numpy as np
import pytest

from tests import prj_offset_ref as PR
import cases

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENERGY_EV, PSIZE_CM = 8000., 1e-6
OFFSET_FLOOR = 32 * 2. ** -24


@pytest.fixture(scope='module')
def A():
    import adorym_amd
    return adorym_amd


@pytest.fixture(scope='module')
def F():
    return np.load(os.path.join(ROOT, 'tests', 'golden', 'F24_prj_offset.npz'))


def _drv_kw(tmp_path, **kw):
    base = dict(theta_st=0, theta_end=np.pi, energy_ev=ENERGY_EV, psize_cm=PSIZE_CM, gamma=0, alpha_d=0, alpha_b=0, optimizer='adam',
                save_path=str(tmp_path), output_folder='out', store_checkpoint=False, use_checkpoint=False, return_state=True)
    base.update(kw)
    return base


def _drv_inputs(F):
    par = ast.literal_eval(str(F['drv/params']))
    N = par['N']
    kw = dict(fname=F['drv/prj'], obj_size=(N, N, N), probe_pos=np.array([(0., 0.)]), n_theta=par['n_theta'], free_prop_cm=par['free_prop_cm'],
              minibatch_size=1, n_epochs=par['n_epochs'], learning_rate=par['learning_rate'],
              initial_guess=[F['drv/guess_delta'].astype(np.float64), F['drv/guess_beta'].astype(np.float64)], probe_type='supplied',
              probe_initial=[F['drv/probe_mag'], F['drv/probe_phase']], optimize_prj_pos_offset=True,
              prj_pos_offset_learning_rate=par['prj_pos_offset_learning_rate'])
    return par, kw


def _check_driver(st, F, run):
    t64, t32 = 'drv/%s_fp64/' % run, 'drv/%s_fp32/' % run
    l64, l32 = F[t64 + 'losses'], F[t32 + 'losses']
    assert len(st['losses']) == len(l64)
    print('losses', st['losses'], l64)
    assert np.allclose(st['losses'], l64, rtol=max(2e-4, 3 * np.abs(l32 / l64 - 1).max()))
    x64 = np.stack([F[t64 + 'delta'], F[t64 + 'beta']], -1).astype(np.float64)
    x32 = np.stack([F[t32 + 'delta'], F[t32 + 'beta']], -1).astype(np.float64)
    x0 = np.stack([F['drv/guess_delta'], F['drv/guess_beta']], -1).astype(np.float64)
    x = np.stack([st['delta'], st['beta']], -1).astype(np.float64)
    upd = np.linalg.norm(x64 - x0)
    e, e_ref = np.linalg.norm(x - x64) / upd, np.linalg.norm(x32 - x64) / upd
    print('object', e, e_ref)
    assert upd > 0 and e <= 3 * e_ref + 1e-4, (e, e_ref)
    o64, o32 = F[t64 + 'offset_trace'], F[t32 + 'offset_trace']
    oh = st['prj_pos_offset_history'].astype(np.float64)
    assert oh.shape == o64.shape
    for k in range(len(o64)):
        moved = np.linalg.norm(o64[k])
        e, e_ref = np.linalg.norm(oh[k] - o64[k]) / moved, np.linalg.norm(o32[k] - o64[k]) / moved
        print('offsets after update %d' % k, oh[k].ravel(), o64[k].ravel(), e, e_ref)
        assert moved > 0 and e <= 3 * e_ref + OFFSET_FLOOR, (k, oh[k], o64[k], e, e_ref)
    assert np.array_equal(st['prj_pos_offset'], st['prj_pos_offset_history'][-1])


def test_driver_default_gd_vs_reference(A, F, tmp_path):
    """No optimiser given: the reference's default, gradient descent with a constant step (optimizers.py:863-875)."""
    par, kw = _drv_inputs(F)
    st = A.reconstruct_ptychography(**_drv_kw(tmp_path, save_intermediate=True, **kw))
    _check_driver(st, F, 'gd')
    # one line per update (save_intermediate_level = 'batch', the default): epoch, batch, the offsets (optimizers.py:1135-1138)
    with open(os.path.join(st['output_folder'], 'intermediate', 'prj_pos_offset', 'prj_pos_offset.txt')) as f:
        lines = f.read().strip().split('\n')
    assert len(lines) == par['n_epochs'] * par['n_theta']
    for k, line in enumerate(lines):
        e_, b_, rest = line.split(',', 2)
        assert (int(e_), int(b_)) == divmod(k, par['n_theta'])
        assert np.array_equal(np.array(ast.literal_eval(rest.strip()), np.float32), st['prj_pos_offset_history'][k].ravel())


def test_driver_supplied_adam_vs_reference(A, F, tmp_path):
    par, kw = _drv_inputs(F)
    opt = A.AdamOptimizer('prj_pos_offset', output_folder=str(tmp_path), options_dict={'step_size': par['adam_step']})
    st = A.reconstruct_ptychography(**_drv_kw(tmp_path, optimizer_prj_pos_offset=opt, **kw))
    _check_driver(st, F, 'adam')


def test_model_returns_a_dense_gradient_at_the_arguments_place(A, F, tmp_path):
    """PtychographyModel.loss_and_gradients: the gradient w.r.t. prj_pos_offset is [n_theta, 2], zero outside the minibatch's angle,
    and the restatement's value inside it."""
    from oracle import adorym_oracle as O
    par, kw = _drv_inputs(F)
    N, n_theta = par['N'], par['n_theta']
    ctx = A.Context(0)
    eng = A.MultisliceEngine(ctx, (N, N, N), (N, N), np.zeros((1, 2)), ENERGY_EV, PSIZE_CM, free_prop_cm=par['free_prop_cm'], max_batch=1,
                             exit_shift=True)
    theta_ls = np.linspace(0, np.pi, n_theta, dtype='float32')
    tables = {}
    cv = dict(engine=eng, prj=F['drv/prj'], optimize_prj_pos_offset=True, two_d_mode=False, theta_ls=theta_ls,
              rotation_tables=lambda i: tables.setdefault(i, A.RotationTable(ctx, (N, N, N), theta_ls[i])))
    fm = A.PtychographyModel(device=ctx, common_vars_dict=cv)
    fm.prj = F['drv/prj']
    offs = np.array(par['true_offsets']) * 0.5
    obj = np.stack([F['drv/guess_delta'], F['drv/guess_beta']], -1).astype(np.float32)
    probe = F['drv/probe_mag'] * np.exp(1j * F['drv/probe_phase'])
    i_po = fm.get_argument_index('prj_pos_offset')
    grad = ctx.zeros(obj.shape)
    i_theta = 2
    out = fm.loss_and_gradients([0, i_po], grad, ctx.array(obj), probe.real[None], probe.imag[None], 0., None, i_theta, np.zeros((1, 2), int),
                                None, None, np.array([0]), None, offs)
    g = out[1].get()
    phys = O.Physics((N, N), ENERGY_EV, PSIZE_CM, free_prop_cm=par['free_prop_cm'])
    ref = {dt: PR.forward_adjoint_object(obj.astype(np.float64), O.rotation_coords((N, N, N), theta_ls[i_theta], dt), probe,
                                         np.zeros((1, 2), int), F['drv/prj'][i_theta, [0]].astype(np.float64), phys, offs,
                                         np.array([i_theta]), dt) for dt in ('float64', 'float32')}
    assert g.shape == (n_theta, 2) and np.all(g[[0, 1, 3]] == 0)
    e = np.linalg.norm(g[i_theta] - ref['float64'][4][i_theta]) / np.linalg.norm(ref['float64'][4][i_theta])
    e32 = np.linalg.norm(ref['float32'][4][i_theta] - ref['float64'][4][i_theta]) / np.linalg.norm(ref['float64'][4][i_theta])
    print('model dL/d prj_pos_offset', g[i_theta], ref['float64'][4][i_theta], e, e32)
    assert e <= 3 * e32 + 2. ** -24
    eng.plan.close()
    ctx.close()


def test_refusals(A, tmp_path):
    N, P = 30, 16
    prj = np.ones((2, 2, P, P), np.float32)
    guess = [np.zeros((N, N, 2)), np.zeros((N, N, 2))]
    kw = _drv_kw(tmp_path, fname=prj, obj_size=(N, N, 2), probe_pos=np.array([(0., 0.), (4., 6.)]), probe_type='plane', initial_guess=guess,
                 n_epochs=1, minibatch_size=2, n_theta=2, free_prop_cm=2e-4, optimize_prj_pos_offset=True)
    with pytest.raises(NotImplementedError, match='optimize_prj_pos_offset with sub-pixel'):
        A.reconstruct_ptychography(**dict(kw, optimize_all_probe_pos=True))
    with pytest.raises(NotImplementedError, match='optimize_prj_pos_offset with sub-pixel'):
        A.reconstruct_ptychography(**dict(kw, probe_pos=np.array([(0., 0.), (4.5, 6.)])))
    with pytest.raises(NotImplementedError, match='optimize_prj_pos_offset with sparse multislice'):
        A.reconstruct_ptychography(**dict(kw, slice_pos_cm_ls=[0, 10e-4]))
    with pytest.raises(NotImplementedError, match='optimize_prj_pos_offset with multi-distance'):
        A.reconstruct_ptychography(**dict(kw, fname=np.ones((1, 4, P, P), np.float32), obj_size=(N, N, 1), two_d_mode=True, n_theta=1,
                                          free_prop_cm=[1e-3, 2e-3], initial_guess=[np.zeros((N, N, 1)), np.zeros((N, N, 1))]))
    # the models that do not serve the flag refuse it by name
    ctx = A.Context(0)
    eng = A.MultisliceEngine(ctx, (N, N, 2), (P, P), np.zeros((1, 2)), ENERGY_EV, PSIZE_CM, max_batch=1, slice_pos_cm=[0., 1e-3])
    sm = A.SparseMultisliceModel(device=ctx, common_vars_dict=dict(engine=eng, optimize_prj_pos_offset=True))
    with pytest.raises(NotImplementedError, match='optimize_prj_pos_offset'):
        sm._check_static(0., None, None, np.zeros((2, 2)))
    eng.plan.close()
    ctx.close()


def test_far_field_is_accepted_with_a_warning(A, F, tmp_path):
    par, kw = _drv_inputs(F)
    with pytest.warns(UserWarning, match='offsets cannot move'):
        st = A.reconstruct_ptychography(**_drv_kw(tmp_path, **dict(kw, free_prop_cm='inf', n_epochs=1)))
    assert np.all(st['prj_pos_offset'] == 0) and np.all(np.isfinite(st['losses']))


def test_checkpoint_resume_gives_the_same_offsets(A, F, tmp_path):
    """A run stopped after its first epoch and resumed from the last checkpoint ends with the offsets of the uninterrupted run,
    bit for bit; params_0 carries them under the reference's key."""
    par, kw = _drv_inputs(F)
    whole = A.reconstruct_ptychography(**_drv_kw(tmp_path, output_folder='whole', **kw))
    common = dict(store_checkpoint=True, n_batch_per_checkpoint=1, output_folder='part')
    part = A.reconstruct_ptychography(**_drv_kw(tmp_path, **dict(kw, n_epochs=1, **common)))
    with open(os.path.join(part['output_folder'], 'checkpoint', 'params_0'), 'rb') as f:
        saved = pickle.load(f)
    assert 'prj_pos_offset' in saved
    # (the last checkpoint is written in front of the epoch's last minibatch)
    assert np.array_equal(np.asarray(saved['prj_pos_offset'], np.float32), part['prj_pos_offset_history'][-2])
    res = A.reconstruct_ptychography(**_drv_kw(tmp_path, **dict(kw, use_checkpoint=True, **common)))
    assert np.array_equal(res['prj_pos_offset'], whole['prj_pos_offset'])
    assert np.array_equal(res['prj_pos_offset_history'], whole['prj_pos_offset_history'][par['n_theta'] - 1:])


# ------------------------------------------------------------------------------------------------------------ two ranks
def _free_port():
    s = socket.socket(); s.bind(('127.0.0.1', 0)); p = s.getsockname()[1]; s.close()
    return p


def _worker(rank, world, port, tmp, q):
    """One rank: a fresh process that has not touched the GPU before (the pattern of tests/test_gpu_world2.py)."""
    sys.path.insert(0, ROOT)
    sys.path.insert(0, os.path.join(ROOT, 'tests', 'golden'))
    os.environ.update(RANK=str(rank), WORLD_SIZE=str(world), LOCAL_RANK='0', MASTER_ADDR='127.0.0.1', MASTER_PORT=str(port), ADM_COMM='host')
    try:
        import adorym_amd as A
        from adorym_amd import comm as C
        F = np.load(os.path.join(ROOT, 'tests', 'golden', 'F24_prj_offset.npz'))
        par, kw = _drv_inputs(F)
        comm = C.from_env()
        assert type(comm) is C.HostStagedComm and comm.size == world
        st = A.reconstruct_ptychography(comm=comm, **_drv_kw(tmp, **kw))
        comm.close()
        q.put(dict(rank=rank, off=st['prj_pos_offset'], hist=st['prj_pos_offset_history'], losses=np.array(st['losses'])))
    except Exception as e:       # report instead of leaving the parent waiting for the queue
        import traceback
        q.put(dict(rank=rank, error='%r\n%s' % (e, traceback.format_exc())))


def test_world2_offsets(F, tmp_path):
    """Two ranks on one GPU (host-staged transport), each with one angle of every global batch: the offset gradients are summed over
    the ranks, so both end with the same offsets -- those of the two-rank restatement (fp64, its fp32 run as the yardstick)."""
    import multiprocessing as mp
    from oracle import adorym_oracle as O
    world, port = 2, _free_port()
    os.environ['ADM_RDV_TOKEN'] = __import__('secrets').token_hex(16)
    mpc = mp.get_context('spawn')
    q = mpc.Queue()
    procs = [mpc.Process(target=_worker, args=(r, world, port, str(tmp_path), q)) for r in range(world)]
    [p.start() for p in procs]
    res = [q.get(timeout=600) for _ in procs]
    [p.join(120) for p in procs]
    for r in res:
        assert 'error' not in r, r['error']
    res = sorted(res, key=lambda r: r['rank'])
    assert np.array_equal(res[0]['off'], res[1]['off']) and np.array_equal(res[0]['hist'], res[1]['hist'])
    par, kw = _drv_inputs(F)
    probe = F['drv/probe_mag'] * np.exp(1j * F['drv/probe_phase'])
    phys = O.Physics(probe.shape, ENERGY_EV, PSIZE_CM, free_prop_cm=par['free_prop_cm'])
    theta_ls = np.linspace(0, np.pi, par['n_theta'], dtype='float32')
    runs = {dt: PR.reconstruct(F['drv/prj'].astype(np.float64), kw['initial_guess'], probe, np.zeros((1, 2)), phys, theta_ls,
                               n_epochs=par['n_epochs'], minibatch_size=1, learning_rate=par['learning_rate'],
                               prj_pos_offset_learning_rate=par['prj_pos_offset_learning_rate'], n_ranks=world, dtype=dt)
            for dt in ('float64', 'float32')}
    o64, o32, oh = runs['float64']['offset_history'], runs['float32']['offset_history'], res[0]['hist'].astype(np.float64)
    assert oh.shape == o64.shape
    for k in range(len(oh)):
        moved = np.linalg.norm(o64[k])
        e, e_ref = np.linalg.norm(oh[k] - o64[k]) / moved, np.linalg.norm(o32[k] - o64[k]) / moved
        print('offsets after update %d' % k, oh[k].ravel(), o64[k].ravel(), e, e_ref)
        assert moved > 0 and e <= 3 * e_ref + OFFSET_FLOOR, (k, e, e_ref)


# ------------------------------------------------------------------------------------------------------------ recovery
@pytest.mark.regression
def test_offsets_are_recovered(A, tmp_path):
    """The object starts at the truth and practically does not move; the data come from offsets of +-0.5 px; gradient descent with
    the step chosen on the CPU (PR.RECOVERY, tests/test_prj_offset_ref_vs_golden.py: the restatement reaches 0.02 px in 40 updates)
    must bring the offsets within 0.05 px."""
    R = PR.RECOVERY
    N = R['N']
    truth, probe, theta_ls, phys, prj = PR.recovery_inputs(cases.smooth_field)
    st = A.reconstruct_ptychography(**_drv_kw(
        tmp_path, fname=prj.astype(np.float32), obj_size=(N, N, N), probe_pos=np.array([(0., 0.)]), n_theta=R['n_theta'],
        free_prop_cm=R['free_prop_cm'], minibatch_size=1, n_epochs=R['n_epochs'], learning_rate=1e-12,
        initial_guess=[truth[..., 0], truth[..., 1]], probe_type='supplied', probe_initial=[np.abs(probe), np.angle(probe)],
        optimize_prj_pos_offset=True, prj_pos_offset_learning_rate=R['step']))
    err = np.abs(st['prj_pos_offset'].astype(np.float64) - np.array(R['true_offsets']))
    print('offsets', st['prj_pos_offset'].ravel(), 'error', err.max())
    assert len(st['prj_pos_offset_history']) == 40 and err.max() < 0.05
