"""reconstruct_ptychography with the conjugate-gradient object optimiser against the reference driver's runs (golden F33, runs a - e
of tests/cg_matrix.py): the decision sequence of every line search is the golden's, the logged losses and the final object are
within 3 x the reference's own fp32-from-fp64 distance.  Also: the instance form and optimizer='cg' with device_cg=True give the same
bits; a run checkpointed inside an epoch and resumed continues the uninterrupted one bit for bit; the 2-D run's losses never rise;
a loss evaluation at a trial point leaves nothing behind that the next gradient reuses; every refusal names what it refuses."""
import os

import numpy as np
import pytest

import cases
from tests import cg_matrix as CM

pytestmark = pytest.mark.gpu
G = os.path.join(os.path.dirname(__file__), 'golden')


@pytest.fixture(scope='module')
def golden():
    return np.load(os.path.join(G, 'F33_cg.npz'))


@pytest.fixture(scope='module')
def prj3d():
    return np.load(os.path.join(G, 'F6_e2e.npz'))['prj']


def recording():
    import adorym_amd as A

    class Recording(A.CGOptimizer):
        def __init__(self, *a, **k):
            super(Recording, self).__init__(*a, **k)
            self.log, self.hook = [], None

        def apply_gradient(self, x, gradient, i_batch=None, **kw):
            if self.hook is not None:
                self.hook(self, x, gradient, i_batch)
            out = super(Recording, self).apply_gradient(x, gradient, i_batch, **kw)
            self.log.append(self.last)
            return out
    return Recording


def drive(g, prj3d, name, tmp_path, opt=None, **extra):
    import adorym_amd as A
    params = CM.driver_params(g, name, cases.e2e_inputs(), cases.E2E, prj3d, tmp_path)
    params.update(extra)
    if opt is not None:
        params['optimizer'] = opt
    return A.reconstruct_ptychography(**params)


@pytest.mark.parametrize('name', list(CM.RUNS))
def test_driver_matches_the_reference_run(golden, prj3d, name, tmp_path):
    g = golden
    opt = recording()('obj', options_dict=CM.options(g, name))
    st = drive(g, prj3d, name, tmp_path, opt)
    log = opt.log
    # the decision sequence
    assert len(log) == int(g[name + '_n_updates'])
    assert [u['step_count'] for u in log] == list(g[name + '_n_trials'])
    assert [u['i_batch'] for u in log] == list(g[name + '_i_batch'])
    assert [u['beta_raw'] < 0 for u in log] == list(g[name + '_beta_raw'] < 0)
    assert [u['descends'] for u in log] == list(g[name + '_descent_check'] < 0)
    assert [u['alpha'] == 0 for u in log] == list(g[name + '_alpha'] == 0)
    assert opt.i_line_search_step == int(g[name + '_n_trials'].sum()) and opt.i_batch == len(log)
    # losses and the final object: 3 x the reference's own fp32 distance (the object on cg_matrix.obj_sample's voxels, like the golden)
    l64 = g[name + '_losses']
    e_loss = np.max(np.abs(np.asarray(st['losses']) - l64) / np.abs(l64))
    x = CM.sampled(np.stack([st['delta'], st['beta']], -1).astype(np.float64))
    e_obj = np.linalg.norm(x - g[name + '_obj'])
    print('%s: losses %.2e (reference fp32 %.2e), object %.2e (reference fp32 %.2e, update %.2e), trials %s'
          % (name, e_loss, g[name + '_dist_losses'], e_obj, g[name + '_dist_obj'], g[name + '_update_norm'], [u['step_count'] for u in log]))
    assert len(st['losses']) == len(l64) and e_loss <= CM.THREE * float(g[name + '_dist_losses'])
    assert e_obj <= CM.THREE * float(g[name + '_dist_obj'])
    if name == 'd':
        assert (np.diff(st['losses']) <= 0).all()           # one minibatch per epoch: an accepted point never has a higher loss
        assert all(u['beta'] == 0 for u in log)
    if name == 'c':
        assert all(u['alpha'] == 0 and u['step_count'] == 2 for u in log)
    if name == 'e':
        assert (st['delta'] >= 0).all() and (st['beta'] >= 0).all() and ((st['delta'] == 0).any() or (st['beta'] == 0).any())


def test_instance_and_keyword_give_the_same_bits(golden, prj3d, tmp_path):
    import adorym_amd as A
    g = golden
    lr = float(g['a_learning_rate'])
    a = drive(g, prj3d, 'a', tmp_path / 'i', A.CGOptimizer('obj', options_dict={'step_size': lr}), n_epochs=1)
    b = drive(g, prj3d, 'a', tmp_path / 'k', optimizer='cg', learning_rate=lr, device_cg=True, n_epochs=1)
    assert a['losses'] == b['losses'] and np.array_equal(a['delta'], b['delta']) and np.array_equal(a['beta'], b['beta'])
    # without the keyword the string is refused as before
    with pytest.raises(NotImplementedError, match="optimizer 'cg' is outside the accelerated path"):
        drive(g, prj3d, 'a', tmp_path / 'n', optimizer='cg', learning_rate=lr, n_epochs=1)


def test_resume_inside_an_epoch_continues_bit_for_bit(golden, prj3d, tmp_path):
    """Run b's setting (12 minibatches per epoch, searches that backtrack), one epoch, a checkpoint every 5 minibatches.  The
    interrupted run stops after minibatch 7: its last checkpoint is (epoch 0, batch 5), with descent_dir_old and s in the place of
    Adam's m and v.  optimizer_batch_number_increment='batch': the resumed step counter is then the uninterrupted one's."""
    g = golden
    lr = float(g['b_learning_rate'])
    kw = dict(optimizer='cg', learning_rate=lr, device_cg=True, n_epochs=1, store_checkpoint=True, n_batch_per_checkpoint=5,
              optimizer_batch_number_increment='batch')
    full = drive(g, prj3d, 'b', tmp_path / 'full', **kw)
    R = recording()

    class Stop(Exception):
        pass

    def stop_at_7(opt, x, gradient, i_batch):
        if len(opt.log) == 7:
            raise Stop()
    cut = R('obj', options_dict={'step_size': lr})
    cut.hook = stop_at_7
    with pytest.raises(Stop):
        drive(g, prj3d, 'b', tmp_path / 'cut', cut, **dict(kw, optimizer=cut))
    ck = os.path.join(str(tmp_path / 'cut'), 'out', 'checkpoint')
    import threading
    for t in threading.enumerate():     # (the files are written by a helper thread, which the interrupted run did not wait for)
        if t is not threading.current_thread() and not t.daemon:
            t.join(timeout=30)
    assert [int(v) for v in np.loadtxt(os.path.join(ck, 'checkpoint.txt'))] == [0, 5]
    assert np.load(os.path.join(ck, 'opt_obj_params_checkpoint.npy')).shape == (2, 32, 32, 32, 2)
    res = drive(g, prj3d, 'b', tmp_path / 'cut', use_checkpoint=True, **kw)
    assert res['losses'] == full['losses'][5:]
    assert np.array_equal(res['delta'], full['delta']) and np.array_equal(res['beta'], full['beta'])


@pytest.mark.parametrize('name', ['a', 'd'])
def test_a_trial_evaluation_leaves_nothing_behind(golden, prj3d, name, tmp_path):
    """The gradient the driver computes after an update -- whose search evaluated the loss at trial points, in another buffer --
    equals, bit for bit, the gradient a fresh run's model computes for the same object and minibatch without any loss-only
    evaluation before it: the rotated object and its slice-transmission cache are rebuilt from the array every evaluation is handed
    (3-D, run a), and so is the thin object that skips the rotation (2-D, run d)."""
    g = golden
    R = recording()
    seen = []

    def capture(opt, x, gradient, i_batch):
        fm = gradient.forward_model
        seen.append(dict(x=x.get(), g=gradient.arr.get(), theta=int(fm.loss_args['this_i_theta']),
                         pos=np.array(fm.loss_args['this_pos_batch']), ind=np.array(fm.loss_args['this_ind_batch'])))
    first = R('obj', options_dict=CM.options(g, name))
    first.hook = capture
    drive(g, prj3d, name, tmp_path / 'first', first, n_epochs=1 if name == 'a' else 3)
    assert len(seen) >= 3 and all(u['step_count'] >= 1 for u in first.log)
    fresh_grads = []

    def replay(opt, x, gradient, i_batch):
        if fresh_grads:
            return
        fm = gradient.forward_model
        ctx = x.ctx
        for st in seen[1:]:
            obj, buf = ctx.array(st['x']), ctx.empty(st['g'].shape)
            args = dict(fm.loss_args, obj=obj, this_i_theta=st['theta'], this_pos_batch=st['pos'], this_ind_batch=st['ind'])
            fm.loss_and_gradients([0], buf, _init_grad=True, **args)
            fresh_grads.append(buf.get())
    second = R('obj', options_dict=CM.options(g, name))
    second.hook = replay
    drive(g, prj3d, name, tmp_path / 'second', second, n_epochs=1)
    assert len(fresh_grads) == len(seen) - 1
    for k, (st, fg) in enumerate(zip(seen[1:], fresh_grads)):
        assert np.abs(st['g']).max() > 0
        assert np.array_equal(st['g'].view(np.uint32), fg.view(np.uint32)), k


def test_refusals_name_what_they_refuse(golden, prj3d, tmp_path):
    import adorym_amd as A
    g = golden
    mk = lambda: A.CGOptimizer('obj', options_dict={'step_size': 1e-4})
    for extra, what in ((dict(update_scheme='per angle'), "CGOptimizer with update_scheme='per angle'"),
                        (dict(rotate_out_of_loop=True), 'CGOptimizer with rotate_out_of_loop'),
                        (dict(update_using_external_algorithm='ctf'), 'CGOptimizer with update_using_external_algorithm'),
                        (dict(optimize_probe=True, optimizer_probe=A.CGOptimizer('probe')), 'CGOptimizer as optimizer_probe')):
        for form in (dict(optimizer=mk()), dict(optimizer='cg', device_cg=True)):
            if 'optimizer_probe' in extra:
                form = dict(optimizer='adam') if form['optimizer'] == 'cg' else form
            with pytest.raises(NotImplementedError) as e:
                drive(g, prj3d, 'a', tmp_path, n_epochs=1, **dict(extra, **form))
            assert what in str(e.value), (what, str(e.value))

    class TwoRanks(object):             # refused before anything is built: nothing of the communicator is touched
        size, rank = 2, 0
    with pytest.raises(NotImplementedError) as e:
        drive(g, prj3d, 'a', tmp_path, n_epochs=1, optimizer=mk(), comm=TwoRanks())
    assert 'CGOptimizer with more than one rank' in str(e.value) and 'user-defined object optimizers with more than one rank' in str(e.value)
