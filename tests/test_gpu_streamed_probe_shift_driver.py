"""reconstruct_ptychography with sub-pixel probe positions on the streamed path (``streamed_probe_shift=True``): a 136 x 136
probe, which 'auto' gives to the streamed plan, at fractional positions, with and without position refinement, against
O.reconstruct_2d in fp64 with its own fp32 run as the yardstick (pytest -m gpu)."""
import numpy as np
import pytest

from oracle import adorym_oracle as O      # checker only
import cases

pytestmark = pytest.mark.gpu

N, P, M = 160, 136, 2
ENERGY_EV, PSIZE_CM = 8000., 1e-6


@pytest.fixture(scope='module')
def A():
    import adorym_amd
    return adorym_amd


def _probes(r):
    yy, xx = np.meshgrid(np.arange(P) - P / 2, np.arange(P) - P / 2, indexing='ij')
    env = np.exp(-(yy ** 2 + xx ** 2) / (2 * (P / 5) ** 2))
    return np.stack([(0.6 ** m) * env * np.exp(1j * (0.3 * m + 0.5 * r.uniform(-1, 1, (P, P)))) for m in range(M)])


@pytest.fixture(scope='module')
def setup():
    """9 positions at fractional nominal positions (offsets within +-0.3 px of a 3 x 3 grid); intensity data of a smooth truth
    object generated at other, true positions (the nominal ones moved by up to 0.4 px)."""
    r = cases.rng(3100)
    grid = np.array([(y, x) for y in (2, 10, 18) for x in (2, 11, 20)], dtype=float)
    nominal = grid + r.uniform(-0.3, 0.3, grid.shape)
    nominal[0] = grid[0] + (0.25, -0.2)                       # (both signs for certain)
    true = nominal + r.uniform(-0.4, 0.4, grid.shape)
    truth = np.stack([2e-3 * cases.smooth_field((N, N, 1), 3101), 2e-4 * cases.smooth_field((N, N, 1), 3102)], -1)
    probes = _probes(r)
    phys = O.Physics((P, P), ENERGY_EV, PSIZE_CM)
    t_int = np.round(true).astype(int)
    tiles, _ = O.extract_tiles(truth, t_int, (P, P))
    mags = [O.predict(tiles[b:b + 1], O.fourier_shift(probes, true[b] - t_int[b], 'float64'), phys, 'float64')[0] for b in range(len(grid))]
    prj = (np.concatenate(mags) ** 2)[None].astype(np.float32)
    guess = [np.full((N, N, 1), 2e-4), np.full((N, N, 1), 2e-5)]
    return dict(nominal=nominal, probes=probes, phys=phys, prj=prj, guess=guess)


BASE = dict(n_epochs=2, minibatch_size=4, learning_rate=1e-5, raw_data_type='intensity', optimize_probe=True, probe_learning_rate=1e-3)
REFINE = dict(BASE, optimize_all_probe_pos=True, all_probe_pos_learning_rate=1e-2)


def drive(A, s, tmp_path, kw, folder='run', **extra):
    probes = s['probes']
    args = dict(fname=s['prj'], obj_size=(N, N, 1), probe_pos=s['nominal'], theta_st=0, theta_end=0, n_theta=1, two_d_mode=True,
                energy_ev=ENERGY_EV, psize_cm=PSIZE_CM, free_prop_cm='inf', n_probe_modes=M, probe_type='supplied',
                probe_initial=[np.abs(probes), np.angle(probes)], initial_guess=s['guess'], gamma=0, alpha_d=0, alpha_b=0, optimizer='adam',
                save_path=str(tmp_path), output_folder=folder, store_checkpoint=False, use_checkpoint=False, return_state=True,
                streamed_probe_shift=True)
    args.update(kw)
    args.update(extra)
    return A.reconstruct_ptychography(**args)


def against_oracle(st, s, kw, pos_floor=1e-4):
    """The bars of test_driver_2d_256_probe_modes_vs_oracle, and the corrections within max(pos_floor px, 3 x fp32) of fp64.
    Every figure is printed before it is held to its bar."""
    runs = {dt: O.reconstruct_2d(s['prj'].astype(np.float64), s['guess'], s['probes'], s['nominal'], s['phys'], dtype=dt, **kw)
            for dt in ('float64', 'float32')}
    o64, o32 = runs['float64'], runs['float32']
    assert len(st['losses']) == len(o64['losses'])
    l64 = np.array(o64['losses'])
    e, e_ref = np.abs(np.array(st['losses']) / l64 - 1).max(), np.abs(np.array(o32['losses']) / l64 - 1).max()
    print('losses %.2e (fp32 oracle %.2e)' % (e, e_ref), st['losses'])
    assert np.allclose(st['losses'], l64, rtol=max(2e-4, 3 * e_ref))
    x = np.stack([st['delta'], st['beta']], -1)
    upd = np.linalg.norm(o64['obj'] - np.stack(s['guess'], -1))
    e, e_ref = np.linalg.norm(x - o64['obj']) / upd, np.linalg.norm(o32['obj'] - o64['obj']) / upd
    print('object update %.2e (fp32 oracle %.2e)' % (e, e_ref))
    assert upd > 0 and e < max(5e-3, 3 * e_ref), (e, e_ref)
    p = st['probe_real'] + 1j * st['probe_imag']
    pn = np.linalg.norm(o64['probes'])
    e, e_ref = np.linalg.norm(p - o64['probes']) / pn, np.linalg.norm(o32['probes'] - o64['probes']) / pn
    print('probes %.2e (fp32 oracle %.2e)' % (e, e_ref))
    assert e < max(1e-4, 3 * e_ref), (e, e_ref)
    c = np.asarray(st['probe_pos_correction'], np.float64).reshape(o64['pos_corr'].shape)
    e, e_ref = np.abs(c - o64['pos_corr']).max(), np.abs(o32['pos_corr'] - o64['pos_corr']).max()
    print('probe_pos_correction %.2e px (fp32 oracle %.2e px)' % (e, e_ref), c.ravel(), o64['pos_corr'].ravel())
    assert e <= max(pos_floor, 3 * e_ref), (e, e_ref)
    return o64


def test_driver_refines_positions_with_a_streamed_probe(A, setup, tmp_path):
    """Adam on the object, on both probe modes and on the positions (optimize_all_probe_pos) over 2 epochs of minibatches of 4:
    losses, object update, probes and probe_pos_correction against the oracle.  The engine must be the streamed one."""
    st = drive(A, setup, tmp_path, REFINE)
    assert st['engine_streamed'] is True and st['engine_probe_shift'] is True
    o64 = against_oracle(st, setup, REFINE)
    start = setup['nominal'] - np.round(setup['nominal'])
    assert np.abs(o64['pos_corr'][0] - (start - start.mean(0))).max() > 5e-3           # (the corrections have moved)
    assert abs(np.asarray(st['probe_pos_correction']).reshape(-1, 2).mean(axis=0)).max() < 1e-6      # re-centred (the drift guard)


def test_driver_static_fractional_positions(A, setup, tmp_path):
    """The same run without refinement: the fractional parts of probe_pos shift the probes and stay as they are."""
    st = drive(A, setup, tmp_path, BASE)
    assert st['engine_streamed'] is True and st['engine_probe_shift'] is True
    against_oracle(st, setup, BASE)
    start = setup['nominal'] - np.round(setup['nominal'])
    assert np.abs(np.asarray(st['probe_pos_correction']).reshape(-1, 2) - start).max() < 1e-6


def test_checkpoint_resume_mid_epoch_gives_the_same_corrections(A, setup, tmp_path):
    """A run stopped after its first epoch and resumed from its last checkpoint (written in front of the epoch's last minibatch)
    ends with the probe_pos_correction of the uninterrupted run, bit for bit.  The checkpoint holds the parameters and the
    object's Adam moments, not the optimiser state of the small parameters (the reference's format), so the positions take
    plain gradient descent with a constant step here and the probe stays fixed; optimizer_batch_number_increment='batch': with
    the default the step counter of a run resumed inside an epoch restarts at the minibatch index (the reference's rule), which
    in two_d_mode is not where the uninterrupted run's counter stands."""
    def kw(folder):
        gd = A.GDOptimizer('probe_pos_correction', output_folder=str(tmp_path / folder), options_dict={'step_size': 1e-3, 'dynamic_rate': False})
        return dict(REFINE, optimize_probe=False, optimizer_all_probe_pos=gd, optimizer_batch_number_increment='batch')
    whole = drive(A, setup, tmp_path, kw('whole'), folder='whole')
    assert whole['engine_streamed'] is True and whole['engine_probe_shift'] is True
    start = setup['nominal'] - np.round(setup['nominal'])
    assert np.abs(np.asarray(whole['probe_pos_correction']).reshape(-1, 2) - (start - start.mean(0))).max() > 1e-5     # (they moved)
    common = dict(store_checkpoint=True, n_batch_per_checkpoint=1)
    part = drive(A, setup, tmp_path, dict(kw('part'), n_epochs=1), folder='part', **common)
    assert not np.array_equal(part['probe_pos_correction'], whole['probe_pos_correction'])
    res = drive(A, setup, tmp_path, kw('part'), folder='part', use_checkpoint=True, **common)
    assert len(res['losses']) == 1 + 3                       # the last minibatch of epoch 0, then epoch 1
    print('resumed', np.asarray(res['probe_pos_correction']).ravel(), 'uninterrupted', np.asarray(whole['probe_pos_correction']).ravel())
    assert np.array_equal(res['probe_pos_correction'], whole['probe_pos_correction'])
    assert np.array_equal(res['losses'][-3:], whole['losses'][-3:])


def test_keyword_does_not_lift_the_other_refusals(A, setup, tmp_path):
    """With the keyword, sub-pixel positions together with optimize_prj_pos_offset or sparse multislice are still refused."""
    n = 30
    kw = dict(fname=np.ones((2, 2, 16, 16), np.float32), obj_size=(n, n, 2), probe_pos=np.array([(0., 0.), (4., 6.)]), theta_st=0,
              theta_end=np.pi, n_theta=2, energy_ev=ENERGY_EV, psize_cm=PSIZE_CM, free_prop_cm=2e-4, probe_type='plane',
              initial_guess=[np.zeros((n, n, 2)), np.zeros((n, n, 2))], n_epochs=1, minibatch_size=2, gamma=0, alpha_d=0, alpha_b=0,
              save_path=str(tmp_path), output_folder='ref', store_checkpoint=False, use_checkpoint=False, return_state=True,
              streamed_probe_shift=True)
    with pytest.raises(NotImplementedError, match='optimize_prj_pos_offset with sub-pixel'):
        A.reconstruct_ptychography(**dict(kw, optimize_prj_pos_offset=True, optimize_all_probe_pos=True))
    with pytest.raises(NotImplementedError, match='optimize_prj_pos_offset with sub-pixel'):
        A.reconstruct_ptychography(**dict(kw, optimize_prj_pos_offset=True, probe_pos=np.array([(0., 0.), (4.5, 6.)])))
    with pytest.raises(NotImplementedError, match='sparse multislice'):
        A.reconstruct_ptychography(**dict(kw, slice_pos_cm_ls=[0, 10e-4], optimize_all_probe_pos=True))
    with pytest.raises(NotImplementedError, match='sparse multislice'):
        A.reconstruct_ptychography(**dict(kw, slice_pos_cm_ls=[0, 10e-4], probe_pos=np.array([(0., 0.), (4.5, 6.)])))


def test_without_the_keyword_the_refusal_names_it(A, setup, tmp_path):
    with pytest.raises(NotImplementedError, match='136 x 136') as ei:
        drive(A, setup, tmp_path, REFINE, streamed_probe_shift=False)
    assert 'streamed_probe_shift=True' in str(ei.value)
