"""
Engine features, all through the C ABI on a real MI355X (pytest -m gpu):
  * the device-built rotation-adjoint tables (adm_rotation_csr_build) equal the host builder's, entry for entry;
  * the pinned upload ring (adm_h2d_async) delivers what the blocking path delivers;
  * the overlap-add refuses, BEFORE launching, a batch that covers a pixel with more than 64 tiles -- also on the
    driver's asynchronous path (the overflow flag was only read by the blocking loss());
"""
import os
import numpy as np
import pytest

import cases
from oracle import adorym_oracle as O      # checker only
from tests import ms_matrix as MM

pytestmark = pytest.mark.gpu


def rel(a, b):
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    return np.linalg.norm(a - b) / np.linalg.norm(b)


@pytest.fixture(scope='module')
def A():
    import adorym_amd
    return adorym_amd


@pytest.fixture(scope='module')
def ctx(A):
    c = A.Context(0)
    yield c
    c.close()


@pytest.mark.parametrize('size,theta,pos', [((12, 12, 12), 0.3, [(-3, -2), (5, 4)]), ((9, 40, 24), 3.44159, [(0, 0)]),
                                            ((6, 256, 256), 0.7853982, [(-2, -36), (1, 228)]), ((5, 64, 64), 0.0, [(0, -5)])])
@pytest.mark.regression
def test_device_built_rotation_tables_equal_host_builder(A, ctx, size, theta, pos):
    """ptr / src / lsrc / boxes identical, weights identical bit for bit (same fp32 pipeline on both sides); the object and
    the padded frame are non-square and the positions hang over the edges so that pad_x0 > 0."""
    P = 8
    eng = A.MultisliceEngine(ctx, size, (P, P), np.array(pos), cases.ENERGY_EV, cases.PSIZE_CM, max_batch=len(pos))
    tab = A.RotationTable(ctx, size, np.float32(theta))
    dev = [a.get() for a in tab.csr(eng.plan)]
    ptr, src, lsrc, w, boxes = tab.csr_host(eng.plan)
    nnz = int(ptr[-1])
    assert np.array_equal(dev[0], ptr)
    assert np.array_equal(dev[1][:nnz], src)
    assert np.array_equal(dev[4].reshape(boxes.shape), boxes)
    assert np.array_equal(dev[2][:nnz], lsrc)
    assert np.array_equal(dev[3][:nnz].view(np.uint32), w.view(np.uint32))
    # and the adjoint evaluated with them equals the atomic scatter of the same operator
    r = cases.rng(5)
    eng.grad_rot.set(r.standard_normal(eng.plan.rot_shape).astype(np.float32))
    g1, g2 = ctx.zeros((*size, 2)), ctx.zeros((*size, 2))
    eng.rotate_adjoint(g1, tab)
    eng.rotate_adjoint(g2, tab.coords)
    assert np.abs(g1.get() - g2.get()).max() <= 5e-6 * np.abs(g2.get()).max()


@pytest.mark.regression
def test_upload_ring_matches_blocking_upload(A, ctx):
    r = cases.rng(11)
    dev = A.DeviceArray(ctx, (7, 33), np.float32)
    ring = A.UploadRing(ctx, 7 * 33 * 4, n_slots=2)
    for i in range(5):                       # more uploads than slots: slots are recycled behind their events
        h = r.standard_normal((7, 33)).astype(np.float32)
        ring.upload(dev, h)
        assert np.array_equal(dev.get(), h)
    small = A.DeviceArray(ctx, (4, 2), np.int32)
    ring.upload(small, np.arange(8, dtype=np.int32).reshape(4, 2))
    assert np.array_equal(small.get().ravel(), np.arange(8))
    big = A.DeviceArray(ctx, (3000,), np.float32)         # larger than a slot: falls back to the blocking copy
    hb = r.standard_normal(3000).astype(np.float32)
    ring.upload(big, hb)
    assert np.array_equal(big.get(), hb)


def test_overlap_add_of_more_than_64_tiles_per_pixel_vs_oracle(A, ctx):
    """A pixel covered by more tiles than the overlap-add's lists hold (64): the batch is added in passes of 64 positions
    (adm_tile_grad_accumulate_range).  70 duplicates of one position + a dense 5-pixel raster of 169 positions under a 16 x 16
    probe (coverage up to 9+70), against the fp64 oracle's gradient; the early cover build is skipped, the loss is unaffected."""
    Y, X, S, P = 80, 80, 2, 16
    pos = np.array([(3, 4)] * 70 + [(y, x) for y in range(0, 65, 5) for x in range(0, 65, 5)])
    B = len(pos)
    eng = A.MultisliceEngine(ctx, (Y, X, S), (P, P), pos, cases.ENERGY_EV, cases.PSIZE_CM, max_batch=B)
    assert eng._check_cover(np.ascontiguousarray(pos.astype(np.int32))) > eng.MAX_COVER
    r = cases.rng(2)
    obj_h = np.stack([r.uniform(0, 1e-3, (Y, X, S)), r.uniform(0, 1e-4, (Y, X, S))], -1)
    obj = ctx.array(obj_h.astype(np.float32))
    probe_h = r.standard_normal((P, P)) + 1j * r.standard_normal((P, P))
    probe = ctx.array(np.stack([probe_h.real, probe_h.imag], -1)[None].astype(np.float32))
    meas = (np.abs(r.standard_normal((B, P, P))) * 5).astype(np.float32)
    g = ctx.zeros(obj.shape)
    eng.set_batch(pos, meas)
    eng.rotate(obj, None)
    eng.build_cover()                                    # (a no-op for such a batch)
    eng.multislice(probe)
    eng.rotate_adjoint(g, None)
    loss = eng.loss()
    phys = O.Physics((P, P), cases.ENERGY_EV, cases.PSIZE_CM)
    lo, _, go, _ = O.forward_adjoint_object(obj_h, None, probe_h, pos, meas.astype(np.float64), phys)
    assert abs(loss - lo) < 1e-5 * abs(lo)
    assert np.linalg.norm(g.get() - go) < 1e-4 * np.linalg.norm(go)
    # ... and the same batch through the path for batches larger than the chip (B = 239 <= 256 here; forced with N_CU = 128)
    eng.N_CU = 128
    try:
        g2 = ctx.zeros(obj.shape)
        eng.set_batch(pos, meas)
        eng.rotate(obj, None)
        eng.multislice_overlapped(probe)
        eng.rotate_adjoint(g2, None)
        assert np.array_equal(g2.get(), g.get())
    finally:
        del eng.N_CU


def test_driver_runs_an_overcovered_fused_angle(A, ctx, tmp_path):
    """The same through reconstruct_ptychography's asynchronous path ('per angle' fuses 80 positions, 72 of them on one spot):
    runs, finite loss (it raised before the multi-pass overlap-add existed)."""
    n_pos, P, N = 80, 16, 32
    pos = np.array([(4, 4)] * 72 + [(i, 2 * i) for i in range(8)])
    r = cases.rng(3)
    prj = (np.abs(r.standard_normal((1, n_pos, P, P))) + 1).astype(np.float32)
    fn = os.path.join(str(tmp_path), 'd.npz')
    np.savez(fn, data=prj)
    st = A.reconstruct_ptychography(fname=fn, save_path=str(tmp_path), output_folder='o', obj_size=(N, N, 4), probe_pos=pos,
                                    theta_st=0, theta_end=0, n_theta=1, energy_ev=cases.ENERGY_EV, psize_cm=cases.PSIZE_CM,
                                    minibatch_size=8, n_epochs=1, update_scheme='per angle', free_prop_cm='inf',
                                    probe_type='gaussian', probe_mag_sigma=4, probe_phase_sigma=4, probe_phase_max=0.5,
                                    initial_guess=[np.full((N, N, 4), 1e-4), np.full((N, N, 4), 1e-5)], gamma=0, alpha_d=None,
                                    random_theta=False, store_checkpoint=False, use_checkpoint=False, cpu_only=False, return_state=True)
    assert len(st['losses']) >= 1 and np.all(np.isfinite(st['losses'])) and np.all(np.isfinite(st['delta']))


@pytest.mark.regression
def test_rccl_restricted_exchange_world1_equals_local_bitwise(A, ctx, rccl_world1):
    """The footprint-restricted exchange through RCCL itself (grouped ncclReduce onto the owner, adm_reduce) at world size 1:
    the gradient buffer holds the data term on the touched range only and NaN elsewhere, the owner's `reg_shard` callback writes
    the (here zero) regulariser term outside the range -- the result equals, bit for bit, the local update with a gradient that
    is zero outside the range."""
    from adorym_amd import comm as C
    from adorym_amd.dp import DataParallelObject, HipOps
    shape = (5, 6, 7, 2)
    r = cases.rng(19)
    n = int(np.prod(shape))
    x0 = (r.standard_normal(n) * 1e-3).astype(np.float32)
    grads = [r.standard_normal(n).astype(np.float32) for _ in range(3)]
    t_lo, t_hi = 84, 336                    # planes 1..3 of 5
    rc = rccl_world1.attach(ctx)
    try:
        out = []
        for comm in (C.LocalComm(), rc):
            st = DataParallelObject(HipOps(ctx), comm, shape)
            st.obj.view(0, (n,)).set(x0)
            for it in range(3):
                g = grads[it].copy()
                if comm is rc:
                    g[:t_lo] = np.nan
                    g[t_hi:] = np.nan

                    def reg_shard(lo, hi, alo, ahi):
                        assert (lo, alo, ahi) == (0, t_lo, t_hi) and hi >= n
                        st.grad.view(0, (alo,)).zero_()
                        st.grad.view(ahi, (n - ahi,)).zero_()
                    st.grad.view(0, (n,)).set(g)
                    st.exchange_and_update('adam', it, {'step_size': 1e-4}, flags=1, touched=(t_lo, t_hi), reg_shard=reg_shard)
                else:
                    g[:t_lo] = 0
                    g[t_hi:] = 0
                    st.grad.view(0, (n,)).set(g)
                    st.exchange_and_update('adam', it, {'step_size': 1e-4}, flags=1)
            st.finish_update()
            out.append((st.obj.view(0, (n,)).get(), st.moments[0].get(), st.moments[1].get()))
        for a, b in zip(out[0], out[1]):
            assert np.all(np.isfinite(b[:n])) and np.array_equal(a[:n], b[:n])
    finally:
        ctx.sync()
        ctx.lib.adm_comm_destroy(ctx.handle)
        rc.ctx = None


@pytest.mark.regression
def test_rccl_comm_world1_equals_local_bitwise(A, ctx, rccl_world1):
    """The multi-GPU code path (adm_comm_init, in-place adm_reduce_scatter / adm_all_gather through RCCL, sharded update) at
    world size 1 gives bit for bit what the single-GPU path gives after 3 Adam steps and a GD step; the small-gradient
    all-reduce leaves a 1-rank buffer unchanged."""
    from adorym_amd import comm as C
    from adorym_amd.dp import DataParallelObject, HipOps
    shape = (5, 6, 7, 2)
    r = cases.rng(9)
    n = int(np.prod(shape))
    x0 = (r.standard_normal(n) * 1e-3).astype(np.float32)
    grads = [r.standard_normal(n).astype(np.float32) for _ in range(4)]
    rc = rccl_world1.attach(ctx)
    try:
        assert (rc.rank, rc.size) == (0, 1) and ctx.lib.adm_comm_size(ctx.handle) == 1
        out = []
        for comm in (C.LocalComm(), rc):
            st = DataParallelObject(HipOps(ctx), comm, shape)
            assert st.inplace == (comm is rc)
            st.obj.view(0, (n,)).set(x0)
            for it in range(3):
                st.zero_grad()
                st.grad.view(0, (n,)).set(grads[it])
                st.exchange_and_update('adam', it, {'step_size': 1e-4}, flags=1)
            st.zero_grad()
            st.grad.view(0, (n,)).set(grads[3])
            # first=: (RCCL) the named planes are broadcast from their owner now (adm_broadcast), the full all-gather is
            # deferred to finish_update(), which the driver queues on the side stream beside the next kernel
            st.exchange_and_update('gd', 0, {'step_size': 1e-5}, first=(84, 252))
            if comm is rc:
                assert st.overlap_gather and st._gather_pending
            ctx.fork()
            st.finish_update()
            ctx.end_fork()
            ctx.join()
            assert not st._gather_pending
            out.append((st.obj.view(0, (n,)).get(), st.moments[0].get(), st.moments[1].get()))
        for a, b in zip(out[0], out[1]):
            assert np.array_equal(a[:n], b[:n])
        small = ctx.array(grads[0][:100])
        rc.all_reduce_device(small)
        assert np.array_equal(small.get(), grads[0][:100])
        assert rc.max_over_ranks(3.5) == 3.5 and rc.bcast_object({'a': 1}) == {'a': 1}
        rc.barrier()
    finally:
        ctx.sync()
        ctx.lib.adm_comm_destroy(ctx.handle)        # this context's communicator; the session's process group stays up
        rc.ctx = None


@pytest.mark.regression
def test_probe_gradient_is_bitwise_reproducible(A, ctx):
    """the probe gradient was accumulated with float atomics.  Every position now stores its own slot and the
    slots are summed in a fixed order: two launches on the same inputs agree bit for bit, and the sum over a batch equals
    the sum of its two halves launched separately (+=) to fp32 rounding."""
    r = cases.rng(21)
    P, Y, X, S, B = 72, 100, 110, 6, 40
    pos = np.stack([r.integers(-8, Y - 60, B), r.integers(-8, X - 60, B)], 1)
    eng = A.MultisliceEngine(ctx, (Y, X, S), (P, P), pos, cases.ENERGY_EV, cases.PSIZE_CM, max_batch=B)
    obj = ctx.array(np.stack([r.uniform(0, 2e-3, (Y, X, S)), r.uniform(0, 2e-4, (Y, X, S))], -1).astype(np.float32))
    probe = ctx.array(r.standard_normal((1, P, P, 2)).astype(np.float32))
    meas = (np.abs(r.standard_normal((B, P, P))) * 20).astype(np.float32)
    eng.rotate(obj, None)
    outs = []
    for rep in range(2):
        eng.set_batch(pos, meas)
        gp = ctx.zeros(probe.shape)
        eng.multislice(probe, grad_probe=gp)
        outs.append(gp.get())
    assert np.array_equal(outs[0].view(np.uint32), outs[1].view(np.uint32))
    assert np.abs(outs[0]).max() > 0
    gp = ctx.zeros(probe.shape)
    for half in (slice(0, B // 2), slice(B // 2, B)):
        eng.set_batch(pos[half], meas[half])
        eng.multislice(probe, grad_probe=gp, grad_scale=2.0 / (B * P * P))
    assert np.abs(gp.get() - outs[0]).max() <= 2e-6 * np.abs(outs[0]).max()


def _generic_case(A, ctx, Py, Px, S=5, B=3, free_prop='inf', binning=1, n_modes=1, unknown_type='delta_beta', generic=False, seed=0):
    """Forward + gradients of one minibatch against the fp64 oracle (and its fp32 run for the 3x rule)."""
    MM.check(MM.run_case(A, ctx, (Py, Px), S=S, B=B, free_prop=free_prop, binning=binning, n_modes=n_modes, unknown_type=unknown_type,
                         generic=generic, margin=(9, 11), seed=seed), MM.GENERIC)


@pytest.mark.parametrize('Py,Px', [(48, 48), (96, 96), (128, 128), (100, 100), (40, 56), (26, 35), (13, 22), (72, 64)])
def test_any_probe_size_vs_oracle(A, ctx, Py, Px):
    """probe sizes outside the compiled set and non-square probes raised; the reference takes whatever
    prj.shape[-2:] is (adorym/ptychography.py:313-317).  adm_ms_generic.hip: 128 x 128 (SURVEY's config-1 shape), 48, 96,
    100 (factor 5), non-square, odd primes 13 / 7 x 5, and a mixed 72 x 64."""
    _generic_case(A, ctx, Py, Px)


@pytest.mark.parametrize('kw', [dict(free_prop=0), dict(free_prop=1e-4), dict(binning=2, S=5), dict(n_modes=3), dict(unknown_type='real_imag'),
                                dict(n_modes=2, free_prop=0)])
def test_generic_kernel_variants_vs_oracle(A, ctx, kw):
    _generic_case(A, ctx, 20, 28, **kw)


@pytest.mark.regression
def test_generic_kernel_equals_tuned_kernel_at_72(A, ctx):
    """The same minibatch through the tuned kernel and through the generic one (forced): both within the oracle bar, and
    within 1e-4 of each other on the gradient."""
    _generic_case(A, ctx, 72, 72, generic=False, seed=5)
    _generic_case(A, ctx, 72, 72, generic=True, seed=5)


def test_driver_runs_with_a_non_square_unlisted_probe(A, ctx, tmp_path):
    """reconstruct_ptychography end to end with a 20 x 28 probe (no tuned kernel): loss decreases, outputs written."""
    r = cases.rng(8)
    N, S, Py, Px = 40, 6, 20, 28
    pos = np.array([(y, x) for y in (0, 8, 16) for x in (0, 6, 12)])
    truth = np.stack([2e-3 * cases.smooth_field((N, N, S), 1), 2e-4 * cases.smooth_field((N, N, S), 2)], -1)
    phys = O.Physics((Py, Px), 5000., 1e-7, free_prop_cm='inf')
    pm, pp = A.util.initialize_probe((Py, Px), 'gaussian', probe_mag_sigma=5, probe_phase_sigma=5, probe_phase_max=0.5)
    probe = np.squeeze(pm) + 1j * np.squeeze(pp)
    tt, _ = O.extract_tiles(truth, pos, (Py, Px))
    prj = O.predict(tt, probe, phys, 'float64')[0][None].astype(np.float32)
    st = A.reconstruct_ptychography(fname=prj, obj_size=(N, N, S), probe_pos=pos, theta_st=0, theta_end=0, n_theta=1, energy_ev=5000.,
                                    psize_cm=1e-7, free_prop_cm='inf', minibatch_size=3, n_epochs=3, learning_rate=2e-5, optimizer='adam',
                                    initial_guess=[0.5 * truth[..., 0], 0.5 * truth[..., 1]], probe_type='gaussian', probe_mag_sigma=5,
                                    probe_phase_sigma=5, probe_phase_max=0.5, gamma=0, alpha_d=None, save_path=str(tmp_path),
                                    output_folder='o', store_checkpoint=False, use_checkpoint=False, return_state=True)
    l = np.array(st['losses'])
    assert np.all(np.isfinite(l)) and l[-3:].mean() < 0.85 * l[:3].mean()
    assert os.path.exists(os.path.join(st['output_folder'], 'delta_ds_1.tiff'))


def test_c2_sixteen_virtual_ranks_sum_vs_oracle(A, ctx):
    """BASELINE's config 2 says 'minibatch 16', but the reference forces minibatch_size = 1 for undivided full-field data
    (adorym/ptychography.py:342-346): 16 in flight = 16 ranks x 1 angle each, gradients SUMMED (:1113-1114), every rank
    adding the L1 term (forward_model.py:138-139), one Adam step.  The same global batch on one GPU: 16 angles accumulated
    into one gradient buffer, one exchange_and_update -- against the fp64 oracle's sum and Adam step."""
    from adorym_amd.dp import DataParallelObject, HipOps
    from adorym_amd.comm import LocalComm
    N, R = 64, 16
    truth = np.stack([2e-5 * cases.smooth_field((N, N, N), 171), 2e-7 * cases.smooth_field((N, N, N), 172)], -1)
    guess = np.stack([1.2e-5 * cases.smooth_field((N, N, N), 173), 1.2e-7 * cases.smooth_field((N, N, N), 174)], -1)
    thetas = np.linspace(0, 2 * np.pi, 50, dtype='float32')[3:3 + R]
    phys = O.Physics((N, N), 800., 0.67e-7, free_prop_cm=0)
    probe = np.ones((N, N), complex)
    pos = np.array([(0, 0)])
    a_d, a_b = 1e-9 * 64 ** 3, 1e-10 * 64 ** 3
    g64 = np.zeros_like(guess)
    g32 = np.zeros(guess.shape, np.float32)
    losses64, data = [], []
    for th in thetas:
        c = O.rotation_coords((N, N, N), th)
        meas = np.abs(O.multislice_forward(O.rotate_fwd(truth, c, 'float64')[None], probe, phys, 'float64'))
        data.append(meas.astype(np.float32))
        l, _, g, _ = O.forward_adjoint_object(guess, c, probe, pos, meas.astype(np.float32).astype(np.float64), phys, 'float64')
        g64 += g + O.l1_value_grad(guess, a_d, a_b)[1]
        losses64.append(l)
        g32 += O.forward_adjoint_object(guess.astype(np.float32), c, probe, pos, meas.astype(np.float32), phys, 'float32')[2] \
            + O.l1_value_grad(guess.astype(np.float32), a_d, a_b)[1].astype(np.float32)
    x64, _, _ = O.adam_step(guess, g64, np.zeros_like(guess), np.zeros_like(guess), 0, 1e-7)
    # ---- GPU ----
    eng = A.MultisliceEngine(ctx, (N, N, N), (N, N), pos, 800., 0.67e-7, free_prop_cm=0, max_batch=1)
    st = DataParallelObject(HipOps(ctx), LocalComm(), (N, N, N, 2))
    n = guess.size
    st.obj.view(0, (n,)).set(guess.astype(np.float32).ravel())
    obj = st.obj.view(0, (N, N, N, 2))
    grad = st.grad.view(0, (N, N, N, 2))
    st.zero_grad()
    d_probe = ctx.array(c2(probe)[None])
    from adorym_amd._lib import check
    losses = []
    for th, meas in zip(thetas, data):
        tab = A.RotationTable(ctx, (N, N, N), th)
        losses.append(eng.loss_and_grad(obj, grad, tab, d_probe, pos, meas))
        check(ctx.lib.adm_reg_grad(eng.plan.handle, obj.ptr, a_d, a_b, 0.0, grad.ptr, None))       # every virtual rank adds it
    g = grad.get()
    st.exchange_and_update('adam', 0, {'step_size': 1e-7})
    x = st.obj.view(0, (N, N, N, 2)).get()
    assert np.allclose(losses, losses64, rtol=2e-5)
    # weak object (delta ~ 1e-5), near field: the data gradient is a small difference of O(1) magnitudes, so fp32 -- the
    # reference's own included -- sits at the per-cent level against fp64: 3x rule against the fp32 oracle
    e, e32 = rel(g, g64), rel(g32, g64)
    assert e <= 3 * e32 + 1e-5, (e, e32)
    d = np.abs(x - x64)
    assert np.sqrt(np.mean(d ** 2)) < 1e-8 and (d > 3e-8).mean() < 2e-3       # Adam's first step is lr * sign-like: lr = 1e-7
    # ---- the same 16 angles in ONE launch (adorym_amd.AngleBatch: 16 workgroups, the object rotated block by block into a
    # stacked frame): the same losses and the same summed gradient ----
    ab = A.AngleBatch(ctx, (N, N, N), (N, N), R, 800., 0.67e-7, free_prop_cm=0)
    obj2 = ctx.array(guess.astype(np.float32))
    grad2 = ctx.zeros((N, N, N, 2))
    tabs = [A.RotationTable(ctx, (N, N, N), th) for th in thetas]
    losses2 = ab.loss_and_grad(obj2, grad2, tabs, d_probe, np.concatenate(data).reshape(R, N, N))
    for _ in range(R):
        check(ctx.lib.adm_reg_grad(eng.plan.handle, obj2.ptr, a_d, a_b, 0.0, grad2.ptr, None))
    g2 = grad2.get()
    assert np.allclose(losses2, losses64, rtol=2e-5)
    assert rel(g2, g64) <= 3 * e32 + 1e-5
    assert rel(g2, g) < 2e-6, rel(g2, g)          # (order of the fp32 additions per voxel differs: data terms first, L1 terms last)


@pytest.mark.parametrize('N,R', [(64, 16), (48, 5)])
@pytest.mark.regression
def test_angle_batch_stacked_rotations_equal_per_angle_launches_bitwise(A, ctx, N, R):
    """adm_rotate_fwd_stack / adm_rotate_adj_staged_stack (one launch for the R angles of an AngleBatch) against R calls of
    adm_rotate_fwd / adm_rotate_adj_staged on the same stacked engine: the stacked rotated object, the losses and the summed
    gradient agree bit for bit (the stacked adjoint adds the angles' contributions r ascending, as the sequence of launches
    does).  N = 48: patches and plane groups with tails."""
    r = cases.rng(1000 + N)
    guess = np.stack([1e-5 * r.uniform(0.5, 1.5, (N, N, N)), 1e-7 * r.uniform(0.5, 1.5, (N, N, N))], -1).astype(np.float32)
    thetas = np.linspace(0.1, 2 * np.pi, R, dtype='float32')
    data = (1 + 0.05 * np.abs(r.standard_normal((R, N, N)))).astype(np.float32)
    probe = ctx.array(c2(np.ones((N, N), complex))[None])
    ab = A.AngleBatch(ctx, (N, N, N), (N, N), R, 800., 0.67e-7, free_prop_cm=0)
    eng = ab.engine
    tabs = [A.RotationTable(ctx, (N, N, N), th) for th in thetas]
    obj = ctx.array(guess)
    # one launch each
    g1 = ctx.zeros((N, N, N, 2))
    l1 = ab.loss_and_grad(obj, g1, tabs, probe, data)
    rot1 = eng.obj_rot.get()
    # R launches each, same engine
    g2 = ctx.zeros((N, N, N, 2))
    eng.set_batch(ab.pos, data)
    for k, t in enumerate(tabs):
        eng.rotate(ab._shifted(obj, k), t, (k * N, (k + 1) * N))
    rot2 = eng.obj_rot.get()
    eng.multislice(probe, grad_scale=2.0 / eng.n_det)
    for k, t in enumerate(tabs):
        eng.rotate_adjoint(ab._shifted(g2, k), t, (k * N, (k + 1) * N))
    l2 = eng.loss_sums(R) / eng.n_det
    assert np.array_equal(rot1, rot2)
    assert np.array_equal(l1, l2)
    a, b = g1.get(), g2.get()
    assert np.abs(a).max() > 0 and np.array_equal(a, b)
    # ... and the one-launch form without scratch (every block walks the angles one after the other)
    assert ab._adj_scratch is not False
    ab._adj_scratch = False
    g3 = ctx.zeros((N, N, N, 2))
    ab.loss_and_grad(obj, g3, tabs, probe, data)
    assert np.array_equal(g3.get(), b)


def c2(z):
    return np.stack([z.real, z.imag], -1).astype(np.float32)


@pytest.mark.parametrize('P,n_modes,theta,sign,generic', [(72, 1, 0.6, 1, False), (64, 2, None, 1, False), (36, 1, 2.1, -1, False),
                                                          (72, 1, None, 1, False), (72, 1, 0.6, 1, True), (20, 2, 1.3, 1, True)])
@pytest.mark.regression
def test_transmission_cache_is_bit_identical(A, ctx, P, n_modes, theta, sign, generic):
    """adm_plan_set_transmission_cache: exp(-k1 beta)(cos, sin)(-sigma k1 delta) stored per rotated-frame voxel by
    adm_rotate_fwd and loaded by the slice loop gives the SAME bits as evaluating it per position inside the loop (the
    same fp32 expression, once per voxel): loss, prediction, object gradient, probe gradient.  Phases beyond pi/4 are
    included so that both sincos paths of the in-loop modulator are compared.  Partial y ranges are rotated the way the
    driver does it (footprint of the batch only), after a full rotation of ANOTHER object, so stale rows would show.
    generic: the any-size kernel (adm_ms_generic.hip) reads the cache too."""
    r = cases.rng(77 + P + n_modes)
    Y, X, S, B = P + 30, P + 41, 7, 9
    pos = np.stack([r.integers(-6, Y - P + 6, B), r.integers(-6, X - P + 6, B)], 1)
    k1 = 2 * np.pi * 1.0 / (1240. / cases.ENERGY_EV)
    delta = r.uniform(0, 2.5 / k1, (Y, X, S))            # phases up to 2.5 rad: beyond the small-angle path
    delta[:, : X // 2] *= 0.01                            # ... and a half that stays inside it
    obj = np.stack([delta, r.uniform(0, 0.3 / k1, (Y, X, S))], -1).astype(np.float32)
    other = np.stack([r.uniform(0, 1e-3, (Y, X, S)), r.uniform(0, 1e-4, (Y, X, S))], -1).astype(np.float32)
    probe = r.standard_normal((n_modes, P, P, 2)).astype(np.float32)
    meas = (np.abs(r.standard_normal((B, P, P))) * 10).astype(np.float32)
    outs = []
    for cache in (False, True):
        eng = A.MultisliceEngine(ctx, (Y, X, S), (P, P), pos, cases.ENERGY_EV, cases.PSIZE_CM, max_batch=B, n_probe_modes=n_modes,
                                 sign_convention=sign, transmission_cache=cache, generic=generic)
        assert eng.transmission_cache == cache
        tab = A.RotationTable(ctx, (Y, X, S), np.float32(theta)) if theta is not None else None
        coords = tab.coords if tab is not None else None
        eng.rotate(ctx.array(other), coords)                               # every row holds something else first
        eng.set_batch(pos, meas)
        lo, hi = eng.y_footprint(pos)
        eng.rotate(ctx.array(obj), coords, y_range=(lo, hi))
        gp = ctx.zeros(probe.shape)
        eng.multislice(ctx.array(probe), grad_probe=gp, want_pred=True)
        g = ctx.zeros(obj.shape)
        eng.rotate_adjoint(g, tab, y_range=(lo, hi))          # the table: deterministic gather (bare coords = float atomics)
        outs.append((eng._loss.view(0, (B,)).get(), eng.pred(), eng.grad_rot.get(), g.get(), gp.get()))
    for a, b in zip(*outs):
        assert np.isfinite(a).all() and np.abs(a).max() > 0
        assert np.array_equal(a.view(np.uint32), b.view(np.uint32))


@pytest.mark.regression
def test_transmission_cache_tracks_its_source_buffer(A, ctx):
    """The cache is used only for the obj_rot buffer adm_rotate_fwd last filled it from: a launch on ANOTHER rotated-frame
    buffer silently takes the in-loop path (right answer), and adm_transmission_refresh adopts a buffer written by other
    means.  Also: binning > 1 and real_imag plans refuse the cache."""
    from adorym_amd import _lib
    r = cases.rng(5)
    P, Y, X, S, B = 16, 30, 34, 4, 3
    pos = np.stack([r.integers(0, Y - P, B), r.integers(0, X - P, B)], 1)
    obj = np.stack([r.uniform(0, 2e-3, (Y, X, S)), r.uniform(0, 2e-4, (Y, X, S))], -1).astype(np.float32)
    obj2 = (obj * 3).astype(np.float32)
    probe = ctx.array(r.standard_normal((1, P, P, 2)).astype(np.float32))
    meas = (np.abs(r.standard_normal((B, P, P))) * 4).astype(np.float32)

    def run(eng, rot_buf):
        eng.set_batch(pos, meas)
        lib = ctx.lib
        assert lib.adm_multislice_fwd_adj(eng.plan.handle, rot_buf.ptr, probe.ptr, eng._cur_pos.ptr, B, eng._cur_target.ptr, 1, None,
                                          None, eng._loss.ptr, 1.0, eng._ws.ptr, eng._ws.nbytes) == _lib.ADM_OK
        return eng._loss.view(0, (B,)).get()

    ref = A.MultisliceEngine(ctx, (Y, X, S), (P, P), pos, cases.ENERGY_EV, cases.PSIZE_CM, max_batch=B, transmission_cache=False)
    ref.rotate(ctx.array(obj2), None)
    want2 = run(ref, ref.obj_rot)
    eng = A.MultisliceEngine(ctx, (Y, X, S), (P, P), pos, cases.ENERGY_EV, cases.PSIZE_CM, max_batch=B)
    eng.rotate(ctx.array(obj), None)                      # cache <- obj
    other = ctx.zeros(eng.plan.rot_shape)
    other.set(ref.obj_rot.get())                          # a second rotated-frame buffer holding obj2, written by a plain copy
    assert np.array_equal(run(eng, other), want2)         # not the cached buffer: in-loop path, obj2's answer
    assert ctx.lib.adm_transmission_refresh(eng.plan.handle, other.ptr, 0, Y) == _lib.ADM_OK
    assert np.array_equal(run(eng, other), want2)         # adopted: cached path, same bits
    assert ctx.lib.adm_transmission_refresh(eng.plan.handle, other.ptr, 3, 2) == _lib.ADM_ERR_INVALID
    for kw in (dict(binning=2), dict(unknown_type='real_imag')):
        e2 = A.MultisliceEngine(ctx, (Y, X, S), (P, P), pos, cases.ENERGY_EV, cases.PSIZE_CM, max_batch=B, **kw)
        assert not e2.transmission_cache
        assert ctx.lib.adm_plan_set_transmission_cache(e2.plan.handle, 1) == _lib.ADM_ERR_UNSUPPORTED
    assert ctx.lib.adm_transmission_refresh(ref.plan.handle, other.ptr, 0, Y) == _lib.ADM_ERR_INVALID     # no cache on that plan


@pytest.mark.regression
def test_probe_gradient_through_shifts_of_a_large_batch_is_bit_reproducible(A, ctx):
    """More than 256 (position, mode) pairs: adm_probe_shift_adj sums the positions' probe-gradient terms from per-position slots in a
    fixed order (two levels) instead of float atomics on the one probe gradient -- the same bits run after run, and the sum equals
    the sum over two halves of the batch launched separately (which take the same path) to rounding."""
    r = cases.rng(77)
    Y, X, P, B = 48, 48, 16, 300
    pos = np.stack([r.integers(-4, Y - 10, B), r.integers(-4, X - 10, B)], 1)
    eng = A.MultisliceEngine(ctx, (Y, X, 1), (P, P), pos, cases.ENERGY_EV, cases.PSIZE_CM, max_batch=B, n_probe_modes=2)
    obj = ctx.array(np.stack([r.uniform(0, 1e-3, (Y, X, 1)), r.uniform(0, 1e-4, (Y, X, 1))], -1).astype(np.float32))
    probe = ctx.array(r.standard_normal((2, P, P, 2)).astype(np.float32))
    shifts = ctx.array(r.uniform(-0.5, 0.5, (B, 2)).astype(np.float32))
    meas = (np.abs(r.standard_normal((B, P, P))) * 5).astype(np.float32)
    outs = []
    for _ in range(3):
        eng.set_batch(pos, meas)
        eng.rotate(obj, None)
        gp, gs = ctx.zeros(probe.shape), ctx.zeros((B, 2))
        eng.multislice(probe, grad_probe=gp, shifts=shifts, grad_shifts=gs)
        outs.append((gp.get(), gs.get()))
    assert np.abs(outs[0][0]).max() > 0
    for o in outs[1:]:
        assert np.array_equal(o[0], outs[0][0]) and np.array_equal(o[1], outs[0][1])
    # the same positions as 2 x 150 (each still beyond 256 pairs): same sum up to the order of the additions
    acc = np.zeros_like(outs[0][0])
    for lo in (0, 150):
        eng.set_batch(pos[lo:lo + 150], meas[lo:lo + 150])
        eng.rotate(obj, None)
        gp = ctx.zeros(probe.shape)
        eng.multislice(probe, grad_probe=gp, shifts=ctx.array(shifts.get()[lo:lo + 150]), grad_shifts=ctx.zeros((150, 2)), grad_scale=2.0 / (B * eng.n_det))
        acc += gp.get()
    assert np.abs(acc - outs[0][0]).max() <= 2e-5 * np.abs(acc).max()


@pytest.mark.parametrize('size', [(8, 64, 64), (4, 48, 80), (4, 256, 256), (2, 37, 53)])
def test_device_built_rotation_table_is_the_reference_table_bitwise(A, ctx, size):
    """adm_rotation_table_build (float32, one rounding per operation, round-to-nearest-even to half) against
    adorym_amd.util.rotation_lookup, which golden F4 pins to the reference's table bit for bit: 25 angles, cubic and non-cubic
    cross-sections (the reference subtracts the OTHER axis' centre)."""
    from adorym_amd.util import rotation_lookup
    for th in np.concatenate([np.linspace(0, 2 * np.pi, 21, dtype='float32'), np.float32([0.4, 0.78, -1.3, 3.0])]):
        tab = A.RotationTable(ctx, size, th)
        want = rotation_lookup(size, th)
        got = tab.coords.get().view(np.float16)
        assert np.array_equal(got.view(np.uint16), want.view(np.uint16)), (size, float(th), int((got != want).sum()))
        assert np.array_equal(tab.host, want)
