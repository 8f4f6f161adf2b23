"""Sub-pixel probe positions on the streamed multislice path (adm_plan_set_probe_shift, adm_multislice_fwd_adj_probe_shift;
ps_colfft_kernel, ps_col_kernel<false / true> of adm_ms_probeshift.hip, st_shift_reduce_kernel) through the engine (pytest -m gpu).

The checker is tests/ms_matrix.py's ``oracle_case(P, pp='shifts')``: shifts of up to +-2.5 px, some entries used by several
positions, the oracle in fp64 with its own fp32 run as the yardstick.  The bars are ``MM.GENERIC``; the shift gradient must
also be within max(GENERIC['shift'], 3 x the fp32 oracle's distance) of fp64.  Every figure is printed before it is asserted.
"""
import functools

import numpy as np
import pytest

from tests import ms_matrix as MM

pytestmark = pytest.mark.gpu


@pytest.fixture(scope='module')
def A():
    import adorym_amd
    return adorym_amd


@pytest.fixture(scope='module')
def ctx(A):
    c = A.Context(0)
    yield c
    c.close()


@functools.lru_cache(maxsize=None)
def _case(P, items):
    return MM.oracle_case(P, **dict(items))


def case_of(P, **kw):
    """oracle_case, computed once per set of arguments and shared (run_ps copies the dict and leaves the arrays alone)."""
    return _case(P, tuple(sorted(kw.items())))


def run_ps(A, ctx, case, want_grad=True, want_gs=True, want_gp=True, use_index=True, shifts=None, gs_init=None, gp_init=None,
           canaries=False, **engine_kw):
    """rotate -> multislice(shifts=...) -> rotate_adjoint on an engine built with streamed=True, probe_shift=True.  Without
    ``use_index`` the engine gets one entry per position (the case's entry of that position) and no index; 'gshift' is then
    gathered back per entry of the case on the host in fp64.  ``shifts``: entries instead of the case's.  ``canaries``: shifts,
    grad_shifts and grad_probe are views into larger arrays whose surroundings must come back untouched."""
    out, k = dict(case), case['kw']
    obj, pos, probes, target, bs = [case[n] for n in ('obj', 'pos', 'probes', 'target', 'beamstop')]
    (Py, Px), S, B, M = k['shape'], k['S'], k['B'], k['n_modes']
    Y, X = obj.shape[:2]
    idx = case['idx']
    if shifts is None:
        shifts = case['shifts']
    shifts = np.asarray(shifts, np.float64)
    if not use_index and idx is not None:
        shifts = shifts[idx]
    n = len(shifts)
    eng = A.MultisliceEngine(ctx, (Y, X, S), (Py, Px), pos, MM.ENERGY_EV, MM.PSIZE_CM, free_prop_cm=k['free_prop'], binning=k['binning'],
                             fresnel_approx=k['fresnel_approx'], sign_convention=k['sign_convention'], normalize_fft=k['normalize_fft'],
                             n_probe_modes=M, max_batch=B, loss_function_type=k['loss'], poisson_multiplier=k['poisson_multiplier'],
                             unknown_type=k['unknown_type'], beamstop=bs, transmission_cache=k['transmission_cache'], streamed=True,
                             probe_shift=True, **engine_kw)
    assert eng.streamed is True and eng.probe_shift is True
    pad = 3 if canaries else 0
    host_s = np.full((n + 2 * pad, 2), 1e30, np.float32)       # (a shift read from the surroundings would wreck everything)
    host_s[pad:pad + n] = shifts
    host_g = np.full((n + 2 * pad, 2), -7.25, np.float32)
    host_g[pad:pad + n] = 0 if gs_init is None else gs_init
    gpad = 1 if canaries else 0
    host_gp = np.full((M + 2 * gpad, Py, Px, 2), -7.25, np.float32)
    host_gp[gpad:gpad + M] = 0 if gp_init is None else gp_init
    all_s, all_g, all_gp = ctx.array(host_s), ctx.array(host_g), ctx.array(host_gp)
    d_s, d_gs = all_s.view(2 * pad, (n, 2)), all_g.view(2 * pad, (n, 2))
    d_gp = all_gp.view(gpad * Py * Px * 2, (M, Py, Px, 2))
    d_idx = ctx.array(np.ascontiguousarray(idx, np.int32)) if (use_index and idx is not None) else None
    d_grad = ctx.zeros(obj.shape)
    eng.set_batch(pos, target)
    eng.rotate(ctx.array(obj, np.float32), None)
    eng.multislice(ctx.array(MM.c2(probes)), grad_probe=d_gp if want_gp else None, want_grad=want_grad, want_pred=True, shifts=d_s,
                   shift_index=d_idx, grad_shifts=d_gs if want_gs else None)
    if want_grad:
        eng.rotate_adjoint(d_grad, None)
        out['grad'] = d_grad.get()
    g_all, gp_all = all_g.get(), all_gp.get()
    out['gprobe_raw'] = gp_all[gpad:gpad + M].copy()
    out['gprobe'] = MM.cplx(out['gprobe_raw'])
    out['gs_raw'] = g_all[pad:pad + n].copy()
    gs = out['gs_raw'].astype(np.float64)
    if not use_index and idx is not None:
        per_entry = np.zeros((len(case['shifts']), 2))
        np.add.at(per_entry, idx, gs)
        gs = per_entry
    if case['shifts'] is not None:
        out['gshift'] = gs
    out['pred'] = eng.pred()
    out['loss'] = eng.loss()
    out['n_rounds'] = len(eng.rounds(B))
    out['ws_bytes_4'], out['ws_bytes_2'] = eng.plan.workspace_bytes(4), eng.plan.workspace_bytes(2)
    if canaries:
        assert np.array_equal(all_s.get(), host_s)
        assert np.all(g_all[:pad] == -7.25) and np.all(g_all[pad + n:] == -7.25)
        assert np.all(gp_all[:gpad] == -7.25) and np.all(gp_all[gpad + M:] == -7.25)
    eng.plan.close()
    return out


def shift_bar(res):
    return max(MM.GENERIC['shift'], 3 * MM.rel(res['gshift_32'], res['gshift_o']))


def report_and_check(res, what=''):
    """Print every figure that ``MM.check(res, MM.GENERIC)`` holds to a bar, with the fp32 oracle's beside it, then check."""
    per = max(MM.rel(p, po) for p, po in zip(res['pred'], res['pred_o']))
    print(what, 'pred %.2e, worst position %.2e (fp32 oracle %.2e)' % (MM.rel(res['pred'], res['pred_o']), per,
                                                                       MM.rel(res['pred_32'], res['pred_o'])))
    print(what, 'loss %.2e (fp32 oracle %.2e)' % (abs(res['loss'] / res['loss_o'] - 1), abs(res['loss_32'] / res['loss_o'] - 1)))
    print(what, 'grad %.2e (fp32 oracle %.2e)' % (MM.rel(res['grad'], res['grad_o']), MM.rel(res['grad_32'], res['grad_o'])))
    print(what, 'gprobe %.2e (fp32 oracle %.2e)' % (MM.rel(res['gprobe'], res['gprobe_o']), MM.rel(res['gprobe_32'], res['gprobe_o'])))
    if 'gshift' in res:
        e = MM.rel(res['gshift'], res['gshift_o'])
        print(what, 'dL/ds %.2e (fp32 oracle %.2e, bar %.2e)' % (e, MM.rel(res['gshift_32'], res['gshift_o']), shift_bar(res)),
              np.asarray(res['gshift']).ravel(), np.asarray(res['gshift_o']).ravel())
    assert 'gprobe_b' not in res
    MM.check(res, MM.GENERIC)
    if 'gshift' in res:
        assert np.linalg.norm(res['gshift_o']) > 0
        assert e <= shift_bar(res), ('shift gradient', e, shift_bar(res))


# ---------------------------------------------------------------------------------------------------- 1. launch geometries
GEOMETRY_CASES = {
    'P24x24_row_group_clipped': dict(P=(24, 24)),
    'P135x201_modes': dict(P=(135, 201), n_modes=2),
    'P640x136_320_thread_columns': dict(P=(640, 136)),
    'P130x1536_ragged_row': dict(P=(130, 1536)),
    'P5x2048_one_full_row': dict(P=(5, 2048)),
    'P2048x5_cw4_last_group_of_1': dict(P=(2048, 5)),
    'P1025x132_smallest_cw4': dict(P=(1025, 132)),
}


@pytest.mark.parametrize('name', list(GEOMETRY_CASES))
def test_geometries_vs_oracle(A, ctx, name):
    """ps_colfft_kernel, ps_col_kernel<false>, ps_col_kernel<true>, st_shift_reduce_kernel and the row launches around them at every
    launch geometry (row groups clipped to Py, whole and ragged rows, column groups of 8 and of 4 with a short last group, 256
    to 512 threads) with shifted probes, S = 2, B = 6, far field."""
    kw = dict(GEOMETRY_CASES[name])
    res = run_ps(A, ctx, case_of(kw.pop('P'), S=2, B=6, pp='shifts', **kw), canaries=True)
    report_and_check(res, name)


# ---------------------------------------------------------------------------------------------------- 2. features
FEATURE_CASES = {
    'S1': dict(S=1),
    'near_field': dict(free_prop=0),
    'fresnel_modes': dict(free_prop=1e-4, n_modes=3),
    'sign_m1': dict(sign_convention=-1),
    'ortho': dict(normalize_fft=True),
    'real_imag': dict(unknown_type='real_imag'),
    'poisson_intensity_modes': dict(loss='poisson', raw_data_type='intensity', poisson_multiplier=50., n_modes=3),
    'beamstop': dict(beamstop=True),
    'binning4_S10': dict(binning=4, S=10),
}


@pytest.mark.parametrize('name', list(FEATURE_CASES))
def test_features_vs_oracle(A, ctx, name):
    """Detector, loss, unknown-type and binning variants of the sweep behind shifted probes, at 40 x 52.

    near_field: with an exit-wave detector and this weak object the terms of dL/ds cancel to 2e-4 ... 4e-4 against 0.05 ... 0.2
    in the far field, so the case is the one that sees the rounding of the phase argument (st_shift_phase forms it in fp64)."""
    kw = dict(S=2, B=6, pp='shifts')
    kw.update(FEATURE_CASES[name])
    report_and_check(run_ps(A, ctx, case_of((40, 52), **kw)), name)


# ---------------------------------------------------------------------------------------------------- 3. contracts
def test_gradients_are_added_to_the_buffers(A, ctx):
    """grad_shifts and grad_probe are accumulated: a non-zero start of grad_shifts comes back with one fp32 addition per element,
    one of grad_probe with the slots added to it in order; views into larger arrays leave their surroundings alone."""
    case = case_of((40, 52), S=2, B=6, n_modes=2, pp='shifts')
    r = np.random.default_rng(11)
    n = len(case['shifts'])
    zero = run_ps(A, ctx, case)
    gs0, gp0 = zero['gs_raw'], zero['gprobe_raw']
    assert np.linalg.norm(gs0) > 0 and np.linalg.norm(gp0) > 0
    gs_init = (np.abs(gs0).max() * r.uniform(-2, 2, (n, 2))).astype(np.float32)
    gp_init = (np.abs(gp0).max() * r.uniform(-2, 2, gp0.shape)).astype(np.float32)
    added = run_ps(A, ctx, case, gs_init=gs_init, gp_init=gp_init, canaries=True)
    assert np.array_equal(added['gs_raw'], gs_init + gs0)
    # probe_grad_reduce starts from the buffer's value and adds the 6 per-position slots to it one by one: 6 roundings of half an
    # ulp of a partial sum each, where the zero start has 5.  With every slot's elements no larger than the largest of the sum
    # (gmax), the partial sums stay below 2 gmax + 6 gmax
    gmax = np.abs(gp0).max()
    err = np.abs(added['gprobe_raw'].astype(np.float64) - (gp_init.astype(np.float64) + gp0)).max()
    print('grad_probe added to a start: worst element off by %.2e (bound %.2e, gmax %.2e)' % (err, 11 * 2. ** -24 * 8 * gmax, gmax))
    assert err <= 11 * 2. ** -24 * 8 * gmax
    for k in ('pred', 'loss', 'grad'):
        assert np.array_equal(np.asarray(zero[k]), np.asarray(added[k])), k


def test_two_launches_give_identical_bits(A, ctx):
    case = case_of((136, 136), S=2, B=6, n_modes=2, pp='shifts')
    a, b = run_ps(A, ctx, case), run_ps(A, ctx, case)
    for k in ('pred', 'loss', 'grad', 'gprobe_raw', 'gs_raw'):
        assert np.array_equal(np.asarray(a[k]), np.asarray(b[k])), k
    assert np.linalg.norm(a['gs_raw']) > 0


def test_no_shift_gradient_leaves_the_rest_unchanged(A, ctx):
    case = case_of((40, 52), S=2, B=6, n_modes=2, pp='shifts')
    with_gs, without = run_ps(A, ctx, case), run_ps(A, ctx, case, want_gs=False)
    for k in ('pred', 'loss', 'grad', 'gprobe_raw'):
        assert np.array_equal(np.asarray(with_gs[k]), np.asarray(without[k])), k
    assert np.all(without['gs_raw'] == 0) and np.linalg.norm(with_gs['gs_raw']) > 0


def test_shift_gradient_only(A, ctx):
    """grad_probe = None: the shift gradient and everything else as with it (the launch that fills the slots is skipped)."""
    case = case_of((40, 52), S=2, B=6, n_modes=2, pp='shifts')
    both, only = run_ps(A, ctx, case), run_ps(A, ctx, case, want_gp=False)
    for k in ('pred', 'loss', 'grad', 'gs_raw'):
        assert np.array_equal(np.asarray(both[k]), np.asarray(only[k])), k
    assert np.all(only['gprobe_raw'] == 0)


def test_forward_only(A, ctx):
    """want_grad = False: prediction and loss of the shifted probes, gradient buffers left as they were."""
    case = case_of((40, 52), S=2, B=6, n_modes=2, pp='shifts')
    gs_init = np.full((len(case['shifts']), 2), 3, np.float32)
    gp_init = np.full((2, 40, 52, 2), 5, np.float32)
    res = run_ps(A, ctx, case, want_grad=False, gs_init=gs_init, gp_init=gp_init, canaries=True)
    e = MM.rel(res['pred'], res['pred_o'])
    print('forward only: pred %.2e, loss %.2e' % (e, abs(res['loss'] / res['loss_o'] - 1)))
    assert e < MM.GENERIC['pred']
    assert abs(res['loss'] - res['loss_o']) <= MM.GENERIC['loss'] * abs(res['loss_o'])
    assert np.array_equal(res['gs_raw'], gs_init) and np.array_equal(res['gprobe_raw'], gp_init)


def test_zero_shifts_match_the_oracle_without_shifts(A, ctx):
    """Shifts of zero: the oracle's case without shifts, under the same bars."""
    case = case_of((40, 52), S=2, B=6, n_modes=2)
    assert case['shifts'] is None
    res = run_ps(A, ctx, case, shifts=np.zeros((6, 2)))
    assert 'gshift' not in res
    report_and_check(res, 'zero shifts')


def test_no_index_one_entry_per_position(A, ctx):
    """index = None with B entries: position b reads entry b and adds to entry b."""
    case = case_of((40, 52), S=2, B=6, n_modes=2, pp='shifts')
    report_and_check(run_ps(A, ctx, case, use_index=False, canaries=True), 'no index')


def test_one_workgroup_plan_ignores_the_switch(A, ctx):
    """probe_shift does not change which plan 'auto' picks: at 24 x 24 the engine stays on the one-workgroup kernels and
    adm_probe_shift serves the shifts, bit for bit as without the keyword."""
    pos = np.array([(0, 0), (3, 5)])
    r = np.random.default_rng(12)
    probe = MM.c2(r.standard_normal((1, 24, 24)) + 1j * r.standard_normal((1, 24, 24)))
    obj = np.stack([1e-3 * r.uniform(size=(30, 30, 2)), 1e-4 * r.uniform(size=(30, 30, 2))], -1).astype(np.float32)
    got = []
    for kw in (dict(), dict(probe_shift=True)):
        eng = A.MultisliceEngine(ctx, (30, 30, 2), (24, 24), pos, MM.ENERGY_EV, MM.PSIZE_CM, max_batch=2, streamed='auto', **kw)
        assert eng.streamed is False and not getattr(eng, 'probe_shift', False)
        gs = ctx.zeros((2, 2))
        eng.set_batch(pos, np.ones((2, 24, 24), np.float32))
        eng.rotate(ctx.array(obj), None)
        eng.multislice(ctx.array(probe), want_pred=True, shifts=ctx.array(np.array([(0.3, -1.2), (2.1, 0.4)], np.float32)), grad_shifts=gs)
        got.append((eng.pred(), eng.loss(), gs.get()))
        eng.plan.close()
    for a, b in zip(*got):
        assert np.array_equal(np.asarray(a), np.asarray(b))
    assert np.linalg.norm(got[0][2]) > 0


# ---------------------------------------------------------------------------------------------------- 4. rounds
@pytest.mark.parametrize('use_index', [True, False], ids=['index', 'no_index'])
def test_rounds_within_workspace_budget(A, ctx, use_index):
    """11 positions of 256 x 256, 2 modes, in 3 rounds: every round passes its slice of the index (or its offset into the
    entries) and adds its share of both gradients.  Loss and prediction bit-equal to the one-round launch."""
    case = case_of(256, S=2, B=11, n_modes=2, pp='shifts', seed=4)
    one = run_ps(A, ctx, case, use_index=use_index)
    parts = run_ps(A, ctx, case, use_index=use_index, workspace_budget=one['ws_bytes_4'], canaries=True)
    assert one['n_rounds'] == 1 and parts['n_rounds'] == 3
    report_and_check(parts, 'rounds')
    assert parts['loss'] == one['loss'] and np.array_equal(parts['pred'], one['pred'])
    e = MM.rel(parts['gshift'], one['gshift'])
    print('rounds vs one launch: dL/ds %.2e, gprobe %.2e' % (e, MM.rel(parts['gprobe'], one['gprobe'])))
    assert e <= shift_bar(parts)
    assert MM.rel(parts['gprobe'], one['gprobe']) < 1e-6


def test_round_offsets_into_the_entries_and_into_the_index(A, ctx):
    """What a round starting at position o is handed: without an index the entries from o on (8 * o bytes into both tables), with
    one the index from o on (4 * o bytes) and the tables whole.  5 positions of 24 x 24 in 3 rounds against one launch, with one
    entry per position and no index, then with the same entries behind a permutation: loss and predictions bit for bit, dL/ds
    inside the bar of the test above."""
    case = case_of((24, 24), S=2, B=5, pp='shifts')
    perm = np.array([3, 0, 4, 1, 2], np.int32)
    entries = np.empty((5, 2))
    entries[perm] = np.asarray(case['shifts'])[case['idx']]           # position b keeps its shift, now at entry perm[b]
    for what, c, use_index in (('no index', case, False), ('index', dict(case, shifts=entries, idx=perm), True)):
        one = run_ps(A, ctx, c, use_index=use_index)
        parts = run_ps(A, ctx, c, use_index=use_index, workspace_budget=one['ws_bytes_2'], canaries=True)
        assert one['n_rounds'] == 1 and parts['n_rounds'] == 3
        assert parts['loss'] == one['loss'] and np.array_equal(parts['pred'], one['pred'])
        e = MM.rel(parts['gshift'], one['gshift'])
        print(what, 'rounds vs one launch: dL/ds %.2e (bar %.2e)' % (e, shift_bar(parts)))
        assert np.linalg.norm(one['gshift']) > 0 and e <= shift_bar(parts)


# ---------------------------------------------------------------------------------------------------- 5. workspace
def test_workspace_of_a_switched_plan(A, ctx):
    """An unswitched streamed plan reports what a plain streamed plan reports; a switched one reports more (the spectra of the
    probe modes and the fp64 partials), a multiple of 8 bytes and linear in the batch (MultisliceEngine.round_cap)."""
    from adorym_amd._lib import check
    for probe, M in (((256, 256), 1), ((1025, 132), 3), ((40, 24), 2)):
        obj = (probe[0] + 37, probe[1] + 20, 3)         # (odd and even frames)
        plan = A.Plan(ctx, obj, probe, ((0, 0), (0, 0)), 1.0, np.ones(probe, complex), n_modes=M, streamed=True)
        w0 = {b: plan.workspace_bytes(b) for b in (1, 2, 3, 7, 64, 300)}
        check(ctx.lib.adm_plan_set_probe_shift(plan.handle, 1))
        w1 = {b: plan.workspace_bytes(b) for b in w0}
        check(ctx.lib.adm_plan_set_probe_shift(plan.handle, 0))
        assert {b: plan.workspace_bytes(b) for b in w0} == w0
        plan.close()
        for b in (3, 7, 64, 300):
            assert w1[b] == w1[1] + (b - 1) * (w1[2] - w1[1]), (probe, b)
        phat = M * probe[0] * probe[1] * 8
        cg = -(-probe[1] // (8 if probe[0] <= 1024 else 4))
        for b in w0:
            assert w1[b] >= w0[b] + phat + b * M * cg * 16 and w1[b] % 8 == 0, (probe, b)


# ---------------------------------------------------------------------------------------------------- 6. refusals
def test_refusals(A, ctx):
    from adorym_amd._lib import check
    pos = np.array([(0, 0), (3, 5)])
    mk = lambda **kw: A.MultisliceEngine(ctx, (30, 30, 3), (24, 24), pos, MM.ENERGY_EV, MM.PSIZE_CM, max_batch=2, **kw)
    with pytest.raises(NotImplementedError, match='probe_shift together with slice_pos_cm'):
        mk(probe_shift=True, slice_pos_cm=[0., 1e-3, 2e-3])
    with pytest.raises(NotImplementedError, match='probe_shift together with exit_shift'):
        mk(probe_shift=True, exit_shift=True)
    with pytest.raises(NotImplementedError, match='probe_shift together with a sequence'):
        mk(probe_shift=True, streamed=True, free_prop_cm=[1e-4, 2e-4])
    lds = mk()                                                   # a plan of adm_plan_create
    assert lds.streamed is False
    with pytest.raises(NotImplementedError, match='streamed plan'):
        check(ctx.lib.adm_plan_set_probe_shift(lds.plan.handle, 1))
    lds.plan.close()
    s, probe = ctx.zeros((2, 2)), ctx.zeros((1, 24, 24, 2))
    st = mk(streamed=True)                                       # streamed, not switched
    st.set_batch(pos, np.ones((2, 24, 24), np.float32))
    with pytest.raises(ValueError, match='adm_plan_set_probe_shift'):
        check(ctx.lib.adm_multislice_fwd_adj_probe_shift(st.plan.handle, st.obj_rot.ptr, probe.ptr, st._cur_pos.ptr, 2, st._cur_target.ptr,
                                                         1, None, None, st._loss.ptr, 1.0, st._ws.ptr, st._ws.nbytes, s.ptr, None, None))
    with pytest.raises(NotImplementedError, match='streamed'):
        st.multislice(probe, shifts=s)
    st.plan.close()
    sw = mk(streamed=True, probe_shift=True)                     # switched: per-position probes stay refused, and the other switches
    sw.set_batch(pos, np.ones((2, 24, 24), np.float32))
    with pytest.raises(NotImplementedError, match='streamed'):
        sw.multislice(None, probes_b=ctx.zeros((2, 1, 24, 24, 2)))
    with pytest.raises(NotImplementedError, match='streamed'):
        check(ctx.lib.adm_probe_shift(sw.plan.handle, probe.ptr, s.ptr, None, 2, ctx.zeros((2, 1, 24, 24, 2)).ptr))
    with pytest.raises(NotImplementedError, match='probe shifts'):
        check(ctx.lib.adm_plan_set_exit_shift(sw.plan.handle, 1))
    z = ctx.array(np.array([0., 1e-3, 2e-3], np.float32))
    with pytest.raises(NotImplementedError, match='probe shifts'):
        check(ctx.lib.adm_plan_set_slice_positions(sw.plan.handle, z.ptr, 3, 0.248, 1.0, 1.0))
    sw.plan.close()
    sp = mk(slice_pos_cm=[0., 1e-3, 2e-3])                       # ... in either order
    with pytest.raises(NotImplementedError, match='slice positions'):
        check(ctx.lib.adm_plan_set_probe_shift(sp.plan.handle, 1))
    sp.plan.close()
    xs = mk(exit_shift=True)
    with pytest.raises(NotImplementedError, match='exit-wave shifts'):
        check(ctx.lib.adm_plan_set_probe_shift(xs.plan.handle, 1))
    xs.plan.close()
