"""The detector fan-out over distance, batch and mode COUNTS, through the engine, against the NumPy restatement in fp64
(tests/multidist3d_ref.py, tied to golden F27 on the CPU) with its fp32 run as the yardstick (pytest -m gpu).

The rows, their classes and the mirrors of what they reach are tests/fan_matrix.py's; tests/test_fanout_domain_coverage.py shows on
the CPU that the fp32 restatement leaves room under every bar applied here and that the bars see a dropped, mis-ordered or
mis-indexed entry, distance or mode.  Bars: ms_matrix.GENERIC through ms_matrix.check, and the band rule of count_matrix item by
item -- none changed, none added.  Every figure is printed before it is asserted.
"""
import numpy as np
import pytest

from tests import fan_matrix as FM
from tests import ms_matrix as MM
from tests import test_gpu_multidist3d as MD
from tests.test_gpu_count_domain import same_bits

pytestmark = pytest.mark.gpu
BARS = FM.BARS
BIT_KEYS = ('pred', 'loss', 'loss_sum', 'grad', 'gprobe_raw')


@pytest.fixture(scope='module')
def A():
    import adorym_amd
    return adorym_amd


@pytest.fixture(scope='module')
def ctx(A):
    c = A.Context(0)
    yield c
    c.close()


def judge(case, res, what):
    res = FM.dressed(case, res)
    MD.report(res, what)
    print(what, 'fractions of the bars:', {k: round(float(v), 4) for k, v in FM.fractions(res).items()})
    FM.check_entries(res, BARS, what)
    return res


# ------------------------------------------------------------------------------------------------------------ against the restatement
@pytest.mark.parametrize('name', list(FM.CASES))
def test_counts(A, ctx, name):
    """md_fanout_kernel and md_fanin_kernel to D = 64, the row launches, st_det_kernel and st_loss_reduce_kernel over E = B * D
    entries on both sides of 256 (and beyond 512), the parked detector fields to M = 64, the probe-gradient reduction over
    B = 32 / 33 / 65 positions, and the distance axis: descending, repeated, near-field and aliased distances, both signs."""
    case = FM.build(name)
    res = FM.run(A, ctx, case)
    assert res['n_rounds'] == 1
    judge(case, res, name)


def test_engine_refuses_65_distances(A, ctx):
    """The other side of n <= 64: the engine hands the 65 kernels to adm_plan_set_detector_fanout, which refuses."""
    case = FM.build_counts(3, 3, 1)
    with pytest.raises(ValueError, match='adm_plan_set_detector_fanout: n must be in'):
        MD._engine(A, ctx, case, FM.default_dists(FM.MAX_FAN + 1))


def test_large_cases_twice(A, ctx):
    for name in FM.TWICE:
        case = FM.build(name)
        a, b = FM.run(A, ctx, case), FM.run(A, ctx, case)
        same_bits(a, b, BIT_KEYS)
        assert np.linalg.norm(a['grad']) > 0 and np.linalg.norm(a['gprobe_raw']) > 0 and np.linalg.norm(a['loss_sum']) > 0


# ------------------------------------------------------------------------------------------------------------ one term of the fan-in
ONE_LIVE = [('B3_D4_M2', d) for d in range(4)] + [('B3_D64_M1', d) for d in (0, 31, 63)]


@pytest.fixture(scope='module')
def live_cases():
    return {'B3_D4_M2': FM.make_case(B=3, D=4, M=2, seed=3), 'B3_D64_M1': FM.make_case(B=3, D=64, M=1, seed=3)}


@pytest.mark.parametrize('name,d', ONE_LIVE, ids=lambda v: v if isinstance(v, str) else 'd%d' % v)
def test_one_live_distance(A, ctx, live_cases, name, d):
    """The targets of every entry whose distance is not d are the GPU's own prediction (a forward-only launch; launches are
    bit-repeatable), so their factor of dL/dPsi is exactly 0 and the fan-in's sum has ONE term: H_d, detector field d, place d.
    The object and probe gradients meet the restatement run on the same targets."""
    case = live_cases[name]
    D = len(case['dists'])
    eng = MD._engine(A, ctx, case, case['dists'])
    eng.set_batch(case['pos'], case['target'])
    eng.rotate(ctx.array(case['obj'], np.float32), None)
    eng.multislice(ctx.array(MM.c2(case['probes'])), want_grad=False, want_pred=True)
    own = eng.pred()
    target = np.array(own, np.float32)
    target[d::D] = case['target'][d::D]
    res = FM.run(A, ctx, case, engine=eng, target=target)
    eng.plan.close()
    assert np.array_equal(res['pred'], own), 'the two launches differ'
    dead = np.ones(len(target), bool)
    dead[d::D] = False
    assert (res['loss_sum'][dead] == 0).all() and (res['loss_sum'][~dead] > 0).all(), res['loss_sum']
    live = FM.with_refs(dict(case, meas=target, target=target))
    out = FM.dressed(live, res)
    MD.report(out, '%s, distance %d alone' % (name, d))
    MM.check(out, BARS)
    for k in ('grad', 'gprobe'):        # (the 3 x rule for both gradients, every mode on its own)
        MM._grad_ok(MM.rel(out[k], out[k + '_o']), MM.rel(out[k + '_32'], out[k + '_o']), BARS, '%s with distance %d alone' % (k, d))
    for m in range(len(out['gprobe'])):
        MM._grad_ok(MM.rel(out['gprobe'][m], out['gprobe_o'][m]), MM.rel(out['gprobe_32'][m], out['gprobe_o'][m]), BARS, 'mode %d' % m)


# ------------------------------------------------------------------------------------------------------------ host paths times D
@pytest.mark.parametrize('name', list(FM.ROUNDS))
def test_rounds_of_several_positions(A, ctx, name):
    """A workspace budget that holds fewer positions than the batch: the rounds start at entry o * D of the targets, predictions
    and loss sums.  Losses, loss sums and predictions are the one-round launch's bit for bit, the gradients up to the order of
    the overlap-add and within the bars of the restatement."""
    from adorym_amd.propagate import equal_parts
    B, D, M, cap, split = FM.ROUNDS[name]
    case = FM.build_counts(B, D, M, seed=4)
    one = FM.run(A, ctx, case)
    probe_eng = MD._engine(A, ctx, case, case['dists'])
    budget = probe_eng.plan.workspace_bytes(cap)
    probe_eng.plan.close()
    parts = FM.run(A, ctx, case, workspace_budget=budget)
    assert [n for _, n in equal_parts(B, cap)] == split and sum(split) == B
    assert one['n_rounds'] == 1 and parts['n_rounds'] == len(split)
    print(name, 'entries per round', [n * D for n in split])
    same_bits(one, parts, ('pred', 'loss', 'loss_sum'))
    eg, ep = MM.rel(parts['grad'], one['grad']), MM.rel(parts['gprobe'], one['gprobe'])
    print(name, 'against one round: grad %.2e  gprobe %.2e' % (eg, ep))
    assert eg < 1e-6 and ep < 1e-6, (eg, ep)
    judge(case, parts, name)


def test_engine_reused_across_batch_sizes(A, ctx):
    """One engine runs B = 2, B = 5 (_reserve grows the targets, predictions, loss sums and the upload ring, all sized by B * D)
    and B = 2 again, at D = 3, M = 2; each result is a fresh engine's bit for bit."""
    big = FM.build_counts(5, 3, 2, seed=5)
    D = len(big['dists'])
    # positions 0 and 2 hang over the top and the bottom edge: their rows cover the object, as launch()'s full-range adjoint assumes
    ent = np.r_[0:D, 2 * D:3 * D]
    small = dict(big, pos=big['pos'][[0, 2]], target=big['target'][ent], meas=big['meas'][ent])
    lo, hi = big['pos'][[0, 2], 0].min(), big['pos'][[0, 2], 0].max() + FM.FIELD[0]
    assert lo <= 0 and hi >= big['obj'].shape[0] and big['pos'][0, 0] + FM.FIELD[0] >= big['pos'][2, 0]
    eng = MD._engine(A, ctx, big, big['dists'])         # (built on all five positions: the pads of both batches)
    for k, case in enumerate((small, big, small)):
        got = FM.run(A, ctx, case, engine=eng)
        assert eng.max_batch == (2 if k == 0 else 5)
        fresh_eng = MD._engine(A, ctx, big, big['dists'])
        fresh = FM.run(A, ctx, case, engine=fresh_eng)
        fresh_eng.plan.close()
        same_bits(got, fresh, BIT_KEYS)
        assert len(got['pred']) == len(case['pos']) * D and np.linalg.norm(got['grad']) > 0
    eng.plan.close()
    judge(big, FM.run(A, ctx, big), 'B5_D3_M2')


def test_loss_readbacks_count_entries(A, ctx):
    """loss(), loss(last=n), loss_async / loss_result at (5, 3, 1): means over 15 and over the last 6 ENTRIES."""
    case = FM.build_counts(5, 3, 1, seed=6)
    B, D = 5, 3
    n_det = case['probes'].shape[-2] * case['probes'].shape[-1]
    eng = MD._engine(A, ctx, case, case['dists'])
    probe = ctx.array(MM.c2(case['probes']))

    def queue():
        eng.set_batch(case['pos'], case['target'])
        eng.rotate(ctx.array(case['obj'], np.float32), None)
        eng.multislice(probe, want_grad=False)

    queue()
    sums = eng.loss_sums(B * D)
    assert sums.shape == (B * D,) and (sums > 0).all()
    whole, last2 = float(sums.sum() / (B * D * n_det)), float(sums[-2 * D:].sum() / (2 * D * n_det))
    assert eng.loss() == whole and eng.loss(last=2) == last2, (eng.loss(), whole, eng.loss(last=2), last2)
    # the deferred read-back, resolved at once ...
    queue()
    t_all = eng.loss_async()
    assert eng.loss_result(t_all) == whole
    queue()
    t_last = eng.loss_async(last=2)
    assert eng.loss_result(t_last) == last2
    # ... and with a second launch queued in between (it writes the other loss buffer)
    queue()
    t_all = eng.loss_async()
    queue()
    t_last = eng.loss_async(last=2)
    assert eng.loss_result(t_all) == whole and eng.loss_result(t_last) == last2
    eng.plan.close()
    want_all = case['loss_o']
    want_last = float(case['loss_e_o'][-2 * D:].sum() / (2 * D * n_det))
    assert abs(float(case['loss_e_o'].sum() / (B * D * n_det)) - want_all) <= 1e-12 * want_all
    print('loss %.3e of the restatement, of the last two positions %.3e' % (abs(whole / want_all - 1), abs(last2 / want_last - 1)))
    assert abs(whole - want_all) <= BARS['loss'] * want_all and abs(last2 - want_last) <= BARS['loss'] * want_last


def test_no_prediction_buffer(A, ctx):
    """want_pred off with a fan-out (the ABI takes pred = NULL): loss, loss sums and gradients are the want_pred launch's bit for
    bit and the prediction buffer, filled with a sentinel beforehand, is untouched."""
    case = FM.build_counts(5, 3, 2, seed=5)
    with_pred = FM.run(A, ctx, case)
    M, Py, Px = case['probes'].shape
    eng = MD._engine(A, ctx, case, case['dists'])
    d_grad, d_gp = ctx.zeros(case['obj'].shape), ctx.zeros((M, Py, Px, 2))
    eng.set_batch(case['pos'], case['target'])
    sentinel = np.full(eng._pred.shape, -7.5, np.float32)
    eng._pred.set(sentinel)
    eng.rotate(ctx.array(case['obj'], np.float32), None)
    eng.multislice(ctx.array(MM.c2(case['probes'])), grad_probe=d_gp, want_pred=False)
    eng.rotate_adjoint(d_grad, None)
    got = dict(loss=eng.loss(), loss_sum=eng.loss_sums(len(case['pos']) * len(case['dists'])), grad=d_grad.get(), gprobe_raw=d_gp.get())
    assert np.array_equal(eng._pred.get(), sentinel), 'the prediction buffer was written'
    eng.plan.close()
    same_bits(with_pred, got, ('loss', 'loss_sum', 'grad', 'gprobe_raw'))
    assert np.linalg.norm(got['grad']) > 0
