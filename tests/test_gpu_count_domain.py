"""The multislice paths over batch, mode and shift-entry COUNTS, through the engine, against the fp64 oracle (pytest -m gpu).

The rows, their classes and the mirrors of the arithmetic they reach are tests/count_matrix.py's; tests/test_count_domain_coverage.py
shows on the CPU that the fp32 oracle leaves room under every bar applied here and that the bars see a dropped or mis-indexed
position.  Bars: ms_matrix.TUNED for the tuned kernels, ms_matrix.GENERIC for the any-size kernel and the streamed path,
``shift_bar`` of test_gpu_streamed_probe_shift.py for the streamed shift gradient, ``check_3x`` of test_gpu_prj_offset.py and of
test_gpu_sparse_multislice.py for their cases -- none of them changed, none added.  Every figure is printed before it is asserted.
"""
import numpy as np
import pytest

from tests import count_matrix as CM
from tests import ms_matrix as MM
from tests import test_gpu_prj_offset as XS
from tests import test_gpu_sparse_multislice as SP
from tests.test_gpu_streamed_probe_shift import shift_bar

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


def report(res, what):
    f = lambda k: '%.2e (%.2e)' % (MM.rel(res[k], res[k + '_o']), MM.rel(res[k + '_32'], res[k + '_o']))
    print(what, 'pred', f('pred'), 'loss %.2e (%.2e)' % (abs(res['loss'] / res['loss_o'] - 1), abs(res['loss_32'] / res['loss_o'] - 1)),
          'grad', f('grad'), 'gprobe', f('gprobe') if res.get('gprobe') is not None else None,
          'gshift', f('gshift') if res.get('gshift') is not None else None, 'cover', res.get('cover'), '(fp32 oracle in brackets)')


def judge(res, name, what=''):
    """The family's whole-array bars, then every count on its own; shift entries nobody uses keep their seed bit for bit."""
    spec = CM.CASES[name]
    bars = CM.bars_of(spec['family'])
    name = name + what
    report(res, name)
    MM.check(res, bars)
    if res.get('gshift') is not None:
        assert np.linalg.norm(res['gshift_o']) > 0
        if spec['family'] == 'streamed':
            e = MM.rel(res['gshift'], res['gshift_o'])
            assert e <= shift_bar(res), ('shift gradient', e, shift_bar(res))
        unused = ~CM.used_entries(res)
        assert np.array_equal(res['gs_raw'][unused].view(np.uint32), res['gs_seed'][unused].view(np.uint32)), 'an unused entry was written'
        assert (res['gs_seed'][unused] == CM.UNUSED_SEED).all()
    CM.check_counts(res, bars, name)


def same_bits(a, b, keys):
    for k in keys:
        x, y = np.ascontiguousarray(a[k], np.float32), np.ascontiguousarray(b[k], np.float32)
        assert np.array_equal(x.view(np.uint32), y.view(np.uint32)), k


def family_rows(family):
    return [n for n, c in CM.CASES.items() if c['family'] == family]


# ------------------------------------------------------------------------------------------------------------ against the oracle
@pytest.mark.parametrize('name', family_rows('tuned'))
def test_tuned(A, ctx, name):
    """ms_fwd_adj_kernel over xcd_position's q and r and its MULTI branch to 64 modes; probe_shift_kernel, probe_shift_adj_kernel
    and the two probe_grad_reduce kernels on both sides of the 256 (position, mode) pairs and of the chunk of 32."""
    res = CM.run(A, ctx, CM.build(name), 'tuned')
    dense = name == CM.DENSE
    assert (res['cover'] > CM.MAX_COVER) == dense, res['cover']
    judge(res, name)


@pytest.mark.parametrize('name', family_rows('generic'))
def test_generic(A, ctx, name):
    """ms_generic_kernel: a grid of 1 and of 257, its mode loops to 64, b % n_hfree with three distances and one probe set."""
    judge(CM.run(A, ctx, CM.build(name), 'generic'), name)


@pytest.mark.parametrize('name', family_rows('streamed'))
def test_streamed(A, ctx, name):
    """st_row_kernel, st_col_conv_kernel, st_det_kernel over B * M fields and 64 modes; st_loss_reduce_kernel's second workgroup;
    ps_col_kernel and both loops of st_shift_reduce_kernel beyond their first trip, under every index pattern."""
    res = CM.run(A, ctx, CM.build(name), 'streamed')
    assert res['n_rounds'] == 1
    judge(res, name)


def test_exit_shift(A, ctx):
    """es_col_conv_kernel and st_shift_reduce_kernel at B = 257 (24 x 20, a ragged last column group) under the 'mixed' index."""
    case = CM.build('exit_shift_B257')
    r64, e32 = XS.yardstick(case)
    unused = np.setdiff1d(np.arange(len(case['shifts'])), case['index'])
    seed = np.zeros((len(case['shifts']), 2), np.float32)
    seed[unused] = CM.UNUSED_SEED
    res = XS.run_shifted(A, ctx, case, gs_init=seed, canaries=True, keep_engine=True)
    res['loss_sum'] = res['engine'].loss_sums(len(case['pos']))
    res.pop('engine').plan.close()
    assert len(unused) >= 2 and np.array_equal(res['gs_raw'][unused].view(np.uint32), seed[unused].view(np.uint32))
    res['gs'] = res['gs'] - seed                    # (exact: one of the two is zero everywhere)
    XS.check_3x(res, r64, e32, 'exit_shift_B257')
    r32 = XS.ref_shifted(case, 'float32')
    l64, l32 = CM.loss_sums_of(r64['pred'], case['meas']), CM.loss_sums_of(r32['pred'], case['meas'])
    used = np.unique(case['index'])
    print('exit_shift_B257 each count:',
          CM._items(res['pred'], r64['pred'], r32['pred'], XS.BARS['pred'], 'pred of a position'),
          CM._items(res['loss_sum'], l64, l32, XS.BARS['loss'], 'loss sum of a position'),
          # (the whole-array bar of dL/ds in check_3x is gs_bar of the whole-array yardstick: that is the floor of the band rule
          # here, as GENERIC['shift'] is for the probe shifts.  Its constant part alone, 2^-24, is no floor for ONE entry: the sum
          # of ~30 cancelling positions was 1.2e-6 of its own norm off against the fp32 reference's 1.9e-7 on one entry of one
          # draw, while the whole array was 2.4e-7 against 4.9e-7.)
          CM._items(res['gs'][used], np.asarray(r64['gs'])[used], np.asarray(r32['gs'])[used], XS.gs_bar(e32[4]), 'offset gradient of an entry'))


@pytest.mark.parametrize('name', family_rows('sparse'))
def test_sparse(A, ctx, name):
    """st_col_conv_sparse_kernel and st_dd_reduce_kernel (its npart = B * M * column groups partials) at B = 257 and M = 5."""
    case = CM.build(name)
    r64, e32 = SP.yardstick(case)
    res = SP.run_sparse(A, ctx, case, keep_engine=True)
    res['loss_sum'] = res['engine'].loss_sums(len(case['pos']))
    res.pop('engine').plan.close()
    SP.check_3x(res, r64, e32, e32[4], name)
    r32 = SP.ref_sparse(case, 'float32')
    l64, l32 = CM.loss_sums_of(r64['pred'], case['meas']), CM.loss_sums_of(r32['pred'], case['meas'])
    print(name, 'each count:',
          CM._items(res['pred'], r64['pred'], r32['pred'], SP.BARS['pred'], 'pred of a position'),
          CM._items(res['loss_sum'], l64, l32, SP.BARS['loss'], 'loss sum of a position'),
          CM._items(res['gprobe'], r64['gprobe'], r32['gprobe'], SP.BARS['grad_abs'], 'probe gradient of a mode', cap=SP.BARS['grad']))


def test_65_modes_are_refused(A, ctx):
    """The other side of n_modes <= 64: adm_plan_create refuses, on either kind of plan."""
    for kw in (dict(), dict(streamed=True)):
        with pytest.raises(ValueError, match='n_modes'):
            A.MultisliceEngine(ctx, (20, 20, 2), (8, 8), np.array([(0, 0)]), MM.ENERGY_EV, MM.PSIZE_CM, n_probe_modes=CM.MAX_MODES + 1, **kw)


# ------------------------------------------------------------------------------------------------------------ bit for bit
BIT_KEYS = ('pred', 'loss_sum', 'grad', 'gprobe_raw', 'gs_raw')


def test_streamed_shift_B300_twice(A, ctx):
    case = CM.build('streamed_shift_B300_mixed')
    a, b = CM.run(A, ctx, case, 'streamed'), CM.run(A, ctx, case, 'streamed')
    same_bits(a, b, BIT_KEYS)
    assert np.linalg.norm(a['gs_raw']) > 0


def test_slot_path_twice(A, ctx):
    """B = 5, M = 64: the slot path (one chunk, a second level of one) leaves nothing to the order of atomics."""
    case = CM.build('tuned_shift_B5_M64')
    a, b = CM.run(A, ctx, case, 'tuned'), CM.run(A, ctx, case, 'tuned')
    same_bits(a, b, ('pred', 'loss_sum', 'gprobe_raw'))
    assert np.linalg.norm(a['gprobe_raw']) > 0


def test_streamed_shift_B300_in_rounds(A, ctx):
    """300 positions in seven rounds (six of 43, a last one of 42) under the 'mixed' index, whose entries cross the rounds: loss
    and prediction bit-identical to the single launch, the gradients inside the same bars."""
    name = 'streamed_shift_B300_mixed'
    case = CM.build(name)
    one = CM.run(A, ctx, case, 'streamed')
    parts = CM.run(A, ctx, case, 'streamed', workspace_budget=one['ws_bytes'][43])
    from adorym_amd.propagate import equal_parts
    assert one['n_rounds'] == 1 and parts['n_rounds'] == 7 and [n for _, n in equal_parts(300, 43)] == [43] * 6 + [42]
    same_bits(one, parts, ('pred', 'loss_sum'))
    assert parts['loss'] == one['loss']
    judge(parts, name, ' in rounds')
