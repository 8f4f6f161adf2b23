"""The holography kernels (adm_holo.hip through HolographyEngine) over the VALUE domain (pytest -m gpu): Fresnel phases to
hundreds of turns, delta/beta objects of many turns, strong and negative absorption, measured data with exact zeros and negative
pixels, matrices that send every sample past the border, a zero probe, shifts beyond the field.  tests/holo_value_matrix.py holds
the classes, their ranges and the reasons for them; tests/test_holo_value_coverage.py decides on the CPU what the oracle pair
alone decides (the one-third rule, the shares each class promises, PHASE_MAX), shows by mutation that the cases bite, and ties
the table to the kernel source.

Judged by holo_matrix.BARS and the 3x rule as they stand, with the helpers of tests/test_gpu_holo_matrix.py (one launch per
engine, whole arrays, then row bands).  Every case also launches twice for identical bits and once forward-only over sentinels,
which no gradient buffer may lose.  Every case is a handful of launches on at most 1024 pixels."""
import numpy as np
import pytest

from tests import holo_matrix as HM
from tests import holo_value_matrix as HV
from tests.test_gpu_holo_matrix import (A, ctx, launch, check_whole, check_row_bands, untouched, same_bits, shift_stage_of)  # noqa: F401

pytestmark = pytest.mark.gpu
BARS = HM.BARS
GRADS = ('g_obj', 'g_probe', 'g_dists', 'g_aff')
cases_of = lambda cls: dict(argnames='p', argvalues=HV.params(cls), ids=HV.case_id)


def name_of(p):
    return '%s %s' % (p[0], HV.case_id(p))


def all_finite(res, what, keys=GRADS + ('pred',)):
    assert np.isfinite(res['loss']), (what, 'loss', res['loss'])
    for k in keys:
        assert np.isfinite(res[k]).all(), (what, k, 'not finite: %d elements' % int((~np.isfinite(res[k])).sum()))


def every_case(ctx, c, res, what, shifted=False):
    """What every case gets: finite results, a second launch with identical bits, and a forward-only launch over sentinels that
    gives the same prediction, the same loss to BARS['loss'], and writes no gradient buffer."""
    keys = GRADS + (('g_shifts', 'target') if shifted else ())
    kw = dict(shifted=True, want=('probe', 'shifts')) if shifted else {}
    all_finite(res, what, keys + ('pred',))
    again = launch(ctx, c, **kw)
    assert again['loss'] == res['loss'], (what, again['loss'], res['loss'])
    for k in keys + ('pred',):
        same_bits(again[k], res[k], (what, k, 'two launches'))
    fwd = launch(ctx, c, want_grad=False, seed='sentinel', **kw)
    untouched(fwd, ('g_obj', 'g_probe', 'g_shifts') if shifted else GRADS, what)
    # (the forward-only launch sums the loss in holo_sums_kernel, the gradient launch in K5: another order, the same terms)
    assert abs(fwd['loss'] / res['loss'] - 1) < BARS['loss'], (what, 'forward-only loss', fwd['loss'], res['loss'])
    same_bits(fwd['pred'], res['pred'], (what, 'forward-only prediction'))


def judged_in_full(ctx, p):
    c = HV.case(*p)
    what = name_of(p)
    res = launch(ctx, c)
    check_whole(res, c, what)
    check_row_bands(res, c, what)
    every_case(ctx, c, res, what)
    return c, res


# ------------------------------------------------------------------------------------------------------------ the Fresnel phase
@pytest.mark.parametrize(**cases_of('fresnel_phase'))
def test_fresnel_phase(ctx, p):
    """holo_h's sincos_fast at arguments to 100 rad, 1000 rad and PHASE_MAX (3000 rad for the matrix's smooth inputs, 300 rad for
    object and data of uncorrelated noise, which put signal where the phase is large), both sigma, the long axis in either stage:
    loss, prediction and every gradient against the fp64 oracle, whole and by row bands."""
    c, _ = judged_in_full(ctx, p)
    print('%s: largest |arg| %.0f rad' % (name_of(p), HV.max_arg(c)))


@pytest.mark.parametrize(**cases_of('unitarity'))
def test_unitarity(ctx, p):
    """|arg| to 3e5 rad, beyond what sincos_fast claims: every output is finite, and every distance keeps the energy of the exit
    wave (H is unimodular) as well as the float32 oracle does on the same inputs: 3 x its own defect + BARS['loss']."""
    c = HV.case(*p)
    what = name_of(p)
    assert HV.max_arg(c) > HV.SINCOS_CLAIM
    res = launch(ctx, c)
    every_case(ctx, c, res, what)
    e, e32 = np.abs(HV.energy_defect(res['pred'], c)), np.abs(HV.energy_defect(c['o32']['pred'], c, np.float32))
    for d in range(c['nd']):
        print('%s: distance %d (%.3g cm): energy defect %.2e (fp32 oracle %.2e, bar %.2e)' % (what, d, c['dists'][d], e[d], e32[d], 3 * e32[d] + BARS['loss']))
    assert (e <= 3 * e32 + BARS['loss']).all(), (what, e, e32)


# ------------------------------------------------------------------------------------------------------------ delta/beta objects
@pytest.mark.parametrize(**cases_of('delta_beta_turns'))
def test_delta_beta_turns(ctx, p):
    """holo_transmission's sincosf at phases over +-6 turns, both sigma."""
    c, _ = judged_in_full(ctx, p)
    assert np.abs(HV.k1_phase(c)[0]).max() > 0.95 * HV.PHI_MAX


@pytest.mark.parametrize(**cases_of('delta_beta_absorbing'))
def test_delta_beta_absorbing(ctx, p):
    """holo_transmission's expf at k1 beta over [0, 30] and, at four voxels or more, in (88, 120], where the transmission is a
    denormal or 0: the gradient there is finite (and, by the chain rule, as small)."""
    c, res = judged_in_full(ctx, p)
    kb = HV.k1_phase(c)[1]
    deep = kb > HV.K1B_UNDERFLOW[0]
    assert deep.sum() >= 4 and kb.max() > 104
    assert np.abs(res['g_obj'][deep]).max() <= 1e-30 * np.abs(res['g_obj']).max()


@pytest.mark.parametrize(**cases_of('delta_beta_amplifying'))
def test_delta_beta_amplifying(ctx, p):
    """15 % of the voxels with k1 beta in [-2, 0): transmissions up to e^2."""
    c, _ = judged_in_full(ctx, p)
    assert abs((HV.k1_phase(c)[1] < 0).mean() - HV.AMPLIFYING_SHARE) < 0.01


# ------------------------------------------------------------------------------------------------------------ measured data
@pytest.mark.parametrize(**cases_of('zero_block'))
def test_zero_block(ctx, p):
    """A 7 x 7 block of exact zeros in the data of every distance, intensity and magnitude: under intensity the cotangent of an
    exactly zero sample is the guarded 0/0.  Every gradient is finite, the prediction has the bits it has without the zeros, and
    the gradients pass the 3x rule -- under the offset matrices all of them; under identity matrices those HV.UNJUDGED does not
    list (there the oracle pair itself disagrees: see the table), and the launch equals the one without matrices bit for bit."""
    c = HV.case(*p)
    what = name_of(p)
    res = launch(ctx, c)
    every_case(ctx, c, res, what)
    plain = launch(ctx, dict(c, data=c['plain_data']))
    same_bits(res['pred'], plain['pred'], (what, 'the prediction depends on the data'))
    assert plain['loss'] != res['loss']
    left = HV.unjudged(p)
    if p[2]['matrices'] == 'identity':
        none = launch(ctx, dict(c, has_affine=False))
        assert none['loss'] == res['loss']
        for k in GRADS + ('pred',):
            same_bits(none[k], res[k], (what, k, 'affine = NULL equals identity matrices'))
    if not left:
        check_whole(res, c, what)
        check_row_bands(res, c, what)
    elif 'loss' not in left:
        assert left == ('gaff',)
        check_whole(res, c, what, oracle_affine=False)
        check_row_bands(res, c, what)
    else:
        e, e32 = HM.rel(res['pred'], c['o64']['pred']), HM.rel(c['o32']['pred'], c['o64']['pred'])
        print('%s: pred %.2e (fp32 oracle %.2e); loss %.2e and the gradients are not judged' % (what, e, e32, abs(res['loss'] / c['o64']['loss'] - 1)))
        assert e < BARS['pred'], (what, e)


@pytest.mark.parametrize(**cases_of('negative_data'))
def test_negative_data(ctx, p):
    """A tenth of the pixels negated; the target is sqrt|samp| or |samp|, the cotangent carries sign(samp), and a third of the
    samples mix pixels of both signs."""
    judged_in_full(ctx, p)


# ------------------------------------------------------------------------------------------------------------ matrices
@pytest.mark.parametrize(**cases_of('all_clamped'))
def test_all_clamped(ctx, p):
    """Every sample beyond the border along x, along y, along both: the matrix gradient's row of a masked axis is exactly zero,
    the other row passes the 3x rule, and nothing but the border pixels reaches any result -- the launch on data whose every
    pixel is replaced by the border pixel the clamped coordinate reads gives the same bits."""
    c = HV.case(*p)
    what = name_of(p)
    axes = p[2]['axes']
    res = launch(ctx, c)
    for q, a in enumerate('xy'):
        if a in axes:
            assert not res['g_aff'][:, q].any(), (what, 'row %d of the matrix gradient' % q, res['g_aff'][:, q])
        else:
            assert np.abs(res['g_aff'][:, q]).min() > 0, (what, q)
    check_whole(res, c, what, oracle_affine=axes != 'xy')
    check_row_bands(res, c, what)
    every_case(ctx, c, res, what)
    edge = HV.border_data(c)
    assert (edge != c['data']).mean() > 0.5
    same = launch(ctx, dict(c, data=edge))
    assert same['loss'] == res['loss'], (what, same['loss'], res['loss'])
    for k in GRADS:
        same_bits(same[k], res[k], (what, k, 'pixels off the border reach the result'))


# ------------------------------------------------------------------------------------------------------------ the probe
@pytest.mark.parametrize(**cases_of('zero_probe'))
def test_zero_probe(ctx, p):
    """A probe of zeros: the prediction and the object, probe and distance gradients are exactly zero (K3's guard for a zero
    prediction), the loss is the mean of the squared targets, the matrix gradient passes the 3x rule, nothing is NaN."""
    c = HV.case(*p)
    o, s = c['o64'], c['o32']
    what = name_of(p)
    res = launch(ctx, c)
    every_case(ctx, c, res, what)
    for k in ('pred', 'g_obj', 'g_probe', 'g_dists'):
        assert not np.asarray(res[k]).any(), (what, k, 'not exactly zero')
        assert not np.asarray(o[k]).any()
    e = abs(res['loss'] / float(np.mean(o['target'] ** 2)) - 1)
    print('%s: loss %.2e' % (what, e))
    assert e < BARS['loss'], (what, e)
    e, e32 = HM.rel(res['g_aff'], o['g_aff']), HM.rel(s['g_aff'], o['g_aff'])
    print('%s: g_aff %.2e (fp32 oracle %.2e, bar %.1e)' % (what, e, e32, max(BARS['gaff'], 3 * e32)))
    assert e < max(BARS['gaff'], 3 * e32), (what, e, e32)


# ------------------------------------------------------------------------------------------------------------ the shift stage
@pytest.mark.parametrize(**cases_of('large_shifts'))
def test_large_shifts(ctx, p):
    """holo_sli / holo_sri / holo_sr / holo_slf at shifts beyond the field (the phase -2 pi (fx sx + fy sy) reaches 500 rad),
    judged as test_shift_stage judges.  Integer shifts, 0 and +-(n + 3): the registered targets are the circular roll of
    sqrt|data|."""
    c = HV.case(*p)
    what = name_of(p)
    res = shift_stage_of(ctx, c, what)
    every_case(ctx, c, res, what, shifted=True)
    if p[2]['kind'] == 'integer':
        e = HM.rel(np.sqrt(np.abs(res['target'])), HV.rolled_targets(c))
        print('%s: targets against the rolled data %.2e' % (what, e))
        assert e < BARS['target'], (what, e)
