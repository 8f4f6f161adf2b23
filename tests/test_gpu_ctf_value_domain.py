"""The CTF kernels over the VALUE domain (pytest -m gpu): adm_holo_ctf.hip's C1 ... C5 through adm_ctf_fwd_adj (distances as host
doubles) and adm_ctfd_fwd_adj (a float32 device array, with grad_dists), adm_ctf_invert.hip's I1 ... I3 through adm_ctfinv_run --
kappa from 0.3 to 1e50, contrast up to I crossing zero, min I down to 1e-3, distances down to 0 and below, three energies and
pixel sizes, data with exact zeros, negative values, four decades of scale and non-finite values, a non-finite beta channel.
tests/ctf_value_matrix.py holds the classes, their ranges and the reasons for them; tests/test_ctf_value_coverage.py decides on
the CPU what the reference pair alone decides (the one-third rule, the caps, every figure), shows by mutation that the cases bite
and ties the table to the sources.

Judged by ctf_matrix.BARS (check_whole of tests/test_gpu_ctf.py), ctf_dist_matrix.dist_bar (check_dists of
tests/test_gpu_ctf_dist.py) and 3 x the restatement's error per inversion case, as they stand; each prints its error next to the
float32 restatement's.  Every forward/adjoint case is one handle, one overwriting launch per entry into NaN-filled gradient
buffers and one forward-only launch per entry, on at most 512 pixels."""
import numpy as np
import pytest

from tests import ctf_matrix as CM
from tests import ctf_value_matrix as V
from tests.test_gpu_ctf import A, ctx, Handle, check_whole, same_bits  # noqa: F401
from tests.test_gpu_ctf import launch as host_launch
from tests.test_gpu_ctf_dist import launch as device_launch
from tests.test_gpu_ctf_dist import check_dists
from tests.test_gpu_ctfinv import engine, run

pytestmark = pytest.mark.gpu
BARS = V.BARS
OUTPUTS = ('pred', 'loss_d', 'g_obj', 'g_kappa', 'g_dists')
cases_of = lambda cls: dict(argnames='p', argvalues=V.params(cls), ids=V.case_id)
inv_cases_of = lambda cls: dict(argnames='p', argvalues=V.inv_params(cls), ids=lambda p: p[1] if isinstance(p, tuple) else str(p))


def both(ctx, c, data=None):
    """The case through both entries on one handle, overwriting NaN-filled gradient buffers: {'host': ..., 'device': ...}.  The
    beta channel of an overwriting launch is +0.  Each entry then runs forward-only (ctf_c3<N, false>, ctf_sums_kernel): the same
    prediction bits, the same loss sums, and no gradient buffer written."""
    c = c if data is None else dict(c, data=data)
    h = Handle(ctx, c['ny'], c['nx'], c['nd'], c['raw'], energy_ev=c['energy'], psize_cm=c['psize'])
    try:
        calls = dict(host=(host_launch, dict(c, dists=c['model_dists'])), device=(device_launch, c))
        res = {entry: fn(ctx, cc, h=h, overwrite=True, seed='nan') for entry, (fn, cc) in calls.items()}
        fwd = {entry: fn(ctx, cc, h=h, want_grad=False, seed='nan') for entry, (fn, cc) in calls.items()}
    finally:
        h.close()
    for entry, r in res.items():
        assert not CM.bits(r['g_obj'][..., 1]).any(), (c['name'], entry, 'dL/dbeta is not +0')
        f = fwd[entry]
        same_bits(f['pred'], r['pred'], (c['name'], entry, 'forward-only prediction'))
        assert np.array_equal(f['loss_d'], r['loss_d'], equal_nan=True), (c['name'], entry, 'forward-only loss sums', f['loss_d'], r['loss_d'])
        for k, seed in f['seeds'].items():
            same_bits(f[k], seed, (c['name'], entry, k, 'written by a forward-only launch'))
    return res


_PLAIN = {}


def plain(ctx, field, raw='intensity'):
    """The unedited inputs of a field, launched once per module."""
    if (field, raw) not in _PLAIN:
        _PLAIN[field, raw] = both(ctx, V.case('plain', field, dict(raw=raw)))
    return _PLAIN[field, raw]


def finite(res, what, keys=OUTPUTS):
    for entry, r in res.items():
        for k in keys:
            if k in r:
                assert np.isfinite(r[k]).all(), (what, entry, k, 'not finite: %d elements' % int((~np.isfinite(r[k])).sum()))


def referenced(res, c, p):
    """Both entries against the fp64 reference, each with the float32 restatement of its own roundings as the yardstick."""
    keys = V.judged(p)
    finite(res, c['name'], tuple(k for k in OUTPUTS if k != 'g_kappa' or 'gkappa' in keys))
    for entry, r in res.items():
        cc = c if entry == 'device' else dict(c, o32=c['o32h'])
        check_whole(r, cc, '%s, %s distances' % (c['name'], entry), grad='grad' in keys, kappa='gkappa' in keys)
    if 'gdists' in keys:
        check_dists(res['device'], c, c['name'])


def equal_outputs(a, b, what, keys=OUTPUTS):
    for entry in a:
        for k in keys:
            if k in a[entry]:
                same_bits(a[entry][k], b[entry][k], (what, entry, k))


# ------------------------------------------------------------------------------------------------------------ forward / adjoint
@pytest.mark.parametrize(**cases_of('kappa_ladder'))
def test_kappa_ladder(ctx, p):
    """Reaches: ctf_c1, ctf_c2, ctf_c3, ctf_c4, ctf_c5, ctf_sums_kernel (both stage_inv_kappa sites, ctf_osc, the scale of ctf_sum_one).
    lg_kappa -0.5 ... 30, the object scaled to keep I in range: every output against the reference.  lg_kappa = 50: 1 / kappa is 0.0f;
    dL/dlg_kappa is finite and below 1e-37, everything else is judged as before."""
    c = V.case(*p)
    res = both(ctx, c)
    referenced(res, c, p)
    if p[2]['lg_kappa'] == V.KAPPA_ZERO:
        for entry, r in res.items():
            print('%s, %s: grad_lg_kappa %r' % (c['name'], entry, r['g_kappa'][0]))
            assert np.isfinite(r['g_kappa']).all() and abs(float(r['g_kappa'][0])) < V.GKAPPA_TINY, (c['name'], entry, r['g_kappa'])


@pytest.mark.parametrize(**cases_of('contrast'))
def test_contrast(ctx, p):
    """Reaches: ctf_c1, ctf_c2, ctf_c3, ctf_c4, ctf_c5, ctf_sums_kernel.  The object x 3 and x 10: min I 0.8 and 0.37."""
    c = V.case(*p)
    referenced(both(ctx, c), c, p)


@pytest.mark.parametrize(**cases_of('low_I'))
def test_low_I(ctx, p):
    """Reaches: ctf_c1, ctf_c2, ctf_c3, ctf_c4, ctf_c5, ctf_sums_kernel (the division by the prediction in C3).  min I = 0.05 ... the lowest rung the
    one-third rule admits for the field; every prediction is positive."""
    c = V.case(*p)
    res = both(ctx, c)
    referenced(res, c, p)
    for entry, r in res.items():
        assert (r['pred'] > 0).all(), (c['name'], entry)


@pytest.mark.parametrize(**cases_of('crossing_zero'))
def test_crossing_zero(ctx, p):
    """Reaches: ctf_c1, ctf_c2, ctf_c3, ctf_c4, ctf_c5, ctf_sums_kernel (C3's I > 0 guards of the prediction and of q).  The object x 20 and x 30: I
    passes through 0 without a gap; prediction and loss by ctf_value_matrix.judge_crossing, every gradient finite.  The gapped clip
    case of ctf_matrix: the prediction is +0 on the clipped pixels and every gradient, dL/dd and dL/dlg_kappa of the device
    entry included, equals the reference's, which drops them."""
    c = V.case(*p)
    res = both(ctx, c)
    finite(res, c['name'])
    if p[2].get('clip'):
        neg = c['o64']['I'] <= 0
        for entry, r in res.items():
            assert not CM.bits(r['pred'][neg]).any() and (r['pred'][~neg] > 0).all(), (c['name'], entry)
        referenced(res, c, p)
        return
    for entry, r in res.items():
        f = V.judge_crossing(r['pred'], r['loss'], c)
        f32 = V.judge_crossing(c['o32' if entry == 'device' else 'o32h']['pred'], c['o32' if entry == 'device' else 'o32h']['loss'], c)
        print('%s, %s: %d pixels clipped, %d within tol %.1e; pred %.2e (fp32 restatement %.2e)  loss %.2e (%.2e, bar %.1e)' % (
            c['name'], entry, f['clipped'], f['within_tol'], f['tol'], f['pred'], f32['pred'], f['loss'], f32['loss'], f['loss_bar']))


@pytest.mark.parametrize(**cases_of('distances'))
def test_distances(ctx, p):
    """Reaches: ctf_c1, ctf_c2, ctf_c3, ctf_c4, ctf_c5, ctf_sums_kernel (ctf_c_of and ctf_sincos at small, zero and negative arguments).  The
    distances x 1e-3 ... 0.1; one distance exactly 0, whose prediction is sqrt(1 + 2 D / kappa) pixel by pixel; one negative."""
    c = V.case(*p)
    res = both(ctx, c)
    referenced(res, c, p)
    if p[2]['kind'] == 'zero':
        want = V.closed_form_at_zero_distance(c)
        for entry, r in res.items():
            e = float(np.abs(r['pred'][1] / want - 1).max())
            print('%s, %s: distance 0 against the closed form, worst pixel %.2e' % (c['name'], entry, e))
            assert e < BARS['pred'], (c['name'], entry, e)


@pytest.mark.parametrize(**cases_of('physical_scales'))
def test_physical_scales(ctx, p):
    """Reaches: ctf_c1, ctf_c2, ctf_c3, ctf_c4, ctf_c5, ctf_sums_kernel (the host's c[d], pil, dscale and the u^2 + v^2 upload).  500 eV at 50 nm,
    17.05 keV at 5 nm, 100 keV at 6.5 um, the distances rescaled to the table's xi: dL/dd moves by many decades."""
    c = V.case(*p)
    res = both(ctx, c)
    referenced(res, c, p)
    print('%s: distances %s cm, dL/dd %s' % (c['name'], c['model_dists'], res['device']['g_dists']))


@pytest.mark.parametrize(**cases_of('data'))
def test_data(ctx, p):
    """Reaches: ctf_c1, ctf_c2, ctf_c3, ctf_c4, ctf_c5, ctf_sums_kernel (C3's fabsf and sqrtf of the measured value).  Exact zeros, a third of the
    values negated (no output bit changes against the launch without the signs), x 1e4, x the smallest admitted scale; intensity
    and magnitude.  The prediction has the bits of the unedited intensity launch throughout."""
    c = V.case(*p)
    res = both(ctx, c)
    referenced(res, c, p)
    equal_outputs(res, plain(ctx, p[1]), c['name'] + ': the prediction depends on the data', keys=('pred',))
    if p[2]['kind'] == 'negated':
        assert (c['data'] < 0).mean() > 0.25
        equal_outputs(res, both(ctx, c, data=c['plain_data']), c['name'] + ': the signs of the data reach the result')


@pytest.mark.parametrize(**cases_of('exact'))
def test_exact(ctx, p):
    """Reaches: ctf_c1, ctf_c2, ctf_c3, ctf_c4, ctf_c5, ctf_sums_kernel (C1 reads delta alone).  Object 0: every prediction is exactly 1.0f; with data 1
    every loss sum is +0 and every gradient +-0, with the table's data the delta gradient equals the reference's and dL/dlg_kappa
    and dL/dd are +-0 (F = 0).  Beta 1e30, Inf, NaN: every output has the bits it has with the table's beta."""
    c = V.case(*p)
    kind = p[2]['kind']
    res = both(ctx, c)
    if kind in V.BETA:
        referenced(res, c, p)
        equal_outputs(res, plain(ctx, p[1]), c['name'] + ': beta reaches the result')
        return
    one = np.ones_like(c['data'])
    for entry, r in res.items():
        same_bits(r['pred'], one, (c['name'], entry, 'prediction of a zero object'))
        for k in ('g_kappa', 'g_dists'):
            if k in r:
                assert (r[k] == 0).all(), (c['name'], entry, k, r[k])
        if kind == 'zero_object_unit_data':
            assert not CM.bits(r['loss_d']).any(), (c['name'], entry, r['loss_d'])
            assert (r['g_obj'] == 0).all(), (c['name'], entry)
    if kind == 'zero_object':
        referenced(res, c, p)


@pytest.mark.parametrize(**cases_of('nonfinite_data'))
def test_nonfinite_data(ctx, p):
    """Reaches: ctf_c1, ctf_c2, ctf_c3, ctf_c4, ctf_c5, ctf_sums_kernel (C3's blocks hold rows of several distances; ctf_sum_one per distance).  One NaN
    and one Inf in the data of distance 1: the call returns ADM_OK, the prediction and the loss sums of the other distances have
    the bits of the clean launch, loss_sum[1] is not finite."""
    c = V.case(*p)
    dirty, clean = both(ctx, c), both(ctx, c, data=c['plain_data'])          # (a return code other than ADM_OK raises)
    assert not np.isfinite(c['data'][1]).all() and np.isfinite(np.delete(c['data'], 1, 0)).all()
    for entry in dirty:
        same_bits(dirty[entry]['pred'], clean[entry]['pred'], (c['name'], entry, 'prediction'))
        others = [d for d in range(c['nd']) if d != 1]
        same_bits(dirty[entry]['loss_d'][others], clean[entry]['loss_d'][others], (c['name'], entry, 'loss sums of the clean distances'))
        assert not np.isfinite(dirty[entry]['loss_d'][1]), (c['name'], entry, dirty[entry]['loss_d'])
        print('%s, %s: loss sums %s (clean %s)' % (c['name'], entry, dirty[entry]['loss_d'], clean[entry]['loss_d']))


# ------------------------------------------------------------------------------------------------------------ the inversion
def inv_judged(A, ctx, p):
    c = V.inv_case(*p)
    phase = run(A, ctx, c)['phase']
    o, s = np.asarray(c['o64']).reshape(phase.shape), np.asarray(c['o32']).reshape(phase.shape)
    assert np.isfinite(phase).all(), c['name']
    e, e32 = V.rel(phase, o), V.rel(s, o)
    print('%s: phase %.2e (fp32 restatement %.2e, bar %.2e); max |phase| %.3g' % (c['name'], e, e32, c['bar'], np.abs(o).max()))
    assert e <= c['bar'], (c['name'], e, e32, c['bar'])
    return c, phase


@pytest.mark.parametrize(**inv_cases_of('inv_kappa_ladder'))
def test_inv_kappa_ladder(A, ctx, p):
    """Reaches: ctfinv_i1, ctfinv_i2, ctfinv_i3 (I2's stage_inv_kappa and w).  lg_kappa -0.5 ... 50 on 32 x 16 x 2 and 16 x 32 x 2."""
    inv_judged(A, ctx, p)


@pytest.mark.parametrize(**inv_cases_of('inv_alpha_ladder'))
def test_inv_alpha_ladder(A, ctx, p):
    """Reaches: ctfinv_i1, ctfinv_i2, ctfinv_i3 (I2's quotient num / (den + alpha)).  Constant alpha 1e-30 ... 1e6: from nothing beside
    2 w^2 to all of the denominator (the phase shrinks to 1e-7), judged relative to the array."""
    inv_judged(A, ctx, p)


@pytest.mark.parametrize(**inv_cases_of('inv_data'))
def test_inv_data(A, ctx, p):
    """Reaches: ctfinv_i1, ctfinv_i2, ctfinv_i3 (I1 uses the data as given).  The contrast about 1 x 1e4 (the phase reaches 625 rad);
    exact zeros and negated values (a stray fabs moves the result by O(1))."""
    inv_judged(A, ctx, p)


def test_inv_nonfinite_batch_entry(A, ctx):
    """Reaches: ctfinv_i1, ctfinv_i2, ctfinv_i3 (I1's blocks hold rows of several batch entries; only the stores separate them).  A NaN
    and an Inf in the holograms of angle 1 of 3, one launch group: angles 0 and 2 have the bits of the clean launch."""
    c = V.inv_nonfinite()
    assert V.IM.geometry(c['ny'], c['nx'], c['nd'], c['nb'])['i1_spans_batch'][0]
    eng = engine(A, ctx, c)
    clean, dirty = run(A, ctx, c, eng, data=c['plain_data'])['phase'], run(A, ctx, c, eng)['phase']
    assert np.isfinite(clean).all() and not np.isfinite(dirty[1]).all()
    for b in (0, 2):
        same_bits(dirty[b], clean[b], 'angle %d beside a non-finite angle 1' % b)
