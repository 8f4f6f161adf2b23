"""The multislice kernels over the VALUE domain (pytest -m gpu): strong, absorbing and amplifying objects through both paths of
modulate<>, gen_modulator and slice_transmission; shifts of tens of pixels through the three fp32 shift phases; invalid numbers
under the detector mask.  tests/value_matrix.py holds the classes and cases, tests/test_value_domain_coverage.py ties them to
the kernel sources and shows on the CPU that every case leaves room under its cap.

Bars: ms_matrix.check with the caps of the path (TUNED / GENERIC) and the 3x rule against the fp32 oracle, unchanged; bit
equality where the code promises it (cached against in-loop transmissions; clean data against dirt under the mask); finite
outputs everywhere.
"""
import functools

import numpy as np
import pytest

from tests import ms_matrix as MM
from tests import value_matrix as VM

pytestmark = pytest.mark.gpu
THETA = 0.7


@pytest.fixture(scope='module')
def A():
    import adorym_amd
    return adorym_amd


@pytest.fixture(scope='module')
def ctx(A):
    c = A.Context(0)
    yield c
    c.close()


_CASES = {}


def object_case(P, cls, M=1, sg=None, unknown_type='delta_beta'):
    """oracle_case of an object class, built once per module and left unchanged (VM.run copies the dict)."""
    key = (P, cls, M, sg, unknown_type)
    if key not in _CASES:
        with np.errstate(all='ignore'):
            _CASES[key] = MM.oracle_case(P, **VM.object_case_kw(cls, P, M, sg, unknown_type))
    return _CASES[key]


def _id(v):
    return str(v).replace(' ', '')


def report(res, what):
    print('%s: pred %.2e (fp32 oracle %.2e)  loss %.2e  grad %.2e (%.2e)  gprobe %.2e (%.2e)' % (
        what, MM.rel(res['pred'], res['pred_o']), MM.rel(res['pred_32'], res['pred_o']), abs(res['loss'] / res['loss_o'] - 1),
        MM.rel(res['grad'], res['grad_o']), MM.rel(res['grad_32'], res['grad_o']),
        MM.rel(res['gprobe'], res['gprobe_o']), MM.rel(res['gprobe_32'], res['gprobe_o'])))


def assert_finite(res, what, where=None):
    fin = VM.all_finite(res, where=where)
    assert all(fin.values()), (what, fin)
    assert np.isfinite(res['loss']), (what, res['loss'])


# ------------------------------------------------------------------------------------------------------------ A. objects
@pytest.mark.parametrize('ev,P,cls,M,sg', VM.object_cases(), ids=_id)
def test_object_classes_in_loop_vs_oracle(A, ctx, ev, P, cls, M, sg):
    """Every class through the in-loop modulation (transmission_cache=False): modulate<> of the tuned kernels, gen_modulator of the
    generic and the streamed kernels.  Bars 1 and 4."""
    res = VM.run(A, ctx, object_case(P, cls, M, sg), ev, cache=0)
    report(res, '%s %s %s' % (ev, P, cls))
    assert_finite(res, cls)
    MM.check(res, VM.bars_of(ev))


BIT_FIELDS = [('tuned', P) for P in VM.TUNED_SIZES] + [('generic', VM.GENERIC_FIELD), ('streamed', VM.STREAMED_FIELDS[0])]
BIT_CASES = [(ev, P, cls, M) for cls in VM.OBJECT_CLASSES for ev, P in BIT_FIELDS
             for M in ((1, 3) if cls in VM.MODES_CLASSES and ev == 'tuned' and P != 27 else (1,))]


@pytest.mark.parametrize('ev,P,cls,M', BIT_CASES, ids=_id)
def test_cached_transmissions_give_the_in_loop_bits(A, ctx, ev, P, cls, M):
    """slice_transmission stored by the rotation (cache modes 1 and 2; the identity kernel with coords = NULL, rotate_fwd_kernel at
    an angle; adm_transmission_refresh) against the in-loop evaluation: prediction, per-position loss sums, rotated-frame and
    object gradient, probe gradient equal bit for bit and finite; the cached run at coords = NULL also meets the oracle's bars.
    Bars 1, 3 and 4."""
    sg = VM.SIGMA_OF.get(cls, 1)
    case = object_case(P, cls, M, sg)
    for theta in (None, THETA):
        base = VM.run(A, ctx, case, ev, cache=0, theta=theta)
        assert_finite(base, (cls, theta))
        assert np.abs(base['grad']).max() > 0 and np.abs(base['gprobe_raw']).max() > 0
        runs = [('mode 1', dict(cache=1)), ('mode 2', dict(cache=2))] + ([('refresh', dict(cache=1, refresh=True))] if theta else [])
        for name, kw in runs:
            res = VM.run(A, ctx, case, ev, theta=theta, **kw)
            d = VM.bits_differ(base, res)
            print(cls, ev, P, M, 'theta', theta, name, 'words that differ', d)
            assert not any(d.values()), (cls, theta, name, d)
            if theta is None and name == 'mode 1':
                MM.check(res, VM.bars_of(ev))


@pytest.mark.parametrize('ev,P,cache', [('tuned', 32, 0), ('tuned', 32, 1), ('tuned', 27, 0), ('generic', (40, 24), 0), ('streamed', (24, 24), 0)], ids=_id)
def test_exp_fast_on_the_device(A, ctx, ev, P, cache):
    """exp_fast itself, through modulate<>, gen_modulator and slice_transmission: S = 1, exit wave, probe 1 + 0i, delta = 0, so
    pred = |exp_fast(-k1 beta)| for k1 beta over [-3, 40].  Bar, in float32 ulps of exp of the kernel's own fp32 argument evaluated
    in fp64: the mirror's measured 1.0 (tests/test_value_domain_coverage.py) + 1 for v_exp_f32 (a 1-ulp instruction, which the
    mirror replaces by the exact 2^t) + 1 for the magnitude sqrt(fl(e * e)) that the prediction takes of it = 3.0."""
    case = MM.oracle_case(P, S=1, B=6, free_prop=0, obj_fn=VM.exp_ramp_fn, probe_edit=lambda p: np.ones_like(p))
    res = VM.run(A, ctx, case, ev, cache=cache)
    Py, Px = case['kw']['shape']
    tiles, _ = MM.O.extract_tiles(case['obj'], case['pos'], (Py, Px), 'delta_beta')
    x32 = -(VM.K1F * tiles[:, :, :, 0, 1].astype(np.float32))                   # the kernel's argument, one fp32 product
    assert x32.min() < -39 and x32.max() > 2.9
    ref = np.exp(x32.astype(np.float64))
    u = VM.ulps(res['pred'], ref)
    m = VM.ulps(VM.exp_fast_mirror(x32), ref)
    print('exp_fast on the device: worst %.3f ulp at x = %.4f (mirror %.3f ulp); beyond 2 ulp: %d of %d' % (
        u.max(), x32.ravel()[u.argmax()], m.max(), (u > 2).sum(), u.size))
    assert u.max() <= 3.0


CONTROL_CASES = [(ev, P, cls) for cls in VM.OBJECT_CLASSES for ev, P in VM.CONTROL_FIELDS]


@pytest.mark.parametrize('ev,P,cls', CONTROL_CASES, ids=_id)
def test_real_imag_control(A, ctx, ev, P, cls):
    """The control: the same numbers as (re, im) of a real_imag plan, where no transcendental is evaluated."""
    res = VM.run(A, ctx, object_case(P, cls, 1, 1, 'real_imag'), ev)
    report(res, 'real_imag %s %s %s' % (ev, P, cls))
    assert_finite(res, cls)
    MM.check(res, VM.bars_of(ev))


# ------------------------------------------------------------------------------------------------------------ C. large shifts
@functools.lru_cache(maxsize=None)
def shift_case(P, **kw):
    return MM.oracle_case(P, pp='shifts', shifts_fn=lambda n: VM.large_shifts(P, n), **kw)


@pytest.mark.parametrize('cache', [True, False], ids=['cached', 'in_loop'])
@pytest.mark.parametrize('M', [1, 3])
@pytest.mark.parametrize('P', [8, 32])
def test_large_shifts_tuned(A, ctx, P, M, cache):
    """shift_phases of adm_multislice.hip (adm_probe_shift, adm_probe_shift_adj) at +-7.3, +-(P/2 - 0.25) and +-(P + 3.6) px."""
    case = dict(shift_case(P, S=3, B=10, n_modes=M, transmission_cache=cache))
    res = MM.run_engine(A, ctx, case)
    report(res, 'tuned shifts %d' % P)
    print('dL/ds %.2e (fp32 oracle %.2e)' % (MM.rel(res['gshift'], res['gshift_o']), MM.rel(res['gshift_32'], res['gshift_o'])))
    MM.check(res, MM.TUNED)


@pytest.mark.parametrize('P', VM.STREAMED_FIELDS, ids=_id)
def test_large_shifts_streamed_probe_shift(A, ctx, P):
    """st_shift_phase (adm_ms_col.h) in adm_ms_probeshift.hip at the same shifts, by test_gpu_streamed_probe_shift's checks."""
    from tests import test_gpu_streamed_probe_shift as PS
    res = PS.run_ps(A, ctx, shift_case(P, S=2, B=6), canaries=True)
    PS.report_and_check(res, 'streamed shifts %s' % (P,))


@pytest.mark.parametrize('free_prop', ['fresnel', 0], ids=['fresnel', 'exit_wave'])
@pytest.mark.parametrize('P', [(24, 20), (640, 12)], ids=_id)
def test_large_shifts_exit_wave(A, ctx, P, free_prop):
    """st_shift_phase (adm_ms_col.h) in adm_ms_exitshift.hip at the same shifts: check_3x / gs_bar of test_gpu_prj_offset with prj_offset_ref, which
    forms its fp32 argument in fp32 as the reference does, as the yardstick."""
    from tests import test_gpu_prj_offset as PO
    fp = PO.FREE_PROP_CM if free_prop == 'fresnel' else 0
    case = PO.make_case(P, free_prop=fp, shifts_fn=lambda n: VM.large_shifts(P, n))
    r64, e32 = PO.yardstick(case)
    res = PO.run_shifted(A, ctx, case, canaries=True)
    PO.check_3x(res, r64, e32, 'exit shifts %s %s' % (P, free_prop))


# ------------------------------------------------------------------------------------------------------------ D. the mask
@functools.lru_cache(maxsize=None)
def mask_case(P, variant):
    return MM.oracle_case(P, beamstop=VM.value_beamstop(P), **dict(VM.OBJ_KW, **VM.MASK_VARIANTS[variant]))


@pytest.mark.parametrize('ev,P,variant', VM.MASK_CASES, ids=_id)
def test_masked_pixels_are_dropped(A, ctx, ev, P, variant):
    """A disc, one whole row and one isolated pixel under the mask.  With NaN, +inf, -1, 0 and 3e38 there instead of model data:
    loss, per-position loss sums, prediction at the kept pixels, object and probe gradient are the clean run's bit for bit, and
    finite; the clean run meets the oracle's bars."""
    case = mask_case(P, variant)
    keep = case['beamstop'] >= 1e-5
    clean = VM.run(A, ctx, case, ev)
    report(clean, 'mask %s %s %s' % (ev, P, variant))
    MM.check(clean, VM.bars_of(ev))
    target = VM.dirty(case['target'], case['beamstop'])
    assert not np.isfinite(target[:, ~keep]).all() and np.array_equal(target[:, keep], case['target'][:, keep])
    dirt = VM.run(A, ctx, case, ev, target=target)
    d = VM.bits_differ(clean, dirt, where=keep)
    print('words that differ', d, 'loss', clean['loss'], dirt['loss'])
    assert_finite(dirt, variant, where=keep)
    assert np.isfinite(dirt['pred']).all()                    # (pred at a masked pixel stays the predicted magnitude)
    assert not any(d.values()), d
    assert np.array_equal(np.float64(clean['loss']), np.float64(dirt['loss']))
    assert VM.bits_differ(clean, dirt, keys=('pred',))['pred'] == 0


def _disc_probe(probes):
    Py, Px = probes.shape[-2:]
    yy, xx = np.meshgrid(np.arange(Py) - Py / 2 + 0.5, np.arange(Px) - Px / 2 + 0.5, indexing='ij')
    return probes * (yy ** 2 + xx ** 2 < (0.3 * min(Py, Px)) ** 2)


ZERO_FIELDS = (('tuned', 8), ('tuned', 27), ('generic', (40, 24)), ('streamed', (24, 24)))


@pytest.mark.parametrize('ev,P', ZERO_FIELDS, ids=_id)
def test_exactly_zero_prediction(A, ctx, ev, P):
    """S = 1, exit-wave detector, one mode, a probe that is exactly 0 outside a disc: pred == 0 exactly there.  Unmasked under
    LSQ the `mag > 0` guard of loss_term makes the gradient factor 0: finite, and the oracle's bars hold.  With those pixels
    under a mask the result is finite, and the oracle's, under both losses (the Poisson term there is 0 * log 0)."""
    kw = dict(S=1, B=6, free_prop=0, probe_edit=_disc_probe)
    case = MM.oracle_case(P, **kw)
    zero = np.abs(case['probes'][0]) == 0
    assert 0.3 < zero.mean() < 0.9
    res = VM.run(A, ctx, case, ev)
    assert (res['pred'][:, zero] == 0).all() and (res['pred'][:, ~zero] > 0).all()
    assert_finite(res, 'unmasked lsq')
    MM.check(res, VM.bars_of(ev))
    for loss_kw in (dict(), dict(loss='poisson', raw_data_type='intensity', poisson_multiplier=50.)):
        with np.errstate(all='ignore'):
            masked = MM.oracle_case(P, beamstop=np.where(zero, 0., 1.), **dict(kw, **loss_kw))
        res = VM.run(A, ctx, masked, ev)
        assert (res['pred'][:, zero] == 0).all()
        assert_finite(res, ('masked', loss_kw))
        MM.check(res, VM.bars_of(ev))


def test_driver_drops_masked_pixels(A, tmp_path):
    """reconstruct_ptychography(beamstop=...): two epochs on clean data and on data with NaN, inf, -1, 0 and 3e38 under the mask
    end in the same object and the same losses, bit for bit."""
    from oracle import adorym_oracle as O      # makes the data only
    r = np.random.default_rng(5)
    N, P = 40, 16
    pos = np.array([(y, x) for y in range(-2, 28, 6) for x in range(-2, 28, 6)], dtype=float)
    obj = np.stack([2e-3 * r.uniform(size=(N, N, 1)), 2e-4 * r.uniform(size=(N, N, 1))], -1)
    probe = (0.5 + r.uniform(0, 1, (P, P))) * np.exp(1j * r.uniform(-1, 1, (P, P)))
    tiles, _ = O.extract_tiles(obj, pos.astype(int), (P, P))
    prj = O.predict(tiles, probe, O.Physics((P, P), 5000., 1e-7))[0][None].astype(np.float32)
    bs = VM.value_beamstop(P).astype(np.float32)
    states = []
    guess = [np.full((N, N, 1), 1e-3), np.full((N, N, 1), 1e-4)]
    for k, data in enumerate((prj, VM.dirty(prj[0], bs)[None].astype(np.float32))):
        np.random.seed(123)                                   # (whatever the driver draws, it draws the same twice)
        st = A.reconstruct_ptychography(
            fname=data, probe_pos=pos, theta_st=0, theta_end=0, n_epochs=2, obj_size=(N, N, 1), two_d_mode=True, energy_ev=5000.,
            psize_cm=1e-7, minibatch_size=10, output_folder='run%d' % k, save_path=str(tmp_path), use_checkpoint=False,
            n_epoch_final_pass=None, save_intermediate=False, initial_guess=guess,
            probe_type='supplied', probe_initial=[np.abs(probe), np.angle(probe)], free_prop_cm='inf',
            raw_data_type='magnitude', beamstop=bs, optimizer='adam', learning_rate=1e-4, update_scheme='immediate',
            loss_function_type='lsq', randomize_probe_pos=False, return_state=True)
        states.append(st)
    assert not np.isfinite(VM.dirty(prj[0], bs)).all()
    for k in ('delta', 'beta'):
        a, b = np.ascontiguousarray(states[0][k], np.float32), np.ascontiguousarray(states[1][k], np.float32)
        assert np.isfinite(b).all() and np.abs(b).max() > 0
        assert np.array_equal(a.view(np.uint32), b.view(np.uint32)), k
    assert np.isfinite(states[1]['losses']).all() and np.array_equal(np.asarray(states[0]['losses']), np.asarray(states[1]['losses']))
