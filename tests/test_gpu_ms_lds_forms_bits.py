"""
The one-workgroup multislice kernels (adm_multislice.hip) bit for bit against digests recorded with an earlier build.

How the LDS field exchanges of these kernels are issued (single or merged DS instructions, compiler- or hand-placed waits:
DESIGN.md section 4) must not change a single bit of what they compute: same addresses, same arithmetic, same order.  A wait
that is too weak reads a register before its LDS value has arrived, and shows at the sizes whose passes have the fewest
instructions between a read and its use (radix 2: sizes 8 and 18) -- hence every compiled size, one launch each:

  * 3 slices (the dithered butterfly constants of two propagations and the nominal ones), 2 positions, the first in the frame's
    corner so that the padded border is read, far field;
  * MODE 2 (cached slice transmissions) and MODE 0 with binning 2;
  * at 72 and 64 also two probe modes (MULTI) and one probe set per position (PP, through sub-pixel probe shifts, which also
    runs the probe-shift kernels of the same translation unit).

Compared: SHA-256 of the raw bytes of the per-position loss sums, the predicted magnitudes, the tile-gradient rows and the
probe-gradient slots (the workspace is zeroed before the launch, so rows of inactive threads are defined), and of the whole
workspace (stored wavefields included).  No tolerance.  tests/golden/ms_lds_forms_bits.json is written by
tools/record_ms_bits.py and names the commit and the ROCm version that wrote it.
"""
import hashlib
import json
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

SIZES = (8, 12, 16, 18, 24, 27, 32, 36, 64, 72)          # ADM_FOR_EACH_SIZE of adm_multislice.hip
KINDS = ('mode2', 'mode0_bin2')
EXTRA = ('multi', 'pp')                                    # at 72 and 64 only
CASES = [(n, k) for n in SIZES for k in KINDS] + [(n, k) for n in (64, 72) for k in EXTRA]
FIXTURE = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden', 'ms_lds_forms_bits.json')
ENERGY_EV, PSIZE_CM, SLICES = 5000., 1.e-7, 3
POS = np.array([(-3, -2), (5, 4)])


def case_id(n, kind):
    return '%d-%s' % (n, kind)


def _sha(a):
    return hashlib.sha256(np.ascontiguousarray(a).tobytes()).hexdigest()


def _inputs(n, modes):
    from adorym_amd import workloads as W
    shape = (n + 8, n + 8, SLICES)
    obj = W.random_guess(shape, seed=n)
    probe = W.probe_array(dict(probe_size=(n, n), probe=W.c3_config()['probe']))
    probes = np.stack([probe * (0.5 ** m) if m == 0 else np.roll(probe, (m, 2 * m), (0, 1)) * (0.5 ** m) for m in range(modes)])
    target = np.abs(np.random.default_rng(n).standard_normal((len(POS), n, n))).astype(np.float32) * 30
    return shape, obj, np.ascontiguousarray(probes, np.float32), target


def run_case(A, ctx, n, kind):
    """One forward + adjoint launch; {name: sha256 of the raw bytes}."""
    modes = 2 if kind == 'multi' else 1
    shape, obj, probes, target = _inputs(n, modes)
    B = len(POS)
    eng = A.MultisliceEngine(ctx, shape, (n, n), POS, ENERGY_EV, PSIZE_CM, free_prop_cm='inf', binning=2 if kind == 'mode0_bin2' else 1,
                             n_probe_modes=modes, max_batch=B)
    assert not eng.streamed and eng.transmission_cache == (kind != 'mode0_bin2')
    d_probe, g_probe = ctx.array(probes), ctx.zeros(probes.shape)
    eng.set_batch(POS, target)
    eng.rotate(ctx.array(obj), None)
    ws = eng._ws
    A._lib.check(ctx.lib.adm_memset(ctx.handle, ws.ptr, 0, ws.nbytes))
    out = {}
    if kind == 'pp':
        shifts = ctx.array(np.array([(0.25, -0.375), (-0.5, 0.125)], np.float32))
        g_shifts = ctx.zeros((B, 2))
        eng.multislice(d_probe, grad_probe=g_probe, want_pred=True, accumulate=False, shifts=shifts, grad_shifts=g_shifts)
        out['probes_b'] = _sha(eng._probes_b.get())
        out['probe_grad_slots'] = _sha(eng._gprobes_b.get())
        out['grad_shifts'] = _sha(g_shifts.get())
    else:
        eng.multislice(d_probe, grad_probe=g_probe, want_pred=True, accumulate=False)
    ctx.sync()
    raw = ws.get()
    # ws_layout (adm_api.hip): stored wavefields [B][M][rows], tile gradients [B][rows], cover lists, ..., probe-gradient slots last
    total = eng.plan.workspace_bytes(B)
    per = eng.plan.workspace_bytes(2) - eng.plan.workspace_bytes(1)
    fld = n * n * 8
    if modes > 1:                                         # (several modes park detector-plane fields too: take the rows from one mode)
        one = A.MultisliceEngine(ctx, shape, (n, n), POS, ENERGY_EV, PSIZE_CM, free_prop_cm='inf', max_batch=1).plan
        per = one.workspace_bytes(2) - one.workspace_bytes(1)
    rows = (per - fld) // 2                               # one position, one mode: stored wavefields + tile gradients + probe-gradient slot
    assert total <= raw.nbytes and rows > 0 and rows % 8 == 0 and 2 * rows + fld == per
    out['loss_sums'] = _sha(eng._loss.view(0, (B,)).get())
    out['pred'] = _sha(eng.pred())
    out['tile_grad_rows'] = _sha(raw[B * modes * rows:B * (modes + 1) * rows])
    if kind != 'pp':
        out['probe_grad_slots'] = _sha(raw[total - B * modes * fld:total])
    out['probe_grad'] = _sha(g_probe.get())
    out['workspace'] = _sha(raw[:total])
    assert np.isfinite(eng.pred()).all(), 'prediction not finite'
    assert np.any(raw[B * modes * rows:B * (modes + 1) * rows]), 'tile-gradient rows all zero'
    return out


@pytest.fixture(scope='module')
def A():
    import adorym_amd
    return adorym_amd


@pytest.fixture(scope='module')
def ctx(A):
    c = A.Context(0)
    yield c
    c.close()


@pytest.fixture(scope='module')
def recorded():
    with open(FIXTURE) as f:
        return json.load(f)


def test_fixture_names_its_origin_and_every_case(recorded):
    assert recorded['written_by']['commit'] and recorded['written_by']['rocm']
    assert sorted(recorded['digests']) == sorted(case_id(n, k) for n, k in CASES)


@pytest.mark.parametrize('n,kind', CASES, ids=[case_id(n, k) for n, k in CASES])
def test_multislice_bits_are_the_recorded_ones(A, ctx, recorded, n, kind):
    got = run_case(A, ctx, n, kind)
    want = recorded['digests'][case_id(n, kind)]
    assert sorted(got) == sorted(want)
    differ = [k for k in sorted(got) if got[k] != want[k]]
    assert not differ, 'P = %d, %s: bits differ from the recorded build in %s' % (n, kind, ', '.join(differ))
