"""
The column kernels of the streamed multislice path bit for bit against digests recorded with an earlier build (pytest -m gpu).

The column kernels (adm_ms_streamed.hip, adm_ms_exitshift.hip, adm_ms_probeshift.hip, adm_ms_multidist.hip) share their prologue,
their launch line, the shift phase, the Fresnel table and the fixed-order reduce of the distance partials (adm_ms_col.h); the fan-out
and fan-in kernels are one template each, with and without the distance gradient.  Stating a piece once must not change a single
bit of what any of them computes: every sum on this path has a fixed order and no atomics.  One launch per case, seeded inputs, the
field 24 x 20 (three column groups, the last clipped to 4 columns) unless the case says otherwise:

  fresnel        S = 3, B = 3, M = 2, Fresnel detector           st_col_conv_kernel, st_det_kernel
  farfield       S = 2, B = 3, M = 2, far field
  sparse_gz      S = 4 uneven slice positions, B = 3, M = 2, grad_slice_pos     st_fresnel_table_kernel (gaps), st_col_conv_sparse_kernel,
                                                                                st_dd_reduce_kernel (gaps)
  exit_shift     B = 4, index [0, 1, 0, 2], M = 2, shifts up to 2.5 px, grad_exit_shifts      es_col_conv_kernel
  probe_shift    the same index and shifts on the probe-shift plan, grad_shifts               ps_colfft_kernel, ps_col_kernel
  fan_host       D = 3 host-built kernels, B = 2, M = 2                          md_fanout_kernel<false>, md_fanin_kernel<false>
  fan_dev        the same distances with refine_distances, no gradient requested        st_fresnel_table_kernel (distances)
  fan_grad       the same with grad_dists, launched twice into the same buffer (+=)     md_fanout_kernel<true>, md_fanin_kernel<true>,
                                                                                        st_dd_reduce_kernel (distances)
  fan_grad_tall  field 1025 x 12 (cw = 4, three groups), D = 2, B = 1, M = 1, grad_dists

Compared: SHA-256 of the raw bytes of the loss sums, the predictions, the object gradient as the engine hands it back (grad_rot,
overlap-added), the probe gradient, and grad_slice_pos / grad_shifts / grad_dists where the case has them.  No tolerance.
tests/golden/streamed_col_bits.json is written by tools/record_ms_bits.py --module test_gpu_streamed_col_bits and names the commit
and the ROCm version that wrote it.

Within the run: fan_dev and fan_grad give the same bits on every output they share (the request for dL/dd changes no other bit), and
both agree with fan_host on every shared output under the bars of tests/ms_matrix.py:GENERIC -- the host table is exp(i a d) in
fp64 rounded once, the device table the same phase reduced in fp64 and then sincosf, so the two differ by a few fp32 roundings per
element, far inside the bars that hold either engine to the fp64 model (test_gpu_multidist3d_dist.py states the same for its shapes).
"""
import hashlib
import json
import os

import numpy as np
import pytest

from tests import ms_matrix as MM

pytestmark = pytest.mark.gpu

CASES = ('fresnel', 'farfield', 'sparse_gz', 'exit_shift', 'probe_shift', 'fan_host', 'fan_dev', 'fan_grad', 'fan_grad_tall')
FIXTURE = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden', 'streamed_col_bits.json')
ENERGY_EV, PSIZE_CM = 8000., 1e-6
FIELD, TALL = (24, 20), (1025, 12)
POS = np.array([(-3, -2), (5, 4), (2, -1), (0, 6)])              # over the object's edges: the padded border is read
INDEX = np.array([0, 1, 0, 2], np.int32)
SHIFTS = np.array([(2.5, -1.25), (-0.375, 0.5), (0.0625, 2.5)], np.float32)
SLICE_POS_CM = [0., 1e-4, 2.5e-4, 6e-4]
DISTS_CM = [1e-4, 2e-4, 3.5e-4]
BARS = MM.GENERIC
SHARED = ('loss_sums', 'pred', 'obj_grad', 'probe_grad')
#   name: field, slices, positions, modes, detector entries per position, engine arguments
SPECS = {
    'fresnel': (FIELD, 3, 3, 2, 1, dict(free_prop_cm=2e-4)),
    'farfield': (FIELD, 2, 3, 2, 1, dict(free_prop_cm='inf')),
    'sparse_gz': (FIELD, 4, 3, 2, 1, dict(free_prop_cm=2e-4, slice_pos_cm=SLICE_POS_CM)),
    'exit_shift': (FIELD, 2, 4, 2, 1, dict(free_prop_cm=2e-4, exit_shift=True)),
    'probe_shift': (FIELD, 2, 4, 2, 1, dict(free_prop_cm=2e-4, probe_shift=True)),
    'fan_host': (FIELD, 2, 2, 2, 3, dict(free_prop_cm=DISTS_CM, detector_fanout=True)),
    'fan_dev': (FIELD, 2, 2, 2, 3, dict(free_prop_cm=DISTS_CM, detector_fanout=True, refine_distances=True)),
    'fan_grad': (FIELD, 2, 2, 2, 3, dict(free_prop_cm=DISTS_CM, detector_fanout=True, refine_distances=True)),
    'fan_grad_tall': (TALL, 2, 1, 1, 2, dict(free_prop_cm=DISTS_CM[:2], detector_fanout=True, refine_distances=True)),
}


def case_id(name):
    return name


def _sha(a):
    return hashlib.sha256(np.ascontiguousarray(a).tobytes()).hexdigest()


def _inputs(P, S, B, M, E):
    """Seeded by the shape alone: the three fan cases of the base field share their inputs."""
    Py, Px = P
    r = np.random.default_rng([Py, Px, S, B, M, E])
    shape = (Py + 8, Px + 8, S)
    obj = np.stack([2e-3 * r.uniform(size=shape), 2e-4 * r.uniform(size=shape)], -1).astype(np.float32)
    probes = (0.5 + r.uniform(0, 1, (M, Py, Px))) * np.exp(1j * r.uniform(-np.pi, np.pi, (M, Py, Px)))
    target = np.abs(r.standard_normal((B * E, Py, Px))).astype(np.float32)
    return shape, obj, MM.c2(probes), target


def run_case(A, ctx, name, raw=False):
    """One forward + adjoint launch (fan_grad: two into the same dL/dd buffer); {name: sha256 of the raw bytes}, or the arrays."""
    P, S, B, M, E, kw = SPECS[name]
    shape, obj, probes, target = _inputs(P, S, B, M, E)
    pos = POS[:B]
    eng = A.MultisliceEngine(ctx, shape, P, pos, ENERGY_EV, PSIZE_CM, n_probe_modes=M, max_batch=B, streamed=True, **kw)
    assert eng.streamed is True and len(eng.rounds(B)) == 1
    d_probe = ctx.array(probes)
    extra, launches = {}, 1
    if name == 'sparse_gz':
        extra = dict(grad_slice_pos=ctx.zeros((S,)))
    elif name == 'exit_shift':
        extra = dict(exit_shifts=ctx.array(SHIFTS), exit_shift_index=ctx.array(INDEX), grad_exit_shifts=ctx.zeros(SHIFTS.shape))
    elif name == 'probe_shift':
        extra = dict(shifts=ctx.array(SHIFTS), shift_index=ctx.array(INDEX), grad_shifts=ctx.zeros(SHIFTS.shape))
    elif name in ('fan_grad', 'fan_grad_tall'):
        extra = dict(grad_dists=ctx.zeros((E,)))
        launches = 2 if name == 'fan_grad' else 1
    eng.set_batch(pos, target)
    eng.rotate(ctx.array(obj), None)
    for _ in range(launches):
        g_probe = ctx.zeros(probes.shape)              # (+=: a buffer of its own per launch)
        eng.multislice(d_probe, grad_probe=g_probe, want_pred=True, **extra)
    ctx.sync()
    out = dict(loss_sums=eng._loss.view(0, (B * E,)).get(), pred=eng.pred(), obj_grad=eng.grad_rot.get(), probe_grad=g_probe.get())
    for k in ('grad_slice_pos', 'grad_exit_shifts', 'grad_shifts', 'grad_dists'):
        if k in extra:
            out['grad_shifts' if k == 'grad_exit_shifts' else k] = extra[k].get()
    eng.plan.close()
    for k, v in out.items():
        assert np.isfinite(v).all() and np.any(v), (name, k, 'not finite, or all zero')
    return out if raw else {k: _sha(v) for k, v in out.items()}


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
    assert sorted(recorded['digests']) == sorted(CASES) == sorted(SPECS)


@pytest.mark.parametrize('name', CASES)
def test_column_kernel_bits_are_the_recorded_ones(A, ctx, recorded, name):
    """st_col_conv_kernel, st_det_kernel, st_col_conv_sparse_kernel, es_col_conv_kernel, ps_colfft_kernel, ps_col_kernel,
    md_fanout_kernel, md_fanin_kernel, st_fresnel_table_kernel, st_dd_reduce_kernel: the bits of the build the fixture names."""
    got = run_case(A, ctx, name)
    want = recorded['digests'][name]
    assert sorted(got) == sorted(want)
    differ = [k for k in sorted(got) if got[k] != want[k]]
    assert not differ, '%s: bits differ from the recorded build in %s' % (name, ', '.join(differ))


def test_fan_cases_agree_with_each_other(A, ctx):
    """md_fanout_kernel, md_fanin_kernel with and without the distance gradient, on the device table and on the host table."""
    host, dev, grad = [run_case(A, ctx, n, raw=True) for n in ('fan_host', 'fan_dev', 'fan_grad')]
    for k in SHARED:
        assert np.array_equal(dev[k], grad[k]), ('the request for dL/dd changed', k)
    once = run_case(A, ctx, 'fan_dev', raw=True)
    assert all(np.array_equal(dev[k], once[k]) for k in SHARED)
    for k, bar in (('pred', BARS['pred']), ('loss_sums', BARS['loss']), ('obj_grad', BARS['grad']), ('probe_grad', BARS['grad'])):
        e = MM.rel(dev[k], host[k])
        print('device table vs host table: %s %.2e (bar %.0e)' % (k, e, bar))
        assert e < bar, (k, e)
