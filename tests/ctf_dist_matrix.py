"""Tables and references of the CTF distance-gradient matrix (tests/test_gpu_ctf_dist.py; importable without a GPU).

adm_ctfd_fwd_adj (adm_ctf_dist.hip) runs the launch group of adm_holo_ctf.hip with the distances on the device and sums dL/dd in
C4 / C5 under run-time branches.  ``BRANCHES`` names every one of them, ``ENTRY_POINTS`` the new entry point, each with the GPU tests
that reach it; ``FIELDS`` are taken from tests/ctf_matrix.FIELDS and are the smallest shapes at which the new code can go wrong.
tests/test_ctf_dist_coverage.py ties all of it to the sources.

The reference is tests/ctf_dist_ref.py in fp64 (held to golden F32 and to central differences by
tests/test_ctf_dist_ref_vs_golden.py), the yardstick the same restatement in float32.  The model sits at
d (1 + 0.1 cos(1.3 i + 2.9)) rounded to float32, the data are made at d: every |dL/dd_i| is then at least 1e-2 of the largest, so a
dropped or doubled distance is 50 bars away.  dL/dd is judged element by element:
    |g - g64| <= max(BARS['grad'], 3 x the restatement's error) x max|g64|.
"""
import numpy as np

from tests import ctf_dist_ref as DR
from tests import ctf_matrix as CM

BARS = CM.BARS
MIN_RATIO = 1e-2          # every |dL/dd_i| >= MIN_RATIO max|dL/dd|

FIELDS = (
    (16, 16, 1),          # one distance, 127 idle slots
    (16, 16, 3),
    (32, 16, 2), (16, 32, 2),
    (1024, 16, 3),        # LPB = 2, two rounds, the second ragged; the line reduction through LDS (two waves)
    (256, 16, 64),        # 8 rounds, 64 + 65 sums over two C5 blocks
    (2048, 16, 3),        # one slot, a four-wave line reduction, twiddles from global memory
    (16, 2048, 2),        # 2048 partial lines per distance
)
VARIANT_FIELD = (16, 16, 3)
PHASE_FIELD, PHASE_RUNG = CM.PHASE_FIELD, CM.PHASE_RUNGS[-1]

ALL_CLASSES = ('nd_1', 'c4_idle_slots', 'c4_ragged_last_round', 'c4_several_rounds', 'c4_one_slot', 'line_sum_shuffle', 'line_sum_lds_2_waves',
               'line_sum_lds_4_waves', 'nd_64', 'several_dist_sums_per_block', 'many_partials_per_distance')


def classes(ny, nx, nd):
    c = set(CM.classes(ny, nx, nd)) & set(ALL_CLASSES)
    tpr = CM.geometry(ny, nx, nd)['gy']['TPR']
    c.add('line_sum_shuffle' if tpr <= 64 else 'line_sum_lds_%d_waves' % (tpr // 64))
    if -(-nd // len(CM.geometry(ny, nx, nd)['row_blocks'])) > 1:
        c.add('several_dist_sums_per_block')
    if nx >= 2048:
        c.add('many_partials_per_distance')
    return c


_ACC = ('test_fields', 'test_golden_cases')
_VAR = ('test_variants',)
# every run-time branch the feature adds: where it is, the text that must be in the source, the tests that reach both sides
BRANCHES = {
    'ctf_c_of: dists_dev set / NULL': ('adm_holo_ctf.hip', 'A.dists_dev ?', _ACC + ('test_one_handle_alternates_the_entries', 'test_the_old_entry_gives_the_recorded_bits')),
    'ctf_c4: the rounds with / without dacc': ('adm_holo_ctf.hip', 'A.grad_dists ? ctf_c4_rounds<NY, true>(', _ACC + ('test_null_grad_dists_changes_no_other_bit',)),
    'ctf_c4: line_sum shuffle / LDS': ('adm_holo_ctf.hip', 'line_sum<LG::TPR, double>(dacc, redd)', ('test_fields',)),
    'ctf_c4: idle slots write nothing': ('adm_holo_ctf.hip', 'if (ok && t == 0) A.partd[', ('test_fields', 'test_variants')),
    'ctf_c5: the second loop of sums': ('adm_holo_ctf.hip', 'for (int o = blockIdx.x; o < A.nd; o += gridDim.x) ctf_sum_dist(A, o);', _ACC),
    'ctf_sum_dist: += / =': ('adm_holo_ctf.hip', '(A.set_obj ? 0.f : A.grad_dists[o]) + g', _VAR),
    'group_run: grad_dists only with want_grad': ('adm_holo_ctf.hip', 'A.grad_dists = want_grad ? grad_dists : nullptr;', ('test_forward_only_touches_no_gradient',)),
    'adm_ctfd_fwd_adj: partials allocated on first use': ('adm_ctf_dist.hip', '!h->partd', ('test_fields', 'test_one_handle_alternates_the_entries')),
}
ENTRY_POINTS = {
    'adm_ctfd_fwd_adj': _ACC + _VAR + ('test_refusals',),
}
ENGINE_TESTS = ('test_engine_refine_distances', 'test_engine_refusals')

# name -> launch keywords of tests/test_gpu_ctf_dist.py:launch
VARIANTS = {
    'accumulate_seeded': dict(seed='seeded'),
    'overwrite_nan_sentinel': dict(seed='nan', overwrite=True),
}


def inputs(ny, nx, nd, phase=None):
    """ctf_matrix.inputs (data made at the true distances) + 'model_dists': where the model sits, float32-exact."""
    c = dict(CM.inputs(ny, nx, nd, phase=phase))
    c['model_dists'] = DR.model_dists(c['dists'])
    return c


def ref_run(c, dtype='float64'):
    return DR.forward_adjoint(c['obj'][:, :, 0], c['model_dists'], c['lg_kappa'], c['data'], CM.ENERGY_EV, CM.PSIZE_CM, c['raw'], dtype)


_CASES = {}


def case(ny, nx, nd, **kw):
    """Inputs and the reference pair (o64, o32), built once per process."""
    key = (ny, nx, nd, tuple(sorted(kw.items())))
    if key not in _CASES:
        c = inputs(ny, nx, nd, **kw)
        c['o64'], c['o32'] = ref_run(c, 'float64'), ref_run(c, 'float32')
        _CASES[key] = c
    return _CASES[key]


def dist_errors(g, g64):
    """Element-wise distance of dL/dd from the fp64 reference, relative to max|dL/dd|."""
    g64 = np.asarray(g64, np.float64)
    return np.abs(np.asarray(g, np.float64) - g64) / np.abs(g64).max()


def dist_bar(c):
    """max(BARS['grad'], 3 x the restatement's error), per element."""
    return np.maximum(BARS['grad'], 3 * dist_errors(c['o32']['grad_dists'], c['o64']['grad_dists']))


def conditions(c):
    """What the reference pair alone decides: min I_d, every |dL/dd_i| >= MIN_RATIO of the largest, and the float32 restatement within
    a third of every bar.  Asserts; returns the figures as a line of text."""
    o, s = c['o64'], c['o32']
    assert o['I'].min() >= CM.MIN_I, float(o['I'].min())
    g = np.abs(o['grad_dists'])
    ratio = float(g.min() / g.max())
    assert ratio >= MIN_RATIO, (c['ny'], c['nx'], c['nd'], ratio)
    e = dict(pred=CM.rel(s['pred'], o['pred']), grad=CM.rel(s['grad_delta'], o['grad_delta']), loss=abs(s['loss'] / o['loss'] - 1),
             gkappa=abs(s['grad_lg_kappa'] / o['grad_lg_kappa'] - 1), gdists=float(dist_errors(s['grad_dists'], o['grad_dists']).max()))
    for k, v in e.items():
        assert v < BARS['grad' if k == 'gdists' else k] / 3, (c['ny'], c['nx'], c['nd'], k, v)
    return 'min |dL/dd| / max %.2e;  fp32 restatement: pred %.1e  grad %.1e  loss %.1e  gkappa %.1e  gdists %.1e' % (
        ratio, e['pred'], e['grad'], e['loss'], e['gkappa'], e['gdists'])
