"""CPU: tests/fresnel_kappa_ref.py -- the checker of the GPU tests of the single-material constraint -- against golden F34 (the
reference implementation's own results, tests/golden/gen_f34_fresnel_kappa.py), its internal consistency, the float32 mirrors of
the two kernels against the double arithmetic they mirror, and the two new entries of the C ABI in header, binding and build."""
import ast
import ctypes
import os
import re

import numpy as np
import pytest

from oracle import adorym_oracle as O
from tests import fresnel_kappa_ref as KR

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENERGY_EV, PSIZE_CM = 8000., 1e-6
rel = lambda a, b: float(np.linalg.norm(np.asarray(a, np.float64) - b) / np.linalg.norm(b))


@pytest.fixture(scope='module')
def F():
    return np.load(os.path.join(ROOT, 'tests', 'golden', 'F34_fresnel_kappa.npz'))


def kernel_case(F, name):
    names = [str(n) for n in F['kernel_cases']]
    geo, sg, rdt, lg = ast.literal_eval(str(F['kernel_case_params'][names.index(name)]))
    c = {k: F['%s/%s' % (name, k)] for k in ('obj', 'probe', 'meas', 'lg_kappa')}
    c.update(geo=geo, sign_convention=sg, raw_data_type=rdt, dists=[float(d) for d in F['kernel_dists_cm']])
    assert float(c['lg_kappa'][0]) == lg
    return c


def ref_run(c, dtype, lg_kappa=None, obj=None):
    phys = O.Physics(c['probe'].shape[-2:], ENERGY_EV, PSIZE_CM, free_prop_cm=c['dists'][0], sign_convention=c['sign_convention'])
    return KR.forward_adjoint(c['obj'].astype(np.float64) if obj is None else obj, c['lg_kappa'][0] if lg_kappa is None else lg_kappa, None,
                              c['probe'].astype(np.complex128), c['meas'], phys, c['dists'], dtype, c['raw_data_type'])


def test_golden_holds_every_stated_case(F):
    names = [str(n) for n in F['kernel_cases']]
    par = [ast.literal_eval(str(p)) for p in F['kernel_case_params']]
    assert len(names) >= 8
    for geo, shape in (('2d', (16, 32, 1, 2)), ('3d', (12, 20, 5, 2))):
        mine = [p for p in par if p[0] == geo]
        assert {p[1] for p in mine} == {1, -1} and {p[2] for p in mine} == {'magnitude', 'intensity'} and {p[3] for p in mine} == {-2., -0.5, 1.7}
        for lg in (-2., -0.5, 1.7):          # every kappa under both sign conventions and both data types
            assert {p[1] for p in mine if p[3] == lg} == {1, -1} and {p[2] for p in mine if p[3] == lg} == {'magnitude', 'intensity'}
        assert all(F[n + '/obj'].shape == shape for n, p in zip(names, par) if p[0] == geo)
    assert len(F['kernel_dists_cm']) == 3
    for n in names:
        assert F[n + '/obj'][..., 1].any() and not F[n + '/grad'][..., 1].any()          # beta is there to be ignored, and is
    assert float(F['gkappa_yardstick']) == max(F[n + '/err32'][3] for n in names) >= 1e-6
    for tag, shape in (('drv2d', (32, 32, 1, 2)), ('drv3d', (16, 16, 16, 2))):
        assert tag + '/ref_error' not in F.files and F[tag + '/fp64/obj'].shape == shape


def test_fp64_restatement_equals_the_reference(F):
    """(a): prediction, loss, dL/dobj and dL/dlg_kappa of the host reference in fp64 against the reference's fp64 run."""
    for name in (str(n) for n in F['kernel_cases']):
        r = ref_run(kernel_case(F, name), 'float64')
        assert rel(r['pred'], F[name + '/pred']) < 1e-10, name
        assert abs(r['loss'] / float(F[name + '/loss']) - 1) < 1e-10, name
        assert rel(r['grad'], F[name + '/grad']) < 1e-10 and not r['grad'][..., 1].any(), name
        assert abs(r['grad_lg_kappa'] / float(F[name + '/gkappa']) - 1) < 1e-10, name


def test_fp32_restatement_errs_like_the_reference_fp32(F):
    """The float32 restatement's distance from fp64 is that of the reference's own float32 run within a factor of three either way
    (prediction and delta gradient)."""
    for name in (str(n) for n in F['kernel_cases']):
        c = kernel_case(F, name)
        o, s = ref_run(c, 'float64'), ref_run(c, 'float32')
        e32 = F[name + '/err32']
        mine = [rel(s['pred'], o['pred']), abs(s['loss'] / o['loss'] - 1), rel(s['grad'][..., 0], o['grad'][..., 0]),
                abs(s['grad_lg_kappa'] / o['grad_lg_kappa'] - 1)]
        print(name, 'reference fp32', e32, 'restatement fp32', mine)
        for k in (0, 2):
            assert e32[k] / 3 < mine[k] < 3 * e32[k], (name, k, mine[k], e32[k])


@pytest.mark.parametrize('name', ['2d_p1_intensity_k1', '3d_m1_magnitude_k1', '3d_p1_magnitude_k2'])
def test_gradients_against_central_differences(F, name):
    """dL/dlg_kappa and a directional derivative of dL/ddelta against central differences of the restatement's own loss."""
    c = kernel_case(F, name)
    r = ref_run(c, 'float64')
    k0, h = float(c['lg_kappa'][0]), 1e-5
    fd = (ref_run(c, 'float64', k0 + h)['loss'] - ref_run(c, 'float64', k0 - h)['loss']) / (2 * h)
    assert abs(fd / r['grad_lg_kappa'] - 1) < 1e-6, (fd, r['grad_lg_kappa'])
    o = c['obj'].astype(np.float64)
    v = np.random.default_rng(7).standard_normal(o.shape[:-1]) * np.abs(o[..., 0]).max()
    step = lambda t: np.stack([o[..., 0] + t * v, o[..., 1]], -1)
    fd = (ref_run(c, 'float64', obj=step(1e-4))['loss'] - ref_run(c, 'float64', obj=step(-1e-4))['loss']) / 2e-4
    an = float((r['grad'][..., 0] * v).sum())
    assert abs(fd / an - 1) < 1e-6, (fd, an)
    # beta of the free object is not an argument: any value gives the same loss
    other = np.stack([o[..., 0], 7 * o[..., 1] + 1], -1)
    assert ref_run(c, 'float64', obj=other)['loss'] == r['loss']


def drv_inputs(F, tag):
    par = ast.literal_eval(str(F[tag + '/params']))
    N = par['N']
    phys = O.Physics((N, N), ENERGY_EV, PSIZE_CM, free_prop_cm=par['dists_cm'][0])
    probe = (F[tag + '/probe_mag'] * np.exp(1j * F[tag + '/probe_phase']))[None]
    theta_ls = np.linspace(0, np.pi, par['n_theta'], dtype='float32')
    kw = dict(n_epochs=par['n_epochs'], learning_rate=par['learning_rate'], ctf_lg_kappa_learning_rate=par['ctf_lg_kappa_learning_rate'],
              raw_data_type=par['raw_data_type'], two_d=par['S'] == 1)
    return par, (F[tag + '/prj'].astype(np.float64), [F[tag + '/guess_delta'], F[tag + '/guess_beta']], probe, phys, list(par['dists_cm']), theta_ls,
                 par['lg_kappa']), kw


@pytest.mark.parametrize('tag', ['drv2d', 'drv3d'])
def test_driver_restatement_equals_the_reference_driver(F, tag):
    """fresnel_kappa_ref.reconstruct against the reference driver's fp64 run (golden F34 (b)): every loss, ctf_lg_kappa after every
    update, the final object; beta has not moved."""
    par, args, kw = drv_inputs(F, tag)
    r = KR.reconstruct(*args, **kw)
    x64 = F[tag + '/fp64/obj']
    assert len(r['losses']) == par['n_epochs'] * par['n_theta'] == len(F[tag + '/fp64/losses'])
    assert np.abs(np.array(r['losses']) / F[tag + '/fp64/losses'] - 1).max() < 1e-9
    assert np.abs(np.array(r['lg_kappa_trace']) - F[tag + '/fp64/lg_kappa_trace']).max() < 1e-9
    assert np.abs(r['obj'] - x64).max() < 1e-9 * np.abs(x64).max()
    assert np.array_equal(x64[..., 1], F[tag + '/guess_beta'].astype(np.float64))
    assert abs(r['lg_kappa'] - par['lg_kappa']) > 5e-3                          # (kappa has moved)


# ------------------------------------------------------------------------------------------------- the kernels' float32 mirrors
@pytest.mark.parametrize('lg', (-3., 0., 1.7, 3.))
def test_mirrors_against_double_arithmetic(lg):
    r = np.random.default_rng(int(10 * (lg + 3)))
    n = 4099
    obj, gt, go = (r.standard_normal((n, 2)).astype(np.float32) for _ in range(3))
    k64 = KR.kappa64(lg)
    assert abs(k64 / 10. ** float(np.float32(lg)) - 1) < 1e-14 and KR.kappa32(lg) == np.float32(k64)
    t = KR.tie(obj, lg)
    assert t.dtype == np.float32 and np.array_equal(t[:, 0], obj[:, 0])
    assert np.abs(t[:, 1] - k64 * obj[:, 0].astype(np.float64)).max() <= 2. ** -23 * np.abs(k64 * obj[:, 0]).max()
    for mode in (1, 2):
        f = KR.fold(lg, gt, go, mode)
        u = gt[:, 0].astype(np.float64) + k64 * gt[:, 1].astype(np.float64)
        want = go[:, 0].astype(np.float64) + u if mode == 1 else u
        assert f.dtype == np.float32 and np.abs(f[:, 0] - want).max() <= 3 * 2. ** -23 * (np.abs(go[:, 0]).max() + np.abs(u).max())
        assert np.array_equal(f[:, 1], go[:, 1]) if mode == 1 else not f[:, 1].any()
    S, scale = KR.fold_sum_exact(obj, gt)
    naive = float((obj[:, 0].astype(np.float64) * gt[:, 1].astype(np.float64)).sum())
    assert abs(naive - S) <= (n - 1) * 2. ** -53 * scale
    assert KR.grad_lg_kappa32(lg, S) == np.float32(KR.LN10 * k64 * S)


# ------------------------------------------------------------------------------------------------------------- ABI and build
def test_the_two_entries_are_declared_bound_built_and_documented():
    from adorym_amd import _lib
    from adorym_amd.csrc import build
    hdr = re.sub(r'/\*.*?\*/', '', open(os.path.join(ROOT, 'include', 'adm.h')).read(), flags=re.S)
    assert re.search(r'int adm_kappa_tie\(adm_ctx\* ctx, const float\* obj, const float\* lg_kappa, size_t n_vox, float\* out\);', hdr)
    assert re.search(r'int adm_kappa_fold\(adm_ctx\* ctx, const float\* obj, const float\* lg_kappa, const float\* grad_tied, size_t n_vox, int mode,\s*'
                     r'float\* grad_obj, float\* grad_lg_kappa, double\* scratch\);', hdr)
    VP, SZ, I = ctypes.c_void_p, ctypes.c_size_t, ctypes.c_int
    assert _lib.SIGNATURES['adm_kappa_tie'] == (I, [VP, VP, VP, SZ, VP])
    assert _lib.SIGNATURES['adm_kappa_fold'] == (I, [VP, VP, VP, VP, SZ, I, VP, VP, VP])
    m = re.search(r'#define ADM_KAPPA_SCRATCH_DOUBLES \(ADM_CG_MAX_BLOCKS \+ 1\)', hdr)
    assert m and _lib.KAPPA_SCRATCH_DOUBLES == _lib.CG_MAX_BLOCKS + 1
    assert 'adm_kappa_tie.hip' in build.SRCS
    lib = _lib.load()
    assert hasattr(lib, 'adm_kappa_tie') and hasattr(lib, 'adm_kappa_fold')
    src = open(os.path.join(ROOT, 'adorym_amd', 'csrc', 'adm_kappa_tie.hip')).read()
    assert 'atomic' not in src.replace('No atomics', '') and '#include "adm_optim.h"' in src
    # the shared walk lives in one place: neither streaming file keeps a copy of its own
    cg = open(os.path.join(ROOT, 'adorym_amd', 'csrc', 'adm_cg.hip')).read()
    for text in (src, cg):
        assert '__shfl_down' not in text and 'flat_walk<' in text
    with open(os.path.join(ROOT, 'INTEGRATION.md')) as f:
        doc = f.read()
    assert '`adm_kappa_tie`' in doc and '`adm_kappa_fold`' in doc
    import adorym_amd
    assert adorym_amd.HomogeneousObject is not None


def test_the_model_refuses_without_a_gpu():
    """What needs no device: the opt-in, and every refusal by name."""
    from adorym_amd import MultiDistModel
    from adorym_amd.multidist_model import KAPPA_REFUSED
    ho = object()
    base = dict(engine=None, holo_engine=None, two_d_mode=True, optimize_ctf_lg_kappa=True, forward_algorithm='fresnel')
    fm = MultiDistModel(device=None, common_vars_dict=dict(base))
    assert fm.homogeneous is None
    with pytest.raises(NotImplementedError, match="^optimize_ctf_lg_kappa with forward_algorithm='fresnel' is outside the accelerated path$"):
        fm._check(0, np.array([1.7]), None)
    fm = MultiDistModel(device=None, common_vars_dict=dict(base, homogeneous_object=ho))
    assert fm.homogeneous is ho
    fm._check(0, np.array([1.7]), None)
    assert MultiDistModel(device=None, common_vars_dict=dict(base, homogeneous_object=ho, optimize_ctf_lg_kappa=False)).homogeneous is None
    for extra, what in ((dict(safe_zone_width=2), 'data divided into sub-tiles or safe_zone_width > 0'),
                        (dict(tile_engine=object()), 'data divided into sub-tiles or safe_zone_width > 0'),
                        (dict(unknown_type='real_imag'), "unknown_type='real_imag'"),
                        (dict(optimize_all_probe_pos=True), 'optimize_all_probe_pos'),
                        (dict(n_ranks=2), 'more than one rank')):
        m = MultiDistModel(device=None, common_vars_dict=dict(base, homogeneous_object=ho, **extra))
        with pytest.raises(NotImplementedError, match=re.escape(KAPPA_REFUSED % what)):
            m._check(extra.get('safe_zone_width', 0), np.array([1.7]), np.zeros((3, 2)))
