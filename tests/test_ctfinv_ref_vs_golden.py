"""CPU: tests/ctfinv_ref.py against golden F31 (the reference's multidistance_ctf_wrapped in fp64 and fp32), the bars of
tests/ctfinv_matrix.py against the figures they were derived from, and every case of the GPU modules against its conditions."""
import os

import numpy as np
import pytest

from tests import ctfinv_matrix as M
from tests import ctfinv_ref as IR

G = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden', 'F31_ctf_invert.npz'))
GOLDEN_CASES = [str(n) for n in G['cases']]


def test_the_golden_holds_the_cases_of_the_issue():
    want = {'%dx%dx%d_%s' % (f + (raw,)) for f, raw in M.CM.GOLDEN_FIELDS.items()} | {'%dx%dx%d_intensity_pure_phase' % M.PHASE_FIELD}
    assert set(GOLDEN_CASES) == want
    assert float(G['%dx%dx%d_intensity_pure_phase/lg_kappa' % M.PHASE_FIELD]) == M.PURE_PHASE_LG_KAPPA


@pytest.mark.parametrize('name', GOLDEN_CASES)
def test_restatement_equals_the_reference(name):
    """fp64 to rounding; the float32 restatement is as far from fp64 as the reference's own float32 run (within a factor of 1.5
    either way: the two order their float32 operations alike, not identically)."""
    data, dists, lgk = G[name + '/data'], G[name + '/dists'], float(G[name + '/lg_kappa'])
    field = tuple(int(v) for v in name.split('_')[0].split('x'))
    ours = M.CM.inputs(*field, raw=name.split('_')[1])
    assert np.array_equal(ours['data'], data) and np.array_equal(ours['dists'], dists)          # the golden's inputs are ctf_matrix.inputs'
    p64 = IR.retrieve(data, dists, lgk, M.ENERGY_EV, M.PSIZE_CM)
    p32 = IR.retrieve(data, dists, lgk, M.ENERGY_EV, M.PSIZE_CM, dtype=np.float32)
    assert p32.dtype == np.float32
    e64, e32, g32 = M.rel(p64, G[name + '/phase']), M.rel(p32, p64), float(G[name + '/err32'])
    print('%s: fp64 %.1e; float32 restatement %.1e, reference %.1e' % (name, e64, e32, g32))
    assert e64 < 1e-13
    assert g32 / 1.5 <= e32 <= 1.5 * g32
    assert g32 <= M.ERR32


def test_pure_phase_is_finite_and_has_no_dc():
    name = '%dx%dx%d_intensity_pure_phase' % M.PHASE_FIELD
    p = G[name + '/phase']
    assert np.isfinite(p).all() and abs(p.mean()) < 1e-15 * np.abs(p).max()


def test_identity_bar_is_the_reference_s_own_resample():
    """'<case>/identity' = (fp64, fp32) distance of the reference's phase with prj_affine_ls = identity from its phase without."""
    ident = np.array([G[n + '/identity'] for n in GOLDEN_CASES])
    assert ident[:, 0].max() < 1e-13
    assert ident[:, 1].max() <= M.IDENTITY_ERR32 <= 1.05 * ident[:, 1].max() and M.IDENTITY_BAR == 3 * M.IDENTITY_ERR32


def test_what_the_reference_driver_does_is_on_record():
    """update_using_external_algorithm='ctf' in the reference driver reads the float argument ctf_lg_kappa with [0]."""
    text = str(G['drv/external_ctf'])
    assert text.startswith('TypeError') and 'subscriptable' in text


def test_alpha_reaches_the_right_bin():
    """The table form of alpha: the value of bin (ky, kx) divides that bin -- a transposed or shifted table is far above the bar."""
    c = M.case('32x16x2_alpha_table')
    a = M.alpha_of('table', c['ny'], c['nx'])
    assert len(np.unique(a)) == a.size and a.dtype == np.float32
    wrong = IR.retrieve(c['data'], c['dists'], c['lg_kappa'], M.ENERGY_EV, M.PSIZE_CM, alpha=np.roll(a, 1, axis=1))
    swapped = IR.retrieve(c['data'], c['dists'], c['lg_kappa'], M.ENERGY_EV, M.PSIZE_CM, alpha=a.reshape(c['nx'], c['ny']).T)
    assert M.rel(wrong, c['o64']) > 10 * c['bar'] and M.rel(swapped, c['o64']) > 10 * c['bar']
    none = IR.retrieve(c['data'], c['dists'], c['lg_kappa'], M.ENERGY_EV, M.PSIZE_CM)
    assert M.rel(none, c['o64']) > 10 * c['bar']


@pytest.mark.parametrize('name', list(M.CASES) + list(M.VALUE_CASES))
def test_conditions(name):
    print(name, M.conditions(M.case(name)))


def test_the_bar_is_three_times_the_worst_float32_restatement():
    worst = max(M.rel(M.case(n)['o32'], M.case(n)['o64']) for n in M.CASES)
    assert worst <= M.ERR32 <= 1.1 * worst and M.BAR == 3 * M.ERR32
    for n, v in M.VALUE_ERR32.items():
        e = M.rel(M.case(n)['o32'], M.case(n)['o64'])
        assert e <= v and (v == M.ERR32 or v <= 1.1 * e), (n, e, v)


def test_driver_conditions():
    print(M.drv_conditions())
    a, b = M.drv_ref('float64'), M.drv_ref('float32')
    e = M.drv_errors(b['lg_kappa_trace'], b['obj'][..., 0], b['losses'])
    assert set(e) == set(M.DRV_ERR32) == set(M.DRV_BARS)
    for k, v in e.items():
        assert v <= M.DRV_ERR32[k] <= 1.1 * v, (k, v)
    # the hook: the delta after the first minibatch is the inversion at the starting lg_kappa; beta never moves
    c = M.drv_inputs()
    first = IR.retrieve(c['data'], c['dists'], np.float32(M.LG_KAPPA), M.ENERGY_EV, M.PSIZE_CM)      # (kappa lives in float32)
    assert np.array_equal(a['first_delta'], first)
    assert np.array_equal(a['obj'][..., 1], c['obj'][..., 1].astype(np.float64))
