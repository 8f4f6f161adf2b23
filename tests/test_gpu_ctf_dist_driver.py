"""optimize_free_prop and optimize_prj_affine under forward_algorithm='ctf' on the GPU (pytest -m gpu): MultiDistModel's CTF route
with a CTFEngine that refines its distances and / or a HologramRegistration, and reconstruct_ptychography with the private keywords
ctf_free_prop / ctf_prj_affine, in 2-D and with ctf_tomography.

Checker: golden F32 (tests/golden/gen_f32_ctf_dist.py: the reference in fp64, its own fp32 run as the yardstick) and
tests/ctf_dist_ref.py (held to that golden by tests/test_ctf_dist_ref_vs_golden.py).  Losses and object by check_run of
tests/test_gpu_ctf_driver.py; distances and matrices after every update by its rule for small parameters:
|x - x64| <= 3 |x32 - x64| + (updates so far) x the float32 spacing at the parameter's value (check_small)."""
import ast
import os
import pickle

import numpy as np
import pytest

from tests import ctf_dist_matrix as DM
from tests import ctf_dist_ref as DR
from tests import ctf_matrix as CM
from tests import ctf_tomo_ref as TR
from tests import multidist3d_affine_ref as AR
from tests.test_gpu_ctf_driver import check_run
from tests.test_gpu_ctf_driver import drv_kw as old_drv_kw
from tests.test_gpu_ctf_tomo_driver import drv_kw as tomo_drv_kw

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OFF = np.array([1.10, 0.92, 1.05])
# (golden F29's matrices: matrix 0 the identity)
KERNEL_THETA = np.stack([AR.IDENTITY, AR.matrix(0.03, 1.04, (0.05, -0.03)), AR.matrix(-0.02, 0.97, (-0.04, 0.06))])
# the warps of the tomography run's holograms 1 and 2 (golden F32's)
WARP = np.stack([AR.IDENTITY, AR.matrix(0.02, 1.03, (0.06, -0.05)), AR.matrix(-0.02, 0.97, (-0.05, 0.06))])


@pytest.fixture(scope='module')
def A():
    import adorym_amd
    return adorym_amd


@pytest.fixture(scope='module')
def F():
    return np.load(os.path.join(ROOT, 'tests', 'golden', 'F32_ctf_dist.npz'))


@pytest.fixture(scope='module')
def F26():
    return np.load(os.path.join(ROOT, 'tests', 'golden', 'F26_ctf.npz'))


@pytest.fixture(scope='module')
def F30():
    return np.load(os.path.join(ROOT, 'tests', 'golden', 'F30_ctf_tomo.npz'))


# ------------------------------------------------------------------------------------------------------------ model level
def model_args(c, dists, theta=None):
    return dict(probe_real=None, probe_imag=None, probe_defocus_mm=0., probe_pos_offset=None, this_i_theta=0, this_pos_batch=np.zeros((1, 2)),
                prj=c['data'][None], probe_pos_correction=None, this_ind_batch=np.array([0]), free_prop_cm=dists, safe_zone_width=0,
                prj_affine_ls=theta, ctf_lg_kappa=np.array([c['lg_kappa']]), prj_pos_offset=None)


def check_gdists(got, c, o64, o32, what):
    e = DM.dist_errors(got, o64['grad_dists'])
    bar = np.maximum(DM.BARS['grad'], 3 * DM.dist_errors(o32['grad_dists'], o64['grad_dists']))
    print('%s: dL/dd %s (fp64 %s) errors %s bars %s' % (what, got, o64['grad_dists'], e, bar))
    assert (e <= bar).all(), (what, e, bar)


@pytest.mark.parametrize('register', (False, True), ids=('plain', 'registered'))
def test_model_level_2d(A, register):
    """The gradients' places in the tuple: dL/d free_prop_cm (a DeviceArray [n_dists], zeroed per evaluation) at that argument's
    place, dL/d prj_affine_ls at its own; '+=' into zeros and '=' over garbage give the same."""
    ctx = A.Context(0)
    c = DM.case(16, 16, 3)
    theta = KERNEL_THETA if register else None
    eng = A.CTFEngine(ctx, (16, 16), 3, CM.ENERGY_EV, CM.PSIZE_CM, raw_data_type='magnitude' if register else 'intensity',
                      refine_distances=True, dists_cm=c['model_dists'])
    ms = A.MultisliceEngine(ctx, (16, 16, 1), (8, 8), np.zeros((1, 2), int), CM.ENERGY_EV, CM.PSIZE_CM, free_prop_cm=0, max_batch=1)
    cv = dict(engine=ms, ctf_engine=eng, forward_algorithm='ctf', two_d_mode=True, unknown_type='delta_beta', optimize_ctf_lg_kappa=True,
              optimize_free_prop=True, optimize_prj_affine=register, prj=c['data'][None], n_probe_modes=1, safe_zone_width=0)
    if register:
        cv['hologram_registration'] = A.HologramRegistration(ctx, 3, (16, 16), 'intensity')
    fm = A.MultiDistModel(device=ctx, common_vars_dict=cv, raw_data_type='intensity')
    run = lambda dt: (DR.registered(c['obj'][..., 0], c['model_dists'], c['lg_kappa'], c['data'], theta, CM.ENERGY_EV, CM.PSIZE_CM, 'intensity', dt)
                      if register else DM.ref_run(c, dt))
    o64, o32 = run('float64'), run('float32')
    obj = ctx.array(c['obj'][:, :, None, :])
    i_k, i_fp, i_af = (fm.get_argument_index(n) for n in ('ctf_lg_kappa', 'free_prop_cm', 'prj_affine_ls'))
    order = [0, i_fp, i_k] + ([i_af] if register else [])
    for dists in (eng.dists, c['model_dists']):          # the engine's own array, and host values uploaded into it
        args = model_args(c, dists, theta)
        assert abs(fm.get_loss_function()(obj, **args) / o64['loss'] - 1) < CM.BARS['loss']
        for init in (False, True):
            g = ctx.zeros((16, 16, 1, 2)) if not init else ctx.array(np.full((16, 16, 1, 2), 7., np.float32))
            out = fm.loss_and_gradients(order, g, obj, _init_grad=init, **args)
            what = 'model 2-D%s (%s)' % (' registered' if register else '', 'overwriting' if init else 'accumulating')
            assert out[0] is g and CM.rel(g.get()[:, :, 0, 0], o64['grad_delta']) < CM.BARS['grad'] and not g.get()[..., 1].any()
            assert out[1].shape == (3,)
            check_gdists(out[1].get(), c, o64, o32, what)
            assert abs(out[2].get()[0] / o64['grad_lg_kappa'] - 1) < CM.BARS['gkappa']
            assert abs(fm.current_loss / o64['loss'] - 1) < CM.BARS['loss']
            if register:
                ga = out[3].get()
                assert ga.shape == (3, 2, 3)
                for d in (1, 2):
                    e, e32 = CM.rel(ga[d], o64['grad_theta'][d]), CM.rel(o32['grad_theta'][d], o64['grad_theta'][d])
                    print('%s: dL/dtheta[%d] %.2e (fp32 restatement %.2e)' % (what, d, e, e32))
                    assert e <= max(1e-3, 3 * e32), (what, d, e, e32)
    with pytest.raises(ValueError, match="engine's own array"):
        fm.loss_and_gradients(order, ctx.zeros((16, 16, 1, 2)), obj, **model_args(c, ctx.array(np.float32(c['model_dists'])), theta))
    ms.plan.close()
    ctx.close()


@pytest.mark.parametrize('register', (False, True), ids=('plain', 'registered'))
def test_model_level_with_a_projector(A, register):
    """A 16^3 object through the RotatedProjector: the same engine call, dL/dd at its place; with a HologramRegistration the
    registered holograms are the group's data and dL/d prj_affine_ls comes from its predictions."""
    ctx = A.Context(0)
    name = 'y16x16z16_t0.7_d3'
    c = TR.inputs(name)
    md = DR.round32(c['dists'] * OFF)
    theta = KERNEL_THETA if register else None
    eng = A.CTFEngine(ctx, (16, 16), 3, CM.ENERGY_EV, CM.PSIZE_CM, raw_data_type='magnitude' if register else 'intensity',
                      refine_distances=True, dists_cm=md)
    rp = A.RotatedProjector(ctx, c['size'])
    table = A.RotationTable(ctx, c['size'], c['theta'])
    cv = dict(engine=None, ctf_engine=eng, ctf_projector=rp, forward_algorithm='ctf', two_d_mode=False, unknown_type='delta_beta',
              optimize_ctf_lg_kappa=True, optimize_free_prop=True, optimize_prj_affine=register, prj=c['data'][None], n_probe_modes=1,
              safe_zone_width=0, rotation_tables=lambda i: table)
    if register:
        cv['hologram_registration'] = A.HologramRegistration(ctx, 3, (16, 16), 'intensity')
    fm = A.MultiDistModel(device=ctx, common_vars_dict=cv, raw_data_type='intensity')
    from oracle import adorym_oracle as O
    coords = O.rotation_coords(c['size'], np.float32(c['theta']))
    slice_of = lambda dt: TR.project(c['obj'], coords, dt)[..., 0]
    run = lambda dt: (DR.registered(slice_of(dt), md, c['lg_kappa'], c['data'], theta, CM.ENERGY_EV, CM.PSIZE_CM, 'intensity', dt) if register
                      else DR.forward_adjoint(slice_of(dt), md, c['lg_kappa'], c['data'], CM.ENERGY_EV, CM.PSIZE_CM, 'intensity', dt))
    o64, o32 = run('float64'), run('float32')
    obj = ctx.array(c['obj'])
    i_fp, i_af = fm.get_argument_index('free_prop_cm'), fm.get_argument_index('prj_affine_ls')
    order = [0, i_fp] + ([i_af] if register else [])
    args = model_args(c, eng.dists, theta)
    assert abs(fm.get_loss_function()(obj, **args) / o64['loss'] - 1) < CM.BARS['loss']
    for init in (False, True):
        g = ctx.zeros(c['obj'].shape) if not init else ctx.array(np.full(c['obj'].shape, 7., np.float32))
        out = fm.loss_and_gradients(order, g, obj, _init_grad=init, **args)
        what = 'model with a projector%s' % (' registered' if register else '')
        assert out[0] is g and abs(fm.current_loss / o64['loss'] - 1) < CM.BARS['loss']
        check_gdists(out[1].get(), c, o64, o32, what)
        want = TR.backproject(np.stack([o64['grad_delta'], np.zeros_like(o64['grad_delta'])], -1), coords, 16)
        assert CM.rel(g.get()[..., 0], want[..., 0]) < CM.BARS['grad'] and not g.get()[..., 1].any()
        if register:
            ga = out[2].get()
            for d in (1, 2):
                e, e32 = CM.rel(ga[d], o64['grad_theta'][d]), CM.rel(o32['grad_theta'][d], o64['grad_theta'][d])
                print('%s: dL/dtheta[%d] %.2e (fp32 restatement %.2e)' % (what, d, e, e32))
                assert e <= max(1e-3, 3 * e32), (what, d, e, e32)
    rp.close()
    ctx.close()


def test_model_refusals(A):
    """A plain engine and no registration: both flags are refused with the messages they had; a registration built for another
    field, raw type or an engine that is not fed magnitudes is a ValueError."""
    ctx = A.Context(0)
    plain = A.CTFEngine(ctx, (16, 16), 3, CM.ENERGY_EV, CM.PSIZE_CM)
    base = dict(engine=None, ctf_engine=plain, forward_algorithm='ctf', two_d_mode=True, unknown_type='delta_beta', n_probe_modes=1)
    for flag in ('optimize_free_prop', 'optimize_prj_affine', 'optimize_all_probe_pos', 'optimize_probe'):
        fm = A.MultiDistModel(device=ctx, common_vars_dict=dict(base, **{flag: True}), raw_data_type='intensity')
        with pytest.raises(NotImplementedError, match="forward_algorithm='ctf' with %s is outside" % flag):
            fm._check(0, np.array([1.7]), None)
    ref = A.CTFEngine(ctx, (16, 16), 3, CM.ENERGY_EV, CM.PSIZE_CM, raw_data_type='magnitude', refine_distances=True)
    for flag in ('optimize_all_probe_pos', 'optimize_probe'):          # ... stay refused whatever the engine can do
        cv = dict(base, ctf_engine=ref, hologram_registration=A.HologramRegistration(ctx, 3, (16, 16), 'intensity'), **{flag: True})
        with pytest.raises(NotImplementedError, match=flag):
            A.MultiDistModel(device=ctx, common_vars_dict=cv, raw_data_type='intensity')._check(0, np.array([1.7]), None)
    for reg, eng, what in ((A.HologramRegistration(ctx, 2, (16, 16), 'intensity'), ref, 'another field'),
                           (A.HologramRegistration(ctx, 3, (16, 32), 'intensity'), ref, 'another field'),
                           (A.HologramRegistration(ctx, 3, (16, 16), 'magnitude'), ref, 'another field'),
                           (A.HologramRegistration(ctx, 3, (16, 16), 'intensity'), plain, "raw_data_type='magnitude'")):
        fm = A.MultiDistModel(device=ctx, common_vars_dict=dict(base, ctf_engine=eng, hologram_registration=reg, optimize_prj_affine=True),
                              raw_data_type='intensity')
        with pytest.raises(ValueError, match=what):
            fm._check(0, np.array([1.7]), None)
    ctx.close()


# ------------------------------------------------------------------------------------------------------------ the driver
def drv_kw(F, F26, tmp_path, dist, aff, **over):
    par = ast.literal_eval(str(F['drv/params']))
    _, kw = old_drv_kw(F26, tmp_path)
    assert np.array_equal(F26['drv/obj'], F['drv/obj']) and np.array_equal(F26['drv/data'], F['drv/data'])
    kw.update(fname=F['drv/data_warped' if aff else 'drv/data'][None], n_epochs=par['n_epochs'], learning_rate=par['learning_rate'],
              free_prop_cm=np.array(F['drv/model_dists' if dist else 'drv/dists_true']), optimize_ctf_lg_kappa=False,
              optimize_free_prop=dist, free_prop_learning_rate=par['free_prop_learning_rate'], ctf_free_prop=dist,
              optimize_prj_affine=aff, prj_affine_learning_rate=par['prj_affine_learning_rate'], ctf_prj_affine=aff)
    kw.update(over)
    return par, kw


def check_small(hist, t64, t32, lr, what):
    """|x - x64| <= 3 y + (updates so far) x (sp(|x64|) + 3 sp(lr)), sp the float32 spacing: the parameter lives in float32 here and
    in the run's precision in the reference, so every update stores it rounded (half a spacing at its value) and forms the Adam
    step, at most ``lr`` long, in float32 -- both moments, the root, the quotient and the product rounded once each, half a
    spacing of the step apiece.  The second term matters only for entries smaller than the step (matrix entries that start at 0).
    y is the yardstick |x32 - x64| of the reference's own float32 run: of the entry itself for a scalar or a vector of scalars
    (each distance has its own gradient sum), and for matrices [updates, D, 2, 3] the largest over the six entries of the same
    matrix at the same update -- they come out of one gradient kernel with one arithmetic, and a single entry of one float32 run
    can lie next to fp64 by chance (golden F32 'drv_both', update 4, matrix 1: 1.1e-9 on entry [1, 0], 2.3e-8 on entry [0, 0]), which says nothing about what float32 can keep there."""
    hist = np.asarray(hist, np.float64)
    assert hist.shape == t64.shape, (what, hist.shape, t64.shape)
    n = np.arange(1, len(t64) + 1).reshape((-1,) + (1,) * (t64.ndim - 1))
    sp = lambda a: np.spacing(np.abs(a).astype(np.float32)).astype(np.float64)
    y = np.abs(t32 - t64)
    if t64.ndim == 4:
        y = np.broadcast_to(y.max(axis=(2, 3), keepdims=True), y.shape)
    bound = 3 * y + n * (sp(t64) + 3 * sp(np.float64(lr)))
    bad = np.abs(hist - t64) > bound
    print(what, 'off by', np.abs(hist - t64).max(axis=0), 'bound', bound.max(axis=0), 'over the bound:',
          [(tuple(int(v) for v in i), float(np.abs(hist - t64)[tuple(i)]), float(bound[tuple(i)])) for i in np.argwhere(bad)])
    assert not bad.any(), (what, np.abs(hist - t64), bound)


@pytest.mark.parametrize('tag', ('drv_dist', 'drv_aff', 'drv_both'))
def test_driver_vs_reference(A, F, F26, tmp_path, tag):
    """The runs of golden F32 (b): losses, final object, the distances and matrices after every update; the distances move towards
    the truth, matrix 0 stays the identity, the matrices are written once per epoch."""
    dist, aff = tag != 'drv_aff', tag != 'drv_dist'
    par, kw = drv_kw(F, F26, tmp_path, dist, aff, save_intermediate=aff)
    st = A.reconstruct_ptychography(**kw)
    t = lambda p, k: F['%s/%s/%s' % (tag, p, k)]
    x64 = np.stack([t('fp64', 'delta'), t('fp64', 'beta')], -1).astype(np.float64)
    x32 = np.stack([t('fp32', 'delta'), t('fp32', 'beta')], -1).astype(np.float64)
    check_run(st, t('fp64', 'losses'), x64, x32, par['learning_rate'], tag)
    if dist:
        d64 = t('fp64', 'dists')
        check_small(st['free_prop_cm_history'], d64, t('fp32', 'dists'), par['free_prop_learning_rate'], tag + ' distances')
        assert np.array_equal(np.float32(st['free_prop_cm']), np.float32(st['free_prop_cm_history'][-1]))
        true, start = F['drv/dists_true'], F['drv/model_dists']
        # (four Adam steps of at most one learning rate each; the reference's fp64 run ends 2.4 to 4 of them nearer)
        assert (np.abs(st['free_prop_cm'] - true) < np.abs(start - true) - 2 * par['free_prop_learning_rate']).all()
    else:
        assert st['free_prop_cm_history'] is None and np.allclose(st['free_prop_cm'], F['drv/dists_true'])
    if aff:
        check_small(st['prj_affine_history'], t('fp64', 'theta'), t('fp32', 'theta'), par['prj_affine_learning_rate'], tag + ' matrices')
        hist = np.asarray(st['prj_affine_history'])
        assert np.array_equal(hist[:, 0], np.tile(np.float32(AR.IDENTITY), (len(hist), 1, 1)))                      # the pin
        assert np.abs(hist[-1, 1:] - AR.IDENTITY).max() > 2 * par['prj_affine_learning_rate']
        d = os.path.join(str(tmp_path), 'out', 'intermediate', 'prj_affine')
        assert sorted(os.listdir(d)) == ['prj_affine_%d.txt' % e for e in range(par['n_epochs'])]
        assert np.array_equal(np.float32(np.loadtxt(os.path.join(d, 'prj_affine_%d.txt' % (par['n_epochs'] - 1)))).reshape(3, 2, 3), hist[-1])
    else:
        assert st['prj_affine_history'] is None


TOMO = dict(free_prop_learning_rate=0.25, prj_affine_learning_rate=1e-3)


def tomo_prj(F30):
    """F30's driver holograms, those of distances 1 and 2 warped at every angle: the matrices have something to find."""
    return np.stack([AR.warp(a.astype(np.float64), WARP) for a in F30['drv/prj']]).astype(np.float32)


def tomo_kw(F30, tmp_path, **over):
    par, kw = tomo_drv_kw(F30, tmp_path)
    kw.update(fname=tomo_prj(F30), free_prop_cm=DR.round32(F30['drv/dists'] * OFF), optimize_free_prop=True, ctf_free_prop=True,
              optimize_prj_affine=True, ctf_prj_affine=True, **TOMO)
    kw.update(over)
    return par, kw


def test_tomography_run_vs_the_restatement(A, F30, tmp_path):
    """ctf_tomography with both keywords on F30's driver inputs, the holograms warped and the distances started 10 %, 8 % and 5 %
    off: against tests/ctf_dist_ref.reconstruct_tomo in fp64 (held to F30's own driver run by tests/test_ctf_dist_ref_vs_golden.py),
    its float32 run the yardstick -- losses and object by check_run, distances, matrices and kappa after every update by the rule
    for small parameters; the distances move towards the truth."""
    par, kw = tomo_kw(F30, tmp_path)
    n, N = par['n_theta'], par['N']
    st = A.reconstruct_ptychography(**kw)
    theta_ls = np.linspace(0, np.pi, n, dtype='float32')
    ref = lambda dt: DR.reconstruct_tomo(kw['fname'], F30['drv/obj'], kw['free_prop_cm'], CM.LG_KAPPA, theta_ls, CM.ENERGY_EV, CM.PSIZE_CM,
                                         n_epochs=par['n_epochs'], learning_rate=par['learning_rate'], optimize_free_prop=True,
                                         optimize_prj_affine=True, optimize_ctf_lg_kappa=True,
                                         ctf_lg_kappa_learning_rate=par['ctf_lg_kappa_learning_rate'], dtype=dt, **TOMO)
    r64, r32 = ref(np.float64), ref(np.float32)
    check_run(st, np.array(r64['losses']), r64['obj'], r32['obj'].astype(np.float64), par['learning_rate'], 'tomography')
    assert len(st['losses']) == par['n_epochs'] * n
    check_small(st['free_prop_cm_history'], r64['dists_trace'], r32['dists_trace'], TOMO['free_prop_learning_rate'], 'tomography distances')
    check_small(st['prj_affine_history'], r64['theta_trace'], r32['theta_trace'], TOMO['prj_affine_learning_rate'], 'tomography matrices')
    check_small(st['ctf_lg_kappa_history'], np.array(r64['lg_kappa_trace']), np.array(r32['lg_kappa_trace']),
                par['ctf_lg_kappa_learning_rate'], 'tomography kappa')
    hist = np.asarray(st['prj_affine_history'])
    assert np.array_equal(hist[:, 0], np.tile(np.float32(AR.IDENTITY), (len(hist), 1, 1)))                          # the pin
    assert np.abs(r64['theta_trace'][-1, 1:] - AR.IDENTITY).max() > 4 * TOMO['prj_affine_learning_rate']           # (the matrices do move)
    true, start = F30['drv/dists'], kw['free_prop_cm']
    print('distances', start, '->', st['free_prop_cm'], 'fp64', r64['dists_trace'][-1], 'truth', true)
    # (eight Adam steps of at most one learning rate each; the restatement's fp64 run decides how far they must have gone)
    moved = np.abs(start - true) - np.abs(r64['dists_trace'][-1] - true)
    assert (moved > 2 * TOMO['free_prop_learning_rate']).all(), moved
    assert (np.abs(st['free_prop_cm'] - true) < np.abs(start - true) - 2 * TOMO['free_prop_learning_rate']).all()


def test_tomography_resume(A, F30, tmp_path):
    """A run stopped after its first epoch and resumed from its checkpoint (distances, matrices and their moments travel under
    'free_prop_cm' / 'prj_affine_ls' and '..._moments') continues the uninterrupted one bit for bit."""
    par, kw = tomo_kw(F30, tmp_path, output_folder='whole')
    n = par['n_theta']
    whole = A.reconstruct_ptychography(**kw)
    hist = np.asarray(whole['free_prop_cm_history'], np.float64)
    common = dict(store_checkpoint=True, n_batch_per_checkpoint=1, output_folder='part')
    A.reconstruct_ptychography(**tomo_kw(F30, tmp_path, n_epochs=1, **common)[1])
    ck = os.path.join(str(tmp_path), 'part', 'checkpoint')
    assert [int(v) for v in np.loadtxt(os.path.join(ck, 'checkpoint.txt'))] == [0, n - 1]
    with open(os.path.join(ck, 'params_0'), 'rb') as f:
        saved = pickle.load(f)
    assert np.array_equal(np.float32(saved['free_prop_cm']).reshape(-1), np.float32(hist[n - 2]))
    assert len(saved['free_prop_cm_moments']) == 2 and len(saved['prj_affine_ls_moments']) == 2
    res = A.reconstruct_ptychography(**tomo_kw(F30, tmp_path, use_checkpoint=True, **common)[1])
    assert np.array_equal(res['losses'], whole['losses'][n - 1:])
    assert np.array_equal(res['delta'], whole['delta'])
    assert np.array_equal(np.asarray(res['free_prop_cm_history']), np.asarray(whole['free_prop_cm_history'])[n - 1:])
    assert np.array_equal(np.asarray(res['prj_affine_history']), np.asarray(whole['prj_affine_history'])[n - 1:])
    assert np.array_equal(res['free_prop_cm'], whole['free_prop_cm']) and np.array_equal(res['prj_affine_ls'], whole['prj_affine_ls'])


def test_driver_refusals(A, F, F26, tmp_path):
    """The new keywords' refusals by name, and the old refusals without them."""
    par, kw = drv_kw(F, F26, tmp_path, True, True)
    run = lambda **over: A.reconstruct_ptychography(**dict(kw, **over))
    for over, what in ((dict(ctf_free_prop=False), "forward_algorithm='ctf' with optimize_free_prop"),
                       (dict(ctf_prj_affine=False, ctf_free_prop=True), "forward_algorithm='ctf' with optimize_prj_affine"),
                       (dict(optimize_probe=True), "forward_algorithm='ctf' with optimize_probe"),
                       (dict(optimize_all_probe_pos=True), "forward_algorithm='ctf' with optimize_all_probe_pos"),
                       (dict(forward_algorithm='fresnel', optimize_ctf_lg_kappa=False), "ctf_free_prop with forward_algorithm='fresnel'"),
                       (dict(forward_algorithm='fresnel', optimize_ctf_lg_kappa=False, ctf_free_prop=False), "ctf_prj_affine with forward_algorithm='fresnel'"),
                       (dict(update_using_external_algorithm='ctf', ctf_direct_update=True), "update_using_external_algorithm='ctf' with ctf_free_prop"),
                       (dict(update_using_external_algorithm='ctf', ctf_direct_update=True, ctf_free_prop=False, optimize_free_prop=False),
                        "update_using_external_algorithm='ctf' with ctf_prj_affine")):
        with pytest.raises(NotImplementedError, match=what.replace('(', r'\(').replace(')', r'\)')):
            run(**over)

    class TwoRanks(object):
        """A communicator that reports two ranks: the refusal comes before anything is exchanged."""
        size, rank = 2, 0
        bcast_object = staticmethod(lambda v, root=0: v)
    with pytest.raises(NotImplementedError, match='ctf_free_prop with more than one rank'):
        run(comm=TwoRanks())
    with pytest.raises(NotImplementedError, match='ctf_prj_affine with more than one rank'):
        run(comm=TwoRanks(), ctf_free_prop=False, optimize_free_prop=False)
    no = {k: v for k, v in kw.items() if k not in ('ctf_free_prop', 'ctf_prj_affine')}
    with pytest.raises(NotImplementedError, match="forward_algorithm='ctf' with optimize_free_prop"):
        A.reconstruct_ptychography(**no)
    with pytest.raises(NotImplementedError, match="forward_algorithm='ctf' with optimize_prj_affine"):
        A.reconstruct_ptychography(**dict(no, optimize_free_prop=False))
