"""The contrast-transfer-function model of a 3-D object on the GPU (pytest -m gpu): MultiDistModel with forward_algorithm='ctf',
two_d_mode=False and a RotatedProjector against golden F30 (the reference in fp64, its own fp32 run as the yardstick), and
ProjectionEngine(fused_rotation=True) against the fp64 restatement under the bars of tests/test_gpu_projection.py.

Bars (tests/ctf_matrix.BARS, the rule of tests/test_gpu_ctf.py): loss 5e-5, prediction 5e-6, delta gradient 2e-4 of the norm and
within 3 x the float32 reference's own distance from fp64, kappa gradient max(2e-3, 3 x the float32 reference's).  dL/dbeta is
exactly zero."""
import os

import numpy as np
import pytest

from tests import ctf_matrix as CM
from tests import ctf_tomo_ref as TR
from tests import test_gpu_projection as TP

pytestmark = pytest.mark.gpu
BARS = CM.BARS
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden', 'F30_ctf_tomo.npz')


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
def F():
    return np.load(GOLDEN)


def build_model(A, ctx, c, **over):
    Y, X, Z = c['size']
    eng = A.CTFEngine(ctx, (Y, X), c['nd'], CM.ENERGY_EV, CM.PSIZE_CM, raw_data_type='intensity')
    rp = A.RotatedProjector(ctx, c['size'])
    tables = {}

    def rotation_tables(i):
        if i not in tables:
            tables[i] = A.RotationTable(ctx, c['size'], c['theta'])
        return tables[i]
    cv = dict(engine=None, ctf_engine=eng, ctf_projector=rp, forward_algorithm='ctf', two_d_mode=False, unknown_type='delta_beta',
              optimize_ctf_lg_kappa=True, prj=c['data'][None], n_probe_modes=1, safe_zone_width=0, rotation_tables=rotation_tables)
    cv.update(over)
    return A.MultiDistModel(device=ctx, common_vars_dict=cv, raw_data_type='intensity'), rp


def model_args(c):
    return dict(probe_real=None, probe_imag=None, probe_defocus_mm=0., probe_pos_offset=None, this_i_theta=0, this_pos_batch=np.zeros((1, 2)),
                prj=c['data'][None], probe_pos_correction=None, this_ind_batch=np.array([0]), free_prop_cm=c['dists'], safe_zone_width=0,
                prj_affine_ls=None, ctf_lg_kappa=np.array([c['lg_kappa']]), prj_pos_offset=None)


@pytest.mark.parametrize('name', list(TR.CASES))
def test_model_vs_reference(A, ctx, F, name):
    """predict, the loss function and loss_and_gradients of one angle against the reference's fp64 run."""
    c = TR.inputs(name)
    Y, X, Z = c['size']
    fm, rp = build_model(A, ctx, c)
    args = model_args(c)
    obj = ctx.array(c['obj'])
    o = {k: F['%s/%s' % (name, k)] for k in ('pred', 'grad')}
    o_loss, o_gk, e32 = float(F[name + '/loss']), float(F[name + '/gkappa']), F[name + '/err32']
    pred = fm.predict(obj, **args)
    assert pred.shape == (c['nd'], Y, X)
    e = CM.rel(pred, o['pred'])
    print('%s: pred %.2e (fp32 reference %.2e, bar %.0e)' % (name, e, e32[0], BARS['pred']))
    assert e < BARS['pred']
    e = abs(fm.get_loss_function()(obj, **args) / o_loss - 1)
    print('%s: loss %.2e (fp32 reference %.2e)' % (name, e, e32[1]))
    assert e < BARS['loss']
    i_k = fm.get_argument_index('ctf_lg_kappa')
    for init in (False, True):
        # into zeros ('+='), and into a buffer that holds garbage (_init_grad: '=')
        grad = ctx.zeros(c['obj'].shape) if not init else ctx.array(np.full(c['obj'].shape, 7., np.float32))
        g = fm.loss_and_gradients([0, i_k], grad, obj, _init_grad=init, **args)
        assert g[0] is grad
        what = '%s (%s)' % (name, 'overwriting' if init else 'accumulating')
        assert abs(fm.current_loss / o_loss - 1) < BARS['loss'], what
        got = grad.get()
        assert not got[..., 1].any(), what + ': dL/dbeta is not exactly zero'
        e, r32 = CM.rel(got[..., 0], o['grad'][..., 0]), e32[2]
        print('%s: grad_delta %.2e (fp32 reference %.2e, bar %.0e and 3x)' % (what, e, r32, BARS['grad']))
        assert r32 < BARS['grad'] / 3, (what, 'ill-conditioned case', r32)
        assert e < BARS['grad'] and e <= 3 * r32, (what, 'grad_delta', e, r32)
        e, r32 = abs(float(g[1].get()[0]) / o_gk - 1), e32[3]
        print('%s: grad_lg_kappa %.2e (fp32 reference %.2e, bar %.1e)' % (what, e, r32, max(BARS['gkappa'], 3 * r32)))
        assert e < max(BARS['gkappa'], 3 * r32), (what, 'grad_lg_kappa', e, r32)
    rp.close()


def test_object_regulariser_is_added(A, ctx):
    """An L1 term on delta, as on the other 3-D paths: value into the loss, gradient into grad_obj."""
    name = 'y32x16z8_t0.3_d2'
    c = TR.inputs(name)
    r = TR.forward_adjoint(c)
    fm, rp = build_model(A, ctx, c)
    alpha = 1e-3
    fm.add_regularizers([A.L1Regularizer(alpha, 0, unknown_type='delta_beta')])
    obj, grad = ctx.array(c['obj']), ctx.zeros(c['obj'].shape)
    fm.loss_and_gradients([0], grad, obj, **model_args(c))
    d = c['obj'][..., 0].astype(np.float64)
    l1 = alpha * np.mean(np.abs(d))
    assert abs(fm.current_loss - (r['loss'] + l1)) < 1e-4 * l1
    # d |x| / dx = sign(x) over the number of voxels: delta's gradient moves by that, beta's stays zero (alpha_b = 0)
    extra = grad.get()[..., 0].astype(np.float64) - r['grad'][..., 0]
    assert CM.rel(extra, alpha * np.sign(d) / d.size) < 1e-2
    assert not grad.get()[..., 1].any()
    rp.close()


def test_model_refusals(A, ctx):
    """Without a projector the 3-D object stays refused; with one, everything _check_ctf refuses stays refused by name, and so are
    rotate_out_of_loop, several ranks and a field the CTF engine does not take."""
    c = TR.inputs('y16x16z16_t0_d2')
    fm, rp = build_model(A, ctx, c, ctf_projector=None)
    with pytest.raises(NotImplementedError, match="forward_algorithm='ctf' with two_d_mode=False"):
        fm._check(0, np.array([1.7]), None)
    for over, what in ((dict(unknown_type='real_imag'), 'real_imag'), (dict(n_probe_modes=3), 'n_probe_modes != 1'),
                       (dict(optimize_probe=True), 'optimize_probe'), (dict(optimize_free_prop=True), 'optimize_free_prop'),
                       (dict(optimize_prj_affine=True), 'optimize_prj_affine'), (dict(optimize_all_probe_pos=True), 'optimize_all_probe_pos'),
                       (dict(safe_zone_width=3), 'safe_zone_width > 0'), (dict(rotate_out_of_loop=True), 'rotate_out_of_loop'),
                       (dict(n_ranks=2), 'more than one rank')):
        fm, rp2 = build_model(A, ctx, c, **over)
        with pytest.raises(NotImplementedError, match="forward_algorithm='ctf' with .*" + what):
            fm._check(over.get('safe_zone_width', 0), np.array([1.7]), None)
        rp2.close()
    with pytest.raises(NotImplementedError, match='LSQ'):
        A.MultiDistModel(loss_function_type='poisson', device=ctx, common_vars_dict=dict(engine=None, ctf_engine=fm.ctf, ctf_projector=rp,
                                                                                       forward_algorithm='ctf', two_d_mode=False))
    other = A.RotatedProjector(ctx, (16, 32, 4))
    fm, rp3 = build_model(A, ctx, c, ctf_projector=other)
    with pytest.raises(NotImplementedError, match='powers of two'):
        fm._check(0, np.array([1.7]), None)
    for p in (rp, rp3, other):
        p.close()


def test_projection_engine_fused_rotation(A, ctx):
    """ProjectionEngine(fused_rotation=True) on the rotated case of tests/test_gpu_projection.py -- 37 x 53 x 7, two modes, a Fresnel
    detector and a beamstop -- under that file's bars against the fp64 restatement; the default engine printed beside it."""
    case = TP.make_case(2561, (37, 53, 7), (12, 20), 5, M=2, free_prop=2e-4, sg=-1, beamstop=True)
    theta = 0.6
    fused = TP.run_engine(A, ctx, case, theta=theta, fused_rotation=True)
    plain = TP.run_engine(A, ctx, case, theta=theta)
    r64, r32 = TP.run_ref(case, 'float64', theta), TP.run_ref(case, 'float32', theta)
    TP.check_3x(fused, r64, TP.yardstick(r32, r64), 'fused rotation')
    assert np.abs(fused['grad']).max() > 0
    print('fused against the default engine: pred %.2e, grad %.2e, loss %.2e' % (
        TP.rel(fused['pred'], plain['pred']), TP.rel(fused['grad'], plain['grad']), abs(fused['loss'] / plain['loss'] - 1)))


def test_fused_projection_engine_builds_no_volume_and_refuses_bare_coordinates(A, ctx):
    """fused_rotation=True: no volume engine and none of its [Z] buffers; the back-rotation takes a RotationTable or None and
    refuses a bare coordinate array by name (the default engine would scatter with atomics there)."""
    from oracle import adorym_oracle as O
    size = (20, 24, 6)
    eng = A.ProjectionEngine(ctx, size, (16, 16), np.array([[-2, 3]]), TP.ENERGY_EV, TP.PSIZE_CM, fused_rotation=True)
    assert eng.volume is None and eng.obj_rot is None and eng.grad_rot is None
    assert eng.plan.obj_size == size and eng.plan.pads == eng.slab.plan.pads and eng.cacheless_plan() is eng.plan
    bare = ctx.array(np.ascontiguousarray(O.rotation_coords(size, np.float32(0.4))).view(np.uint16))
    with pytest.raises(NotImplementedError, match='bare coordinate array'):
        eng.rotate_adjoint(ctx.zeros(size + (2,)), bare)
    eng.close()
