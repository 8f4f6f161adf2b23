"""The affine registration of measured holograms on the GPU (pytest -m gpu): adm_register.hip through adorym_amd.HologramRegistration
and the C ABI (adm_register_create / destroy / targets / grad), alone and in front of / behind the detector fan-out launch of a
streamed MultisliceEngine (multi-distance holography of a 3-D object with optimize_prj_affine).

Checkers: golden F29 (recorded from the reference with the data through w.affine_transform, tests/golden/gen_f29_multidist3d_affine.py)
and the NumPy restatement tests/multidist3d_affine_ref.py (tied to the reference by tests/test_multidist3d_affine_ref_vs_golden.py).
Prediction, loss, object and probe gradients: ms_matrix.GENERIC, as the fan-out tests judge them; the registered target:
GENERIC['pred'].  dL/dtheta of the free matrices against the reference: e <= 3 * (the reference's own fp32 distance from its fp64
run) + floor, floor = the fp32 restatement's own distance from fp64 (test_gpu_multidist3d_dist.py's rule); against the restatement:
e <= 3 * (the fp32 restatement's distance) + GENERIC['grad_abs'] under the cap GENERIC['grad'].  At the identity every sampling
point sits on a pixel centre and float32 and float64 see different one-sided derivatives: there the gradient is judged against
float32 arithmetic (the fp32 restatement, the reference's own fp32 run) under GENERIC['grad'], and the tests print the disagreement.
"""
import ast
import ctypes as C
import os

import numpy as np
import pytest

from tests import ms_matrix as MM
from tests import multidist3d_affine_ref as AR
from tests import test_gpu_multidist3d as MD
from oracle import adorym_oracle as O      # checker only

gpu = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, 'adorym_amd', 'csrc', 'adm_register.hip')
ENERGY_EV, PSIZE_CM = MD.ENERGY_EV, MD.PSIZE_CM
BARS = MM.GENERIC
rel = MM.rel


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
    return np.load(os.path.join(ROOT, 'tests', 'golden', 'F29_multidist3d_affine.npz'))


def f32(a):
    return np.ascontiguousarray(a, dtype=np.float32)


# ------------------------------------------------------------------------------------------- 1. the fixture's cases (the reference)
def fixture_case(F, name):
    names = [str(n) for n in F['kernel_cases']]
    sg, M, rdt = ast.literal_eval(str(F['kernel_case_params'][names.index(name)]))
    c = {k: F['%s/%s' % (name, k)] for k in ('obj', 'pos', 'probes', 'meas')}
    c.update(sign_convention=sg, raw_data_type=rdt, dists=[float(d) for d in F['kernel_dists_cm']], theta=F['kernel_theta'])
    return c


def launch_registered(A, ctx, eng, case, host_target=None):
    """targets() -> rotate -> the fan-out launch with the registered holograms as its target -> rotate_adjoint -> grad().  The
    registration engine holds one matrix per ENTRY (b * D + d takes matrix d); dL/dtheta is summed over the positions on the host.
    ``host_target``: that array is uploaded as the launch's target instead (no registration kernels run)."""
    obj, pos, probes, theta = case['obj'], case['pos'], case['probes'], case['theta']
    M, Py, Px = probes.shape
    B, D = len(pos), len(case['dists'])
    out = {}
    if host_target is None:
        reg = A.HologramRegistration(ctx, B * D, (Py, Px), case['raw_data_type'])
        d_data, d_theta = ctx.array(f32(np.abs(case['meas']))), ctx.array(f32(AR.per_entry(theta, B * D)))
        target = reg.targets(d_data, d_theta)
        out['target'] = target.get()
    else:
        target = np.asarray(host_target, np.float32)
    d_grad, d_gp = ctx.zeros(obj.shape), ctx.zeros((M, Py, Px, 2))
    eng.set_batch(pos, target)
    eng.rotate(ctx.array(obj, np.float32), None)
    eng.multislice(ctx.array(MM.c2(probes)), grad_probe=d_gp, want_pred=True)
    eng.rotate_adjoint(d_grad, None)
    out.update(grad=d_grad.get(), gprobe=MM.cplx(d_gp.get()), pred=eng.pred(), loss=eng.loss())
    if host_target is None:
        g = ctx.zeros((B * D, 2, 3))
        reg.grad(d_data, d_theta, eng.pred_device(), g)
        out['gtheta'] = g.get().astype(np.float64).reshape(B, D, 2, 3).sum(axis=0)
    return out


def ref_registered(case, dtype):
    phys = O.Physics(case['probes'].shape[-2:], ENERGY_EV, PSIZE_CM, free_prop_cm=case['dists'][0], sign_convention=case['sign_convention'])
    return AR.forward_adjoint_object(case['obj'].astype(np.float64), None, case['probes'].astype(np.complex128), case['pos'], case['meas'],
                                     phys, case['dists'], case['theta'], dtype, raw_data_type=case['raw_data_type'])


@gpu
@pytest.mark.parametrize('name', MD.FIXTURE_CASES)
def test_kernels_vs_reference(A, ctx, F, name):
    """reg_sample_kernel, reg_grad_kernel, reg_reduce_kernel around the fan-out launch: prediction, registered target, loss, object
    gradient, probe gradient and dL/dtheta against the reference's fp64 run with the data through w.affine_transform (field 12 x 20,
    S = 5, D = 3, B = 3; matrix 0 the identity, 1 and 2 rotation + scale + shift; one and two modes, both sign conventions, magnitude
    and intensity data).  Matrix 0 against the reference's own FLOAT32 gradient (see the module's docstring)."""
    case = fixture_case(F, name)
    eng = MD._engine(A, ctx, case, case['dists'])
    res = launch_registered(A, ctx, eng, case)
    eng.plan.close()
    e32 = F[name + '/err32']
    e = rel(res['pred'], F[name + '/pred'])
    print(name, 'pred %.2e (fp32 ref %.2e)' % (e, e32[0]))
    assert e < BARS['pred'], ('pred', e)
    e = rel(res['target'], F[name + '/target'])
    print(name, 'target %.2e (fp32 ref %.2e)' % (e, e32[5]))
    assert e < BARS['pred'], ('target', e)
    e = abs(res['loss'] / float(F[name + '/loss']) - 1)
    print(name, 'loss %.2e (fp32 ref %.2e)' % (e, e32[1]))
    assert e <= BARS['loss'], ('loss', e)
    for k, i in (('grad', 2), ('gprobe', 3)):
        e = rel(res[k], F['%s/%s' % (name, k)])
        print(name, '%s %.2e (fp32 ref %.2e)' % (k, e, e32[i]))
        assert e < BARS['grad'] and e <= 3 * e32[i] + BARS['grad_abs'], (k, e, e32[i])
    g64, g32 = ref_registered(case, 'float64')['gtheta'], ref_registered(case, 'float32')['gtheta']
    floor = rel(g32[1:], g64[1:])
    e = rel(res['gtheta'][1:], F[name + '/gtheta'][1:])
    print(name, 'dL/dtheta[1:] %.2e (fp32 ref %.2e, fp32 restatement %.2e)' % (e, e32[4], floor))
    assert e <= 3 * e32[4] + floor, ('dL/dtheta', e, e32[4], floor)
    for d in (1, 2):
        e = rel(res['gtheta'][d], F[name + '/gtheta'][d])
        assert e <= 3 * e32[6 + d] + rel(g32[d], g64[d]), ('dL/dtheta of matrix', d, e)
    # the identity: float32 arithmetic is the yardstick
    e_ref, e_rs = rel(res['gtheta'][0], F[name + '/gtheta32'][0]), rel(res['gtheta'][0], g32[0])
    print(name, 'dL/dtheta[0] (identity): vs the reference\'s fp32 run %.2e, vs the fp32 restatement %.2e; fp32 and fp64 disagree by %.2e '
          '(reference) / %.2e (restatement)' % (e_ref, e_rs, e32[6], rel(g32[0], g64[0])))
    assert e_ref < BARS['grad'] and e_rs < BARS['grad'], ('dL/dtheta of the identity', e_ref, e_rs)


# --------------------------------------------------------------------------------- 2. geometries, matrices, data (the restatement)
def kernel_constant(name):
    """#define NAME value, read from adm_register.hip."""
    import re
    with open(CSRC) as f:
        return int(re.search(r'^#define %s (\d+)\b' % name, f.read(), re.M).group(1))


GENERIC_THETA = [AR.matrix(0.03, 1.04, (0.05, -0.03)), AR.matrix(-0.02, 0.97, (-0.04, 0.06)), AR.matrix(0.011, 0.93, (0.021, 0.013))]
HALF = AR.matrix(0.01, 0.5, (0.013, -0.021))                       # magnification 0.5
ONE_AND_A_HALF = AR.matrix(0.01, 1.5, (0.5, -0.021))               # magnification 1.5, shifted: a third of the points beyond the right border
MIRROR = AR.matrix(0.02, 0.96, (0.03, 0.017), mirror=True)         # negative determinant


def thetas(D, first=None):
    t = [GENERIC_THETA[d % 3] for d in range(D)]
    if first is not None:
        t[0] = first
    return np.stack(t)


#   name: field, D, matrices, raw_data_type, a patch of exact zeros in the data
REG_CASES = {
    '12x20': ((12, 20), 3, thetas(3), 'magnitude', False),
    '2x2_smallest': ((2, 2), 2, np.stack([HALF, AR.matrix(0.1, 0.4, (0.05, -0.1))]), 'magnitude', False),
    '24x20_intensity': ((24, 20), 3, thetas(3), 'intensity', False),
    '33x70_ragged_rows': ((33, 70), 2, thetas(2), 'magnitude', False),
    '1025x12': ((1025, 12), 2, thetas(2), 'intensity', False),
    'D1': ((24, 20), 1, thetas(1), 'magnitude', False),
    'D64': ((24, 20), 64, thetas(64), 'magnitude', False),
    'partials_255': ((255, 256), 1, thetas(1), 'magnitude', False),        # one below reg_reduce_kernel's stride
    'partials_257': ((257, 256), 1, thetas(1), 'intensity', False),        # ... and one above
    'magnification_0.5': ((24, 20), 2, thetas(2, HALF), 'magnitude', False),
    'magnification_1.5_clamped': ((24, 20), 2, thetas(2, ONE_AND_A_HALF), 'intensity', False),
    'mirror': ((33, 70), 2, thetas(2, MIRROR), 'magnitude', False),
    'intensity_zero_patch': ((24, 20), 2, thetas(2), 'intensity', True),
}
_BUILT = {}


def holograms(r, D, Py, Px):
    """[D, Py, Px] float32 fringes of 6 to 40 pixels' period with a little roughness on top.  (Not white noise: a float32 coordinate
    of a 1025-row field is uncertain by 2e-5 pixels, and times the slope of white noise that alone exceeds the prediction bar.)"""
    y, x = np.mgrid[:Py, :Px].astype(np.float64)
    ly, lx = min(max(Py / 2., 6.), 40.), min(max(Px / 2., 6.), 40.)
    out = [0.6 + 0.25 * np.sin(2 * np.pi * (y / ly + r.uniform())) * np.cos(2 * np.pi * (x / lx + r.uniform())) + 0.03 * r.uniform(size=(Py, Px))
           for _ in range(D)]
    return np.stack(out).astype(np.float32)


def misregistered(r, data, theta, rdt):
    """Predictions [D, Py, Px] float32 that differ from the registered holograms the way a wrong registration does: the same data
    through matrices half a pixel off in shift and scale, 2 % noise.  (pred - target is then correlated with the image's slope
    and the sums of dL/dtheta add up; against predictions unrelated to the data they cancel over the fringes and fp32 has nothing
    left to be compared on.)"""
    Py, Px = data.shape[1:]
    off = np.array(theta, dtype=np.float64)
    off[:, 0, 2] += 1. / Px
    off[:, 1, 2] -= 1. / Py
    off[:, 0, 0] *= 1 + 1. / Px
    off[:, 1, 1] *= 1 - 1. / Py
    t = AR.register(data, off, rdt, 'float64')[1]
    return (t * (1 + 0.02 * r.standard_normal(t.shape))).astype(np.float32)


def built(name):
    """The case and the restatement's results on it (fp64 and fp32), computed once per process and left unchanged."""
    if name not in _BUILT:
        (Py, Px), D, theta, rdt, zeros = REG_CASES[name]
        r = np.random.default_rng([Py, Px, D, sorted(REG_CASES).index(name)])
        data = holograms(r, D, Py, Px)
        if rdt == 'intensity':
            data = (data ** 2).astype(np.float32)
        if zeros:
            data[:, 5:12, 4:11] = 0
        pred = misregistered(r, data, theta, rdt)
        case = dict(field=(Py, Px), D=D, theta=theta, raw_data_type=rdt, data=data, pred=pred)
        ref = {dt: (AR.register(data, theta, rdt, dt)[1], AR.affine_grad(data, theta, pred, rdt, dt)) for dt in ('float64', 'float32')}
        _BUILT[name] = (case, ref)
    return _BUILT[name]


def run_registration(A, ctx, case, grad_scale=1., g=None):
    reg = A.HologramRegistration(ctx, case['D'], case['field'], case['raw_data_type'])
    d_data, d_theta, d_pred = ctx.array(case['data']), ctx.array(f32(case['theta'])), ctx.array(case['pred'])
    target = reg.targets(d_data, d_theta).get()
    if g is None:
        g = ctx.zeros((case['D'], 2, 3))
    reg.grad(d_data, d_theta, d_pred, g, grad_scale=grad_scale)
    return target, g.get().astype(np.float64)


def test_the_cases_sit_on_both_sides_of_the_constants():
    nt, stride = kernel_constant('REG_NT'), kernel_constant('REG_RED_NT')
    blocks = lambda name: -(-int(np.prod(REG_CASES[name][0])) // nt)
    assert blocks('partials_255') == stride - 1 and blocks('partials_257') == stride + 1
    assert blocks('2x2_smallest') == 1 and blocks('12x20') == 1 and blocks('24x20_intensity') == 2       # one block, part of one, more than one
    assert 33 * 70 % nt != 0 and 70 % 64 != 0 and 1025 * 12 % nt != 0                                     # ragged rows and last blocks
    assert REG_CASES['D1'][1] == 1 and REG_CASES['D64'][1] == 64
    assert np.linalg.det(MIRROR[:, :2]) < 0 and abs(np.sqrt(np.linalg.det(HALF[:, :2])) - 0.5) < 1e-3
    # magnification 1.5 with the shift: a third of the sampling points lie beyond the right border (their gradient is zero)
    X = np.linspace(-1, 1, 20) * 19 / 20
    Y = np.linspace(-1, 1, 24) * 23 / 24
    gx = ONE_AND_A_HALF[0, 0] * X[None] + ONE_AND_A_HALF[0, 1] * Y[:, None] + ONE_AND_A_HALF[0, 2]
    ix = ((gx + 1) * 20 - 1) / 2
    assert 0.28 < np.mean(ix >= 19) < 0.4
    case = built('intensity_zero_patch')[0]
    assert np.count_nonzero(case['data'] == 0) == case['D'] * 49


@pytest.mark.parametrize('name', list(REG_CASES))
def test_the_fp32_restatement_is_a_yardstick_for_every_admitted_case(name):
    """CPU: every case of the geometry table has the fp32 restatement's dL/dtheta within 1e-2 of the fp64 one (and everything
    finite), or it is no case."""
    _, ref = built(name)
    e = rel(ref['float32'][1], ref['float64'][1])
    assert np.all(np.isfinite(ref['float64'][1])) and np.all(np.isfinite(ref['float32'][1])) and e < 1e-2, (name, e)
    assert np.all(np.abs(ref['float64'][1]).reshape(len(ref['float64'][1]), -1).max(axis=1) > 0)


@gpu
@pytest.mark.parametrize('name', list(REG_CASES))
def test_geometries_vs_restatement(A, ctx, name):
    """reg_sample_kernel, reg_grad_kernel, reg_reduce_kernel over the fields (the smallest, odd, ragged against waves and blocks, 1025
    rows), D = 1 and 64, both sides of the reduce kernel's stride, magnifications 0.5 and 1.5 (clamped points), a mirror, both data
    types and a patch of exact zeros: the registered target and dL/dtheta against the fp64 restatement."""
    case, ref = built(name)
    target, g = run_registration(A, ctx, case)
    (t64, g64), (t32, g32) = ref['float64'], ref['float32']
    e_t = rel(target, t64)
    e, e32 = rel(g, g64), rel(g32, g64)
    print(name, 'target %.2e (fp32 restatement %.2e)  dL/dtheta %.2e (fp32 restatement %.2e)' % (e_t, rel(t32, t64), e, e32))
    assert np.all(np.isfinite(target)) and e_t < BARS['pred'], (name, 'target', e_t)
    assert np.all(np.isfinite(g)) and e < BARS['grad'] and e <= 3 * e32 + BARS['grad_abs'], (name, 'dL/dtheta', e, e32)


@gpu
def test_grad_scale_scales_the_gradient(A, ctx):
    case, ref = built('12x20')
    _, g = run_registration(A, ctx, case, grad_scale=0.25)
    assert rel(g, 0.25 * ref['float64'][1]) < BARS['grad']


# ------------------------------------------------------------------------------------------ 3. the identity
@gpu
@pytest.mark.parametrize('field,rdt', [((24, 20), 'magnitude'), ((33, 70), 'intensity'), ((2, 2), 'magnitude')])
def test_identity_matrices(A, ctx, field, rdt):
    """reg_grad_kernel at the identity, where every sampling point sits on a pixel centre: against the fp32 restatement, which
    reproduces torch's float32 roundings of the coordinates.  Where fp32 and fp64 agree to 1e-2 the 3x rule against fp64 holds as
    well; where they do not, the test says so and float32 alone is the yardstick, under GENERIC['grad']."""
    D = 3
    r = np.random.default_rng([field[0], field[1], 31])
    data = holograms(r, D, *field)
    data = (data ** 2).astype(np.float32) if rdt == 'intensity' else data
    theta = np.tile(AR.IDENTITY, (D, 1, 1))
    t64 = AR.register(data, theta, rdt, 'float64')[1]
    pred = misregistered(r, data, theta, rdt)
    case = dict(field=field, D=D, theta=theta, raw_data_type=rdt, data=data, pred=pred)
    target, g = run_registration(A, ctx, case)
    g64, g32 = AR.affine_grad(data, theta, pred, rdt, 'float64'), AR.affine_grad(data, theta, pred, rdt, 'float32')
    assert rel(target, t64) < BARS['pred']
    if field == (2, 2):
        # both points of a 2-pixel line are AT the borders: no gradient passes (clip_coordinates_set_grad)
        assert np.all(g == 0) and np.all(g64 == 0) and np.all(g32 == 0)
        return
    dis = rel(g32, g64)
    e32, e64 = rel(g, g32), rel(g, g64)
    if dis <= 1e-2:
        print(field, rdt, 'identity: fp32 and fp64 restatements agree to %.2e; vs fp64 %.2e, vs fp32 %.2e' % (dis, e64, e32))
        assert e64 < BARS['grad'] and e64 <= 3 * dis + BARS['grad_abs'], (e64, dis)
    else:
        print(field, rdt, 'identity: the fp32 and fp64 restatements DISAGREE by %.2e (one-sided derivatives on pixel centres): judged '
              'against the fp32 restatement alone; vs fp32 %.2e, vs fp64 %.2e' % (dis, e32, e64))
    assert e32 < BARS['grad'], (e32, dis)


# ------------------------------------------------------------------------------------------ 4. bit for bit
@gpu
def test_same_bits_twice_and_accumulation(A, ctx):
    """The same call twice gives the same dL/dtheta bits; a second call into the same buffer gives exactly twice the first (+=)."""
    for name in ('33x70_ragged_rows', 'partials_257', 'D64'):
        case, _ = built(name)
        t1, g1 = run_registration(A, ctx, case)
        t2, g2 = run_registration(A, ctx, case)
        assert np.array_equal(t1, t2) and np.array_equal(g1, g2) and np.all(g1 != 0), name
        buf = ctx.zeros((case['D'], 2, 3))
        run_registration(A, ctx, case, g=buf)
        _, twice = run_registration(A, ctx, case, g=buf)
        assert np.array_equal(twice, 2 * g1), name


@gpu
def test_the_registration_changes_no_other_bit(A, ctx, F):
    """A launch whose target came from targets() and a launch whose target is that same array downloaded and handed in from the
    host: prediction, loss, object gradient and probe gradient are bit-identical."""
    case = fixture_case(F, 'm2_p1_intensity')
    eng = MD._engine(A, ctx, case, case['dists'])
    a = launch_registered(A, ctx, eng, case)
    b = launch_registered(A, ctx, eng, case, host_target=a['target'])
    eng.plan.close()
    for k in ('pred', 'loss', 'grad', 'gprobe'):
        assert np.array_equal(np.asarray(a[k]), np.asarray(b[k])), k


# ------------------------------------------------------------------------------------------ 5. refusals
@gpu
def test_abi_refusals(A, ctx):
    from adorym_amd._lib import check
    lib = ctx.lib
    h = C.c_void_p()
    with pytest.raises(ValueError, match='adm_register_create: null argument'):
        check(lib.adm_register_create(None, 2, 8, 8, 0, C.byref(h)))
    with pytest.raises(ValueError, match='adm_register_create: null argument'):
        check(lib.adm_register_create(ctx.handle, 2, 8, 8, 0, None))
    for ny, nx in ((1, 8), (8, 1), (2049, 8), (8, 2049), (0, 0)):
        with pytest.raises(NotImplementedError, match=r'adm_register_create: field sizes must be in \[2, 2048\]'):
            check(lib.adm_register_create(ctx.handle, 2, ny, nx, 0, C.byref(h)))
    for n in (0, -1, 65):
        with pytest.raises(ValueError, match=r'adm_register_create: n_dists must be in \[1, 64\]'):
            check(lib.adm_register_create(ctx.handle, n, 8, 8, 0, C.byref(h)))
    assert not h.value
    check(lib.adm_register_create(ctx.handle, 2, 8, 8, 1, C.byref(h)))
    data, theta, out, g = ctx.zeros((2, 8, 8)), ctx.array(f32(thetas(2))), ctx.zeros((2, 8, 8)), ctx.zeros((2, 2, 3))
    for args in ((None, data.ptr, theta.ptr, out.ptr), (h, None, theta.ptr, out.ptr), (h, data.ptr, None, out.ptr), (h, data.ptr, theta.ptr, None)):
        with pytest.raises(ValueError, match='adm_register_targets: null argument'):
            check(lib.adm_register_targets(*args))
    full = (h, data.ptr, theta.ptr, out.ptr, 1., g.ptr)
    for i in (0, 1, 2, 3, 5):
        with pytest.raises(ValueError, match='adm_register_grad: null argument'):
            check(lib.adm_register_grad(*(full[:i] + (None,) + full[i + 1:])))
    check(lib.adm_register_destroy(h))
    check(lib.adm_register_destroy(None))


@gpu
def test_engine_refusals(A, ctx):
    reg = A.HologramRegistration(ctx, 2, (8, 12), 'magnitude')
    data, theta, g = ctx.zeros((2, 8, 12)), ctx.array(f32(thetas(2))), ctx.zeros((2, 2, 3))
    assert reg.targets(data, theta).shape == (2, 8, 12)
    with pytest.raises(ValueError, match=r'data must be float32 \[2, 8, 12\]'):
        reg.targets(ctx.zeros((3, 8, 12)), theta)
    with pytest.raises(ValueError, match=r'affine must be float32 \[2, 2, 3\]'):
        reg.targets(data, ctx.zeros((2, 3, 3)))
    with pytest.raises(ValueError, match=r'data must be float32'):
        reg.targets(ctx.array(np.zeros((2, 8, 12), np.int32)), theta)
    with pytest.raises(TypeError, match='affine must be a DeviceArray'):
        reg.targets(data, thetas(2))
    with pytest.raises(ValueError, match=r'pred must be float32 \[2, 8, 12\]'):
        reg.grad(data, theta, ctx.zeros((2, 8, 13)), g)
    with pytest.raises(ValueError, match=r'grad_affine must be float32 \[2, 2, 3\]'):
        reg.grad(data, theta, data, ctx.zeros((2, 6, 2)))
    with pytest.raises(ValueError, match="raw_data_type must be 'magnitude' or 'intensity'"):
        A.HologramRegistration(ctx, 2, (8, 12), 'counts')
    with pytest.raises(ValueError, match='adm_register_create: n_dists must be in'):
        A.HologramRegistration(ctx, 65, (8, 12))
    with pytest.raises(NotImplementedError, match='adm_register_create: field sizes must be in'):
        A.HologramRegistration(ctx, 2, (8, 4096))
