"""The options of a streamed plan that exclude one another -- slice positions, exit-wave shifts, probe shifts and the detector
fan-out (host kernels or device distances) -- as a matrix (pytest -m gpu): every ordered pair of their setters through the C ABI,
and the same pairs as engine options and as arguments of ``MultisliceEngine.multislice``.  Only setters and refusals: no kernel
is launched.  What is accepted and what is refused, and with which code, is read off the setters of adm_api.hip and the checks
of propagate.py as they stood before the table of options existed."""
import itertools

import numpy as np
import pytest

from adorym_amd import _lib

pytestmark = pytest.mark.gpu
ENERGY_EV, PSIZE_CM = 8000., 1e-6
OBJ, PROBE = (26, 26, 3), (17, 13)          # (the smallest streamed field of tests/test_gpu_prj_offset.py; three slices)
GEO = (0.155, 10., 10.)
NOUN = {'slice_positions': 'slice positions', 'exit_shift': 'exit-wave shifts', 'probe_shift': 'probe shifts',
        'detector_fanout': 'detector fan-out', 'fanout_distances': 'detector fan-out'}
FANOUT = ('detector_fanout', 'fanout_distances')


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
def setters(ctx):
    """name -> (on, off): calls that take a plan handle and return the setter's code."""
    lib = ctx.lib
    z = ctx.array(np.array([0., 1e-3, 2e-3], np.float32))
    d = ctx.array(np.array([1e-4, 2e-4], np.float32))
    re, im = np.ones((2,) + PROBE, np.float32), np.zeros((2,) + PROBE, np.float32)
    fan_off = lambda h: lib.adm_plan_set_detector_fanout(h, 0, None, None)
    return {'slice_positions': (lambda h: lib.adm_plan_set_slice_positions(h, z.ptr, 3, *GEO),
                                lambda h: lib.adm_plan_set_slice_positions(h, None, 0, *GEO)),
            'exit_shift': (lambda h: lib.adm_plan_set_exit_shift(h, 1), lambda h: lib.adm_plan_set_exit_shift(h, 0)),
            'probe_shift': (lambda h: lib.adm_plan_set_probe_shift(h, 1), lambda h: lib.adm_plan_set_probe_shift(h, 0)),
            'detector_fanout': (lambda h: lib.adm_plan_set_detector_fanout(h, 2, re.ctypes.data, im.ctypes.data), fan_off),
            'fanout_distances': (lambda h: lib.adm_plan_set_fanout_distances(h, d.ptr, 2, *GEO), fan_off)}


def _plan(A, ctx, streamed):
    one = np.ones(PROBE, complex)
    return A.Plan(ctx, OBJ, PROBE, ((0, 0), (0, 0)), 1.0, one, det_mode=_lib.DET_FRESNEL, h_free=one, streamed=streamed)


def _message(ctx):
    return ctx.lib.adm_last_error().decode()


@pytest.mark.parametrize('first,second', list(itertools.permutations(NOUN, 2)))
def test_every_ordered_pair_of_setters(A, ctx, setters, first, second):
    plan = _plan(A, ctx, True)
    h = plan.handle
    assert setters[first][0](h) == _lib.ADM_OK, _message(ctx)
    rc = setters[second][0](h)
    if first in FANOUT and second in FANOUT:         # (the two fan-out setters replace each other)
        assert rc == _lib.ADM_OK, _message(ctx)
    else:
        msg = _message(ctx)
        assert rc == _lib.ADM_ERR_UNSUPPORTED, (rc, msg)
        assert msg.startswith('adm_plan_set_%s: ' % second) and NOUN[first] in msg and NOUN[second] in msg, msg
        assert setters[first][1](h) == _lib.ADM_OK, _message(ctx)          # the first switched off: the second is accepted
        assert setters[second][0](h) == _lib.ADM_OK, _message(ctx)
    plan.close()


def test_plans_of_the_other_kind(A, ctx, setters):
    """A one-workgroup plan takes none of the five and takes several detector kernels; a streamed plan takes one detector kernel."""
    re, im = np.ones((2,) + PROBE, np.float32), np.zeros((2,) + PROBE, np.float32)
    kernels = lambda h, n: ctx.lib.adm_plan_set_detector_kernels(h, n, re.ctypes.data, im.ctypes.data)
    lds = _plan(A, ctx, False)
    for name in NOUN:
        assert setters[name][0](lds.handle) == _lib.ADM_ERR_UNSUPPORTED, name
        msg = _message(ctx)
        assert msg.startswith('adm_plan_set_%s: ' % name) and NOUN[name] in msg and 'streamed plan' in msg, msg
    assert kernels(lds.handle, 2) == _lib.ADM_OK, _message(ctx)
    lds.close()
    st = _plan(A, ctx, True)
    assert kernels(st.handle, 2) == _lib.ADM_ERR_UNSUPPORTED and _message(ctx).startswith('adm_plan_set_detector_kernels: ')
    assert kernels(st.handle, 1) == _lib.ADM_OK, _message(ctx)
    st.close()


# ------------------------------------------------------------------------------------------------------ the engine's options
POS = np.array([(0, 0), (3, 5)])
DISTS = [1e-4, 2e-4]
SEQUENCE = 'sequence of detector distances'
OPTION_KW = {'detector_fanout': dict(detector_fanout=True, free_prop_cm=DISTS, streamed=True), 'exit_shift': dict(exit_shift=True),
             'probe_shift': dict(probe_shift=True), 'slice_pos_cm': dict(slice_pos_cm=[0., 1e-3, 2e-3]), SEQUENCE: dict(free_prop_cm=DISTS)}


def _engine(A, ctx, **kw):
    return A.MultisliceEngine(ctx, OBJ, PROBE, POS, ENERGY_EV, PSIZE_CM, max_batch=2, **kw)


@pytest.mark.parametrize('a,b', list(itertools.combinations(list(OPTION_KW)[:4], 2)) + [(SEQUENCE, o) for o in list(OPTION_KW)[1:4]])
def test_engine_options_exclude_one_another(A, ctx, a, b):
    with pytest.raises(NotImplementedError) as e:
        _engine(A, ctx, **dict(OPTION_KW[a], **OPTION_KW[b]))
    assert a in str(e.value) and b in str(e.value) and 'not implemented' in str(e.value), str(e.value)


def test_call_time_arguments_exclude_one_another(A, ctx):
    """multislice() refuses each pair on the smallest engine that takes the first of the two, before anything is launched."""
    s, probe = ctx.zeros((2, 2)), ctx.zeros((1,) + PROBE + (2,))
    per_position = ctx.zeros((2, 1) + PROBE + (2,))
    arg = {'shifts': dict(shifts=s), 'probes_b': dict(probes_b=per_position), 'exit_shifts': dict(exit_shifts=s),
           'grad_probe': dict(grad_probe=ctx.zeros((1,) + PROBE + (2,)))}
    cases = [('exit_shifts', dict(exit_shift=True), arg['exit_shifts'], ('shifts', 'probes_b'), NotImplementedError),
             ('exit_shifts', OPTION_KW['slice_pos_cm'], arg['exit_shifts'], ('slice_pos_cm',), NotImplementedError),
             ('detector_fanout', OPTION_KW['detector_fanout'], {}, ('shifts', 'probes_b', 'exit_shifts'), NotImplementedError),
             ('probes_b', {}, arg['probes_b'], ('shifts', 'grad_probe'), ValueError)]
    for first, engine_kw, first_kw, others, refusal in cases:
        eng = _engine(A, ctx, **engine_kw)
        eng.set_batch(POS, np.ones((2 * eng.det_per_pos,) + PROBE, np.float32))
        for other in others:
            with pytest.raises(refusal) as e:
                eng.multislice(probe, **dict(first_kw, **arg.get(other, {})))
            assert first in str(e.value) and other in str(e.value), (first, other, str(e.value))
        eng.plan.close()
