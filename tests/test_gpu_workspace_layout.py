"""adm_plan_workspace_bytes over plans of every kind (tuned, any-size, streamed, sparse; one and several modes; padded frames with
an odd and an even number of pixels; an odd number of column groups): linear in the batch, which MultisliceEngine.round_cap
assumes, and equal to a recorded table, so that a change of the workspace layout (ws_layout, adm_api.hip) is a deliberate edit of
that table -- a different size changes how a budgeted batch is split into rounds, hence the order of additions (pytest -m gpu)."""
import numpy as np
import pytest

from adorym_amd._lib import check

pytestmark = pytest.mark.gpu

# name: (probe, n_modes, streamed, slice positions, obj_size, pads)
PLANS = {
    'tuned 72': ((72, 72), 1, False, 0, (120, 90, 16), ((5, 6), (3, 4))),
    'tuned 64, 5 modes': ((64, 64), 5, False, 0, (100, 100, 12), ((0, 0), (0, 0))),
    'any-size 40x24': ((40, 24), 1, False, 0, (70, 45, 9), ((3, 4), (2, 4))),
    'any-size 40x24, 3 modes': ((40, 24), 3, False, 0, (70, 45, 9), ((3, 4), (2, 4))),
    'streamed 256x256': ((256, 256), 1, True, 0, (300, 301, 8), ((0, 0), (0, 0))),
    'streamed 1025x132, 3 modes': ((1025, 132), 3, True, 0, (1100, 200, 4), ((0, 0), (0, 0))),
}
for S_ in (1, 2, 8):
    PLANS.update({
        'sparse S=%d 256x256, odd frame' % S_: ((256, 256), 1, True, S_, (299, 300, S_), ((1, 1), (2, 1))),
        'sparse S=%d 256x256, even frame' % S_: ((256, 256), 1, True, S_, (300, 303, S_), ((0, 0), (0, 0))),
        'sparse S=%d 1025x132, 3 modes, odd frame, 33 column groups' % S_: ((1025, 132), 3, True, S_, (1101, 201, S_), ((0, 0), (0, 0))),
        'sparse S=%d 40x24, 2 modes, even frame, 3 column groups' % S_: ((40, 24), 2, True, S_, (78, 51, S_), ((0, 0), (0, 0))),
    })

TABLE_BATCHES = (1, 2, 7, 300)

# adm_plan_workspace_bytes(plan, b) for b in TABLE_BATCHES as the commit before ws_layout computed them: its chain of offset functions,
# evaluated in a host program on plans filled in like these
RECORDED = {
    'tuned 72': [4787148, 6270412, 13686732, 448283084],
    'tuned 64, 5 modes': [5287040, 7974016, 21408896, 808692864],
    'any-size 40x24': [1167004, 1312924, 2042524, 44797084],
    'any-size 40x24, 3 modes': [1343644, 1666204, 3279004, 97789084],
    'streamed 256x256': [32915376, 42352688, 89539248, 2854671664],
    'streamed 1025x132, 3 modes': [84260196, 111320328, 246620988, 8175239664],
    'sparse S=1 256x256, odd frame': [25810124, 27907404, 38393804, 652896844],
    'sparse S=1 256x256, even frame': [25731344, 27828624, 38315024, 652818064],
    'sparse S=1 1025x132, 3 modes, odd frame, 33 column groups': [71609656, 85680988, 156037648, 4278937924],
    'sparse S=1 40x24, 2 modes, even frame, 3 column groups': [1103476, 1172608, 1518268, 21773944],
    'sparse S=2 256x256, odd frame': [27383248, 31053648, 49405648, 1124832848],
    'sparse S=2 256x256, even frame': [27304464, 30974864, 49326864, 1124754064],
    'sparse S=2 1025x132, 3 modes, odd frame, 33 column groups': [79187256, 100836184, 209080824, 6552216728],
    'sparse S=2 40x24, 2 modes, even frame, 3 column groups': [1141928, 1249512, 1787432, 33309544],
    'sparse S=8 256x256, odd frame': [36821968, 49931088, 115476688, 3956448848],
    'sparse S=8 256x256, even frame': [36743184, 49852304, 115397904, 3956370064],
    'sparse S=8 1025x132, 3 modes, odd frame, 33 column groups': [124652808, 191767288, 527339688, 20191882328],
    'sparse S=8 40x24, 2 modes, even frame, 3 column groups': [1372616, 1710888, 3402248, 102515944],
}


def workspace_bytes(A, ctx, batches):
    """{plan name: [adm_plan_workspace_bytes(plan, b) for b in batches]} over PLANS."""
    out = {}
    z = ctx.array(np.linspace(0., 1e-4, 8).astype(np.float32))
    for name, (probe, M, streamed, S, obj, pads) in PLANS.items():
        plan = A.Plan(ctx, obj, probe, pads, 1.0, np.ones(probe, complex), n_modes=M, streamed=streamed)
        if S:
            check(ctx.lib.adm_plan_set_slice_positions(plan.handle, z.ptr, S, 0.248, 1.0, 1.0))
        out[name] = [plan.workspace_bytes(b) for b in batches]
        plan.close()
    return out


@pytest.fixture(scope='module')
def sizes():
    import adorym_amd as A
    ctx = A.Context(0)
    yield workspace_bytes(A, ctx, (1, 2, 3, 7, 64, 300))
    ctx.close()


@pytest.mark.parametrize('name', list(PLANS))
def test_workspace_is_linear_in_the_batch(sizes, name):
    w = dict(zip((1, 2, 3, 7, 64, 300), sizes[name]))
    for b in (3, 7, 64, 300):
        assert w[b] == w[1] + (b - 1) * (w[2] - w[1]), (name, b)


@pytest.mark.parametrize('name', list(PLANS))
def test_workspace_sizes_are_the_recorded_ones(sizes, name):
    w = dict(zip((1, 2, 3, 7, 64, 300), sizes[name]))
    assert [w[b] for b in TABLE_BATCHES] == RECORDED[name], name
