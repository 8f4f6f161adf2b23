"""Time the rotation adjoint alone at config 3's shape: python tools/rot_bench.py [label]

One line per run: us per launch of adm_rotate_adj_staged at seven angles between 0 and 90 degrees, planes [60, 168) of a 256^3
object; 20 back-to-back launches between two events, best of 4 windows.  `label` names the build in the line (default: the
library's path).  ADM_LIB_PATH=... times an experiment build of the library, e.g. the three bounds of
profiles/r08/r08a_bounds_experiment.patch (a patch of the parent's adm_rotate.hip, never shipped), one library per switch:
    -DADM_BOUND_A   rim blocks return at once (wrong results: how much of a launch is the rim)
    -DADM_BOUND_B   interior boxes staged in one iteration (RB = 4)
    -DADM_BOUND_C   stage stores dropped for the clamped duplicates past the box's end
Alternate the builds, three rounds each: the spread between rounds is the yardstick for a difference."""
import sys, os
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np, adorym_amd as A
from adorym_amd import workloads as W
label = sys.argv[1] if len(sys.argv) > 1 else os.environ.get('ADM_LIB_PATH', 'default')
cfg = W.c3_config(); ctx = A.Context(0)
eng = A.MultisliceEngine(ctx, cfg['obj_size'], cfg['probe_size'], cfg['probe_pos'], cfg['energy_ev'], cfg['psize_cm'], max_batch=32)
g = ctx.zeros((256, 256, 256, 2))
eng.grad_rot.set(np.random.default_rng(0).standard_normal(eng.grad_rot.shape).astype(np.float32))
thetas = np.linspace(0, 2 * np.pi, 500, dtype='float32')
e0, e1 = ctx.event(), ctx.event()
out = []
for it in (0, 20, 41, 62, 83, 104, 125):
    tab = A.RotationTable(ctx, cfg['obj_size'], thetas[it]); tab.csr(eng.plan)
    eng.rotate_adjoint(g, tab, (60, 168))
    ts = []
    for r in range(4):
        e0.record()
        for _ in range(20):
            eng.rotate_adjoint(g, tab, (60, 168))
        e1.record(); ts.append(e0.elapsed_ms(e1) / 20)
    out.append('%.2f: %.1f' % (thetas[it], 1e3 * min(ts)))
print('%-18s adj us/launch | %s' % (label, ' | '.join(out)))
