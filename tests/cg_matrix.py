"""The conjugate-gradient tests' tables: the driver runs of golden F33 (tests/golden/gen_f33_cg.py writes them, tests/cg_ref.py
restates them, tests/test_gpu_cg*.py holds the GPU code to them), the kernel sizes, and every bar -- written once, with its reason.

Runs, all on cases.e2e_inputs() (32^3 object, 16^2 probe, 4 angles x 9 positions; 3-D data: golden F6's 'prj'):
  a  first-trial acceptances with beta > 0       3-D, minibatch 9, learning_rate 1e-4, 3 epochs (12 updates)
  b  backtracking, three halvings and more       3-D, minibatch 3, 2 epochs; learning_rate: the first of B_CANDIDATES whose Armijo
                                                 margins clear the fp32 noise (the generator decides and stores it)
  c  a failed search                             an instance with max_backtracking_iter = 1 at a large step (C_CANDIDATES likewise)
  d  2-D, one slice, one minibatch per epoch     beta = 0 at every update (i_batch is 0): steepest descent with a line search
  e  non_negativity=True                         run a's setting, 2 epochs, at the first step of E_CANDIDATES that leaves voxels clipped
"""
import numpy as np

RUNS = {
    'a': dict(three_d=True, minibatch_size=9, n_epochs=3, learning_rate=1e-4),
    'b': dict(three_d=True, minibatch_size=3, n_epochs=2, learning_rate=None),
    'c': dict(three_d=True, minibatch_size=9, n_epochs=1, learning_rate=None, options=dict(max_backtracking_iter=1)),
    'd': dict(three_d=False, minibatch_size=9, n_epochs=8, learning_rate=1e-4),
    'e': dict(three_d=True, minibatch_size=9, n_epochs=2, learning_rate=None, non_negativity=True),
}
B_CANDIDATES = (1., 0.3, 0.1, 0.03, 0.01)          # the issue: a learning_rate between 1e-2 and 1
C_CANDIDATES = (1., 3., 0.3, 10.)
E_CANDIDATES = (1e-4, 1e-3, 1e-2, 3e-2)            # the first at which the constraint binds: voxels of the final object at 0
# a fixture is usable when every decision of its line searches is further from its threshold than the reference's own fp32 run is
# from its fp64 run, by this factor (the generator asserts it; both numbers are stored)
MARGIN_FACTOR = 10.

# ---- bars ----
REF_REL = 1e-9          # tests/cg_ref.py against the reference's fp64 run: both are float64 restatements of the same formulas
THREE = 3.              # the GPU against fp64: 3 x the reference's own fp32 distance for that quantity (check_run's rule)
SUM_REL = 1e-12         # a sum against NumPy's float64 sum of the same float32 inputs, relative to sum |terms|: the products are
#                         exact in double (24 x 24 bits), only the additions round: <= (n_adds on any path) x 2^-53 x sum |terms|, and
#                         no path of the kernels' trees is longer than ~ n / (1024 x 256) + 8 + 4 + 1024 additions (4.5e3 x 1.1e-16)
FMA_ULP = 2.0 ** -23    # s_new, x_trial against NumPy float32: |diff| <= 2^-23 (|a| + |b c|) allows a fused multiply-add, nothing more

SIZES = (1, 63, 64, 65, 255, 257, 1023, 1025, 2 * 16 ** 3, 2 * 33 ** 3, 2 ** 20 + 3)
FLAGS = tuple(range(8))


def two_d_inputs(inp, N):
    """Run d: the middle slice of the 3-D case as a one-slice object (8 x the per-voxel values: a comparable projected thickness)."""
    sl = slice(N // 2, N // 2 + 1)
    truth = np.stack(inp['truth'], -1)[:, :, sl] * 8
    guess = [g[:, :, sl] for g in inp['guess']]
    return truth, guess


def obj_sample(shape, n=4096):
    """The voxels of a [Y, X, Z, 2] object whose float64 values the golden keeps (a committed file is limited to 1 MiB, five whole
    float64 objects are 2.6 MB): a fixed random subset, sorted flat voxel indices; everything when the object is that small.  Distances
    between objects -- the reference's fp32 run from its fp64 run, the GPU's from the fp64 run -- are taken on these voxels."""
    V = int(np.prod(shape[:3]))
    return np.arange(V) if V <= n else np.sort(np.random.default_rng(33).choice(V, n, replace=False))


def sampled(obj):
    """obj [Y, X, Z, 2] (or delta, beta stacked so) -> [n, 2] on obj_sample's voxels."""
    obj = np.asarray(obj)
    return obj.reshape(-1, 2)[obj_sample(obj.shape)]


def kernel_inputs(n, seed=0):
    """Values of mixed sign and scale: normal deviates times 10^u, u uniform in [-3, 3]; x, g, s, d_old."""
    r = np.random.default_rng(1000 + seed)
    mk = lambda: (r.standard_normal(n) * 10.0 ** r.uniform(-3, 3, n)).astype(np.float32)
    return dict(x=mk(), g=mk(), s=mk(), d_old=mk())


def options(g, name):
    """The optimiser's options_dict of run ``name`` (``g``: golden F33, which holds the step the generator settled on)."""
    return dict(RUNS[name].get('options') or {}, step_size=float(g[name + '_learning_rate']))


def driver_params(g, name, inp, E, prj3d, save_path):
    """reconstruct_ptychography's keywords for run ``name`` (without the optimiser), as the generator gave them to the reference."""
    spec, N = RUNS[name], E['N']
    if spec['three_d']:
        data, obj_size, theta_end, n_theta, guess = np.asarray(prj3d, np.float32), [N] * 3, 2 * np.pi, E['n_theta'], inp['guess']
    else:
        data, obj_size, theta_end, n_theta, guess = np.asarray(g[name + '_prj'], np.float32), [N, N, 1], 0, 1, two_d_inputs(inp, N)[1]
    return dict(fname=data, obj_size=obj_size, probe_pos=inp['probe_pos'], theta_st=0, theta_end=theta_end, n_theta=n_theta,
                energy_ev=E['energy_ev'], psize_cm=E['psize_cm'], free_prop_cm='inf', minibatch_size=spec['minibatch_size'],
                n_epochs=spec['n_epochs'], initial_guess=[guess[0], guess[1]], probe_type='supplied',
                probe_initial=[inp['probe_mag'], inp['probe_phase']], gamma=0, alpha_d=0, alpha_b=0, two_d_mode=not spec['three_d'],
                non_negativity=bool(spec.get('non_negativity')), save_path=str(save_path), output_folder='out', store_checkpoint=False,
                use_checkpoint=False, return_state=True)
