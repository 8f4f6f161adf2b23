"""
reconstruct_ptychography -- the reference's entry point (adorym/ptychography.py:54-1296), data-parallel
mode (``distribution_mode=None``), driving the HIP path.  The keyword surface is the reference's,
verbatim; combinations outside the accelerated path raise NotImplementedError instead of silently doing
something else.  Control flow (epoch / batching / update / constraints / logging order) follows the
reference line by line so that runs are comparable minibatch for minibatch:

    :783-847   epoch task list (np.random.seed(i_epoch), theta shuffle, padding of the spot list)
    :901-912   this rank's slice of the global batch, sorted
    :1017-1039 gradient of the loss   -> Differentiator.get_gradients -> hand adjoint (HIP)
    :1063-1066 gradient accumulation  -> fused into the adjoint's output buffer
    :1095-1099 'per angle' update scheme
    :1113-1129 allreduce + optimiser  -> reduce_scatter + fused Adam/GD on the shard + all_gather
    :1135-1158 constraints, :1210-1215 support mask -> fused into the optimiser kernel
    :1254-1271 throughput print, convergence log, optimiser step counter
"""
import datetime
import os
import sys
import threading
import time
import warnings

import numpy as np

from . import _lib
from . import global_settings
from .array_ops import ObjectFunction, Gradient, Mask
from .comm import from_env
from .util import epoch_task_list, rank_batch, initialize_probe
from .constants import PI
from .device import Context, DeviceArray
from .differentiator import Differentiator
from .dp import DataParallelObject, HipOps, constraint_flags
from .forward_model import PtychographyModel, MultiDistModel, SparseMultisliceModel
from .optimizers import Optimizer, AdamOptimizer, GDOptimizer, MomentumOptimizer, CGOptimizer, apply_small_params, plain_adam
from .propagate import MultisliceEngine, ProjectionEngine, RotationTable, get_kernel
from .regularizers import L1Regularizer, TVRegularizer, ReweightedL1Regularizer, combined_weights
from ._io import DataFile, write_tiff, read_tiff


def print_flush(a, designate_rank=None, this_rank=None, save_stdout=False, output_folder='', timestamp='', **kwargs):
    """adorym/misc.py:233-257."""
    a = '[{}][{}] '.format(str(datetime.datetime.today())[:-3], this_rank) + a
    if designate_rank is None or this_rank == designate_rank:
        print(a)
        if save_stdout:
            os.makedirs(output_folder, exist_ok=True)     # (the first lines are printed before the driver creates the folder)
            with open(os.path.join(output_folder, 'stdout_{}.txt'.format(timestamp)), 'a') as f:
                f.write(a + '\n')
    sys.stdout.flush()


def _atomic_write(path, writer):
    """Write through a temporary name and os.replace() it into place: a reader never sees a half-written file."""
    tmp = path + '.tmp'
    with open(tmp, 'wb') as f_tmp:
        writer(f_tmp)
        f_tmp.flush()
        os.fsync(f_tmp.fileno())        # the invalidate -> data -> stamp order must also hold on the disk (power loss)
    os.replace(tmp, path)
    try:
        dfd = os.open(os.path.dirname(path) or '.', os.O_RDONLY)
        try:
            os.fsync(dfd)
        finally:
            os.close(dfd)
    except OSError:
        pass


def save_checkpoint(i_epoch, i_batch, output_folder, obj_array, moments, opt_name='obj', rank=0, n_ranks=1, params=None):
    """Reference file formats (adorym/misc.py:179-194, adorym/optimizers.py:170-188, :779-790):
    checkpoint/checkpoint.txt (epoch, batch), obj_checkpoint.npy [Y,X,Z,2], opt_obj_params_checkpoint.npy
    (stacked moments [n,Y,X,Z,2]) and the pickled params_{rank}.  With more than one rank the moments are sharded,
    so every rank writes its shard as opt_obj_params_checkpoint_rank_{r}.npy (the reference's per-rank naming).

    Every rank writes its files from its own helper thread, so a crash can leave files of different minibatches side by
    side.  To make that detectable (not part of the reference's format): every file goes through a temporary name +
    os.replace; each rank first INVALIDATES its stamp_rank_{r}.txt (-1, -1), then replaces its data files, then writes the
    stamp (epoch, batch), and rank 0 writes checkpoint.txt last; restore_checkpoint() only accepts a checkpoint whose stamp
    equals checkpoint.txt -- so a crash between two of one rank's own files (new object, old moments, old counter) is refused
    like a crash between two ranks' saves."""
    import pickle
    path = os.path.join(output_folder, 'checkpoint')
    os.makedirs(path, exist_ok=True)
    stamp = np.array([i_epoch, i_batch])
    _atomic_write(os.path.join(path, 'stamp_rank_{}.txt'.format(rank)), lambda f_: np.savetxt(f_, np.array([-1, -1]), fmt='%d'))
    if rank == 0:
        _atomic_write(os.path.join(path, 'obj_checkpoint.npy'), lambda f_: np.save(f_, obj_array))
    if len(moments) > 0:
        arr = np.stack(moments)
        if n_ranks == 1:
            arr = arr.reshape((len(moments),) + obj_array.shape)
            name = 'opt_{}_params_checkpoint.npy'.format(opt_name)
        else:
            name = 'opt_{}_params_checkpoint_rank_{}.npy'.format(opt_name, rank)
        _atomic_write(os.path.join(path, name), lambda f_: np.save(f_, arr))
    if params is not None:
        _atomic_write(os.path.join(path, 'params_{}'.format(rank)), lambda f_: pickle.dump(params, f_))
    _atomic_write(os.path.join(path, 'stamp_rank_{}.txt'.format(rank)), lambda f_: np.savetxt(f_, stamp, fmt='%d'))
    if rank == 0:
        _atomic_write(os.path.join(path, 'checkpoint.txt'), lambda f_: np.savetxt(f_, stamp, fmt='%d'))


def restore_checkpoint(output_folder, n_moments, opt_name='obj', rank=0, n_ranks=1, obj_shape=None, shard_size=None):
    """adorym/misc.py:197-211 + load_params_checkpoint (adorym/ptychography.py:462).  Everything is read and shape-checked
    BEFORE anything is returned, so a partial checkpoint cannot leave a run half restored; the stamps of ALL ranks must equal
    checkpoint.txt (a checkpoint torn by a crash in the middle of a save is refused; checkpoints written by the reference
    itself carry no stamps and are accepted as they are).
    Returns (i_epoch, i_batch, obj [Y,X,Z,2], moments or None, params dict or None)."""
    import pickle
    path = os.path.join(output_folder, 'checkpoint')
    i_epoch, i_batch = [int(i) for i in np.loadtxt(os.path.join(path, 'checkpoint.txt'))]
    # EVERY rank's stamp is checked by every rank: ranks > 0 load the object rank 0 wrote, so a save that rank 0 did not finish
    # must be refused by them too, not only by rank 0 (the driver then agrees on the verdict over the communicator)
    if os.path.exists(os.path.join(path, 'stamp_rank_{}.txt'.format(rank))):
        for r_ in range(n_ranks):
            fs = os.path.join(path, 'stamp_rank_{}.txt'.format(r_))
            if not os.path.exists(fs):
                raise ValueError('torn checkpoint: rank %d never wrote a stamp (checkpoint written with fewer ranks?)' % r_)
            st = [int(i) for i in np.loadtxt(fs)]
            if st != [i_epoch, i_batch]:
                raise ValueError('torn checkpoint: rank %d %s, checkpoint.txt says %s'
                                 % (r_, 'was interrupted in the middle of a save' if st == [-1, -1] else
                                    'wrote its files for (epoch, batch) = %s' % (tuple(st),), (i_epoch, i_batch)))
    obj = np.load(os.path.join(path, 'obj_checkpoint.npy'))
    if obj_shape is not None and tuple(obj.shape) != tuple(obj_shape):
        raise ValueError('obj_checkpoint.npy has shape %s, expected %s' % (obj.shape, tuple(obj_shape)))
    mom = None
    if n_moments > 0:
        f1 = os.path.join(path, 'opt_{}_params_checkpoint.npy'.format(opt_name))
        fr = os.path.join(path, 'opt_{}_params_checkpoint_rank_{}.npy'.format(opt_name, rank))
        mom = np.load(f1 if n_ranks == 1 else fr)
        if len(mom) != n_moments:
            raise ValueError('optimizer checkpoint holds %d moment arrays, expected %d' % (len(mom), n_moments))
        if n_ranks > 1 and shard_size is not None and mom[0].size != shard_size:
            raise ValueError('optimizer checkpoint shard has %d elements, expected %d (written with another rank count?)'
                             % (mom[0].size, shard_size))
    params = None
    fp = os.path.join(path, 'params_{}'.format(rank))
    if os.path.exists(fp):
        with open(fp, 'rb') as f_pcp:
            params = pickle.load(f_pcp)
    return i_epoch, i_batch, obj, mom, params


_SUMMARY_VARS = ('obj_size probe_size output_folder theta_downsample n_theta n_epochs learning_rate alpha_d alpha_b gamma n_dp_batch '
                 'minibatch_size free_prop_cm psize_cm energy_ev fname cpu_only optimizer probe_mag_sigma probe_phase_sigma '
                 'probe_phase_max probe_learning_rate probe_type optimize_probe_defocusing probe_defocusing_learning_rate '
                 'optimizer_probe_defocusing optimize_all_probe_pos all_probe_pos_learning_rate optimizer_all_probe_pos '
                 'optimize_probe_pos_offset probe_pos_offset_learning_rate optimizer_probe_pos_offset shared_file_object '
                 'reweighted_l1 initial_guess binning').split()


def create_summary(save_path, values, verbose=True):
    """summary.txt of a run (adorym/misc.py:149-176, preset 'ptycho'): one '{:<30}{}' line per reported parameter; a
    learning rate is left out when a ready-made optimiser object was passed for that parameter, names that do not exist
    in this run are skipped (the reference's bare except)."""
    os.makedirs(save_path, exist_ok=True)
    lines = []
    for name in _SUMMARY_VARS:
        if name == 'learning_rate' and values.get('optimizer') is not None and not isinstance(values.get('optimizer'), str):
            continue
        if name.endswith('_learning_rate') and values.get('optimizer_' + name[:-14]) is not None:
            continue
        if name not in values:
            continue
        v = values[name]
        if name == 'fname' and not isinstance(v, str):
            v = '<array %s>' % (np.shape(v),)
        lines.append('{:<30}{}\n'.format(name, str(v)))
    with open(os.path.join(save_path, 'summary.txt'), 'w') as f_sum:
        f_sum.writelines(lines)
    if verbose:
        print('============== PARAMETERS ==============')
        print(''.join(lines))
        print('========================================')


def _host(v):
    return v.get() if hasattr(v, 'get') else v


def _mag_phase(a):
    return np.sqrt(a[..., 0] ** 2 + a[..., 1] ** 2), np.arctan2(a[..., 1], a[..., 0])


def _write_images(obj_dir, probe_dir, tag, arr, unknown_type, probe=None, complex_probe=False):
    """The object's images (delta / beta, or obj_mag / obj_phase for unknown_type='real_imag', util.py:1990-2005) under ``obj_dir``
    and, given ``probe`` [modes, Py, Px, 2], probe_mag / probe_phase under ``probe_dir``; every name ends in ``tag``.
    ``complex_probe``: the probe's images are np.abs / np.angle of the complex probe (the outputs after an epoch) instead of
    sqrt(re^2 + im^2) / arctan2 (the intermediate ones); the two can differ in the last bit."""
    if unknown_type == 'delta_beta':
        images = [(obj_dir, 'delta', arr[..., 0]), (obj_dir, 'beta', arr[..., 1])]
    else:
        images = list(zip((obj_dir,) * 2, ('obj_mag', 'obj_phase'), _mag_phase(arr)))
    if probe is not None:
        if complex_probe:
            pc = probe[..., 0] + 1j * probe[..., 1]
            mag_phase = np.abs(pc), np.angle(pc)
        else:
            mag_phase = _mag_phase(probe)
        images += zip((probe_dir,) * 2, ('probe_mag', 'probe_phase'), mag_phase)
    for d_, name, im in images:
        os.makedirs(d_, exist_ok=True)
        write_tiff(im, os.path.join(d_, name + tag), dtype='float32')


def _not_implemented(cond, what):
    if cond:
        raise NotImplementedError(what + ' is outside the accelerated path of adorym_amd (see DESIGN.md, out of scope)')


def reconstruct_ptychography(
        # |Raw data and experimental parameters|
        fname, obj_size, probe_pos=None, theta_st=0, theta_end=PI, n_theta=None, theta_downsample=None,
        energy_ev=None, psize_cm=None, free_prop_cm=None,
        raw_data_type='magnitude', is_minus_logged=False, slice_pos_cm_ls=None,
        # |Reconstruction parameters|
        n_epochs='auto', crit_conv_rate=0.03, max_nepochs=200,
        regularizers=None, alpha_d=None, alpha_b=None, gamma=1e-6,
        minibatch_size=None, multiscale_level=1, n_epoch_final_pass=None,
        initial_guess=None, random_guess_means_sigmas=(8.7e-7, 5.1e-8, 1e-7, 1e-8),
        n_batch_per_update=1, reweighted_l1=False, interpolation='bilinear',
        update_scheme='immediate', unknown_type='delta_beta', randomize_probe_pos=False,
        common_probe_pos=True, fix_object=False,
        # |Object optimizer options|
        optimize_object=True, optimizer='adam', learning_rate=1e-5, update_using_external_algorithm=None,
        optimizer_batch_number_increment='angle',
        # |Finite support constraint|
        finite_support_mask_path=None, shrink_cycle=None, shrink_threshold=1e-9,
        # |Object contraints|
        object_type='normal', non_negativity=False,
        # |Forward model|
        forward_model='auto', forward_algorithm='fresnel', ctf_lg_kappa=1.7,
        binning=1, fresnel_approx=True, pure_projection=False, two_d_mode=False,
        probe_type='gaussian', probe_initial=None, probe_extra_defocus_cm=None, n_probe_modes=1,
        shared_probe_among_angles=True, rescale_probe_intensity=False,
        loss_function_type='lsq', poisson_multiplier=1., beamstop=None, normalize_fft=False, safe_zone_width=0,
        scale_ri_by_k=True, sign_convention=1, fourier_disparity=False,
        # |I/O|
        save_path='.', output_folder=None, save_intermediate=False, save_intermediate_level='batch', save_history=False,
        store_checkpoint=True, use_checkpoint=True, force_to_use_checkpoint=False, n_batch_per_checkpoint=10,
        save_stdout=False,
        # |Performance|
        cpu_only=False, core_parallelization=True, gpu_index=0, n_dp_batch=20,
        distribution_mode=None, dist_mode_n_batch_per_update=None, precalculate_rotation_coords=True,
        cache_dtype='float32', rotate_out_of_loop=False, n_split_mpi_ata='auto',
        # |Other optimizer options|
        optimize_probe=False, probe_learning_rate=1e-5, optimizer_probe=None,
        probe_update_delay=0, probe_update_limit=None,
        optimize_probe_defocusing=False, probe_defocusing_learning_rate=1e-5, optimizer_probe_defocusing=None,
        optimize_probe_pos_offset=False, probe_pos_offset_learning_rate=1e-2, optimizer_probe_pos_offset=None,
        optimize_prj_pos_offset=False, prj_pos_offset_learning_rate=1e-2, optimizer_prj_pos_offset=None,
        optimize_all_probe_pos=False, all_probe_pos_learning_rate=1e-2, optimizer_all_probe_pos=None,
        optimize_slice_pos=False, slice_pos_learning_rate=1e-4, optimizer_slice_pos=None,
        optimize_free_prop=False, free_prop_learning_rate=1e-2, optimizer_free_prop=None,
        optimize_prj_affine=False, prj_affine_learning_rate=1e-3, optimizer_prj_affine=None,
        optimize_tilt=False, tilt_learning_rate=1e-3, optimizer_tilt=None, initial_tilt=None,
        optimize_ctf_lg_kappa=False, ctf_lg_kappa_learning_rate=1e-3, optimizer_ctf_lg_kappa=None,
        other_params_update_delay=0,
        # |Alternative algorithms|
        use_epie=False, epie_alpha=0.8,
        # |Other settings|
        dynamic_rate=True, pupil_function=None, probe_circ_mask=0.9, dynamic_dropping=False, dropping_threshold=8e-5,
        backend='hip', debug=False, t_max_min=None, xpu=False, run_bfloat16=False, run_float64=False,
        **kwargs):
    """
    Same contract as the reference: returns None; results are files under ``save_path/output_folder``
    (delta_ds_1.tiff, beta_ds_1.tiff, probe_mag_ds_1.tiff, probe_phase_ds_1.tiff, convergence/loss_rank_*.txt).
    ``fname`` may also be a NumPy array / dict holding 'exchange/data' (no file needed), and ``kwargs`` may
    carry ``comm=`` (an adorym_amd.comm object) and ``return_state=True`` (returns a dict of final arrays; for sparse
    multislice also 'slice_pos_cm_ls' and, when they are refined, 'slice_pos_history': the positions after every update).
    ``backend`` accepts 'hip' (and, for script compatibility, the reference's 'pytorch' / 'autograd' names,
    which are mapped to 'hip' with a warning).
    """
    _call_args = dict(locals())         # the keyword surface as called (for summary.txt); first statement on purpose
    _call_args.update(_call_args.pop('kwargs', {}))
    run = _Run(_call_args, kwargs)
    run.refuse_unsupported()
    run.open_device()
    run.read_data()
    run.create_engines()
    run.create_object()
    run.create_forward_model()
    run.create_probe_and_small_params()
    run.run_epochs()
    return run.finish()


class _SmallParam(object):
    """One optimised small parameter (optimizers.py:1022-1083): its ``key`` in optimizable_params, its optimiser, device value ``x``,
    gradient accumulator ``g``, index ``i_grad`` in the gradient tuple, the extras of its update (``pin``: copied over the first entries
    of x; ``center_cols``: the drift guard) and the global minibatch indices [delay, limit) in which it is updated."""

    def __init__(self, key, opt, x, i_grad, delay, limit, **extras):
        self.key, self.opt, self.x, self.i_grad, self.delay, self.limit, self.extras = key, opt, x, i_grad, delay, limit, extras
        self.g = x.ctx.zeros(x.shape)

    def due(self, i_global):
        return self.delay <= i_global < self.limit


# the small parameters that the fused holography launch (adm_holo_fwd_adj_adam) updates, with its argument for each; a run that
# optimises any other one takes the separate launches
_HOLO_FUSED_SLOTS = {'free_prop_cm': 'dists', 'prj_affine_ls': 'affine'}


class _Run(object):
    """One call of reconstruct_ptychography.  The named keywords are its attributes and every stage adds what it builds.  Like the
    reference's locals, some keywords are rewritten once: output_folder (save_path joined), obj_size, two_d_mode, n_theta, probe_pos,
    energy_ev, psize_cm, free_prop_cm, safe_zone_width and minibatch_size by open_device / read_data; fuse_per_angle and forward_model
    ('auto' or a class, then the model itself) by create_forward_model."""

    def __init__(self, call_args, kwargs):
        self.call_args = call_args
        self.__dict__.update((k, v) for k, v in call_args.items() if k not in kwargs)
        self.t_zero = time.time()
        self.comm = kwargs.pop('comm', None) or from_env()       # (the private keywords; the rest of kwargs goes to initialize_probe)
        self.return_state = kwargs.pop('return_state', False)
        self.fuse_per_angle = kwargs.pop('fuse_per_angle', True)
        # sub-pixel probe positions on the streamed path (probes beyond 128 x 128): applied inside the sweep on request
        self.streamed_probe_shift = bool(kwargs.pop('streamed_probe_shift', False))
        # optimize_free_prop for multi-distance data of a 3-D object (holotomography): the distances refined on the device, on request
        self.fanout_free_prop = bool(kwargs.pop('fanout_free_prop', False))
        # optimize_prj_affine for the same data: the holograms registered by kernels of their own (HologramRegistration), on request
        self.fanout_prj_affine = bool(kwargs.pop('fanout_prj_affine', False))
        # forward_algorithm='ctf' for multi-distance data of a 3-D object (CTF holotomography: RotatedProjector + CTFEngine), on request
        self.ctf_tomography = bool(kwargs.pop('ctf_tomography', False))
        # update_using_external_algorithm='ctf': the delta channel overwritten by the direct CTF inversion in every minibatch
        # (CTFInversion), on request
        self.ctf_direct_update = bool(kwargs.pop('ctf_direct_update', False))
        # optimize_free_prop under forward_algorithm='ctf': the distances refined on the device (CTFEngine(refine_distances=True)), on request
        self.ctf_free_prop = bool(kwargs.pop('ctf_free_prop', False))
        # optimize_prj_affine under forward_algorithm='ctf': the holograms registered in front of the launch group
        # (HologramRegistration), on request
        self.ctf_prj_affine = bool(kwargs.pop('ctf_prj_affine', False))
        # optimizer='cg': conjugate gradient with a line search for the object (CGOptimizer), on request
        self.device_cg = bool(kwargs.pop('device_cg', False))
        # optimize_ctf_lg_kappa under forward_algorithm='fresnel': the single-material constraint beta = kappa delta wrapped around
        # the object of the multi-distance Fresnel models (HomogeneousObject), on request
        self.fresnel_kappa = bool(kwargs.pop('fresnel_kappa', False))
        self.ops =kwargs.pop('ops', None)
        kwargs.pop('probe_size', None)
        self.kwargs = kwargs
        self.n_ranks, self.rank = self.comm.size, self.comm.rank

    def log(self, msg):
        print_flush(msg, self.sto_rank, self.rank, **self.stdout_options)

    def refuse_unsupported(self):
        """Combinations outside the accelerated path fail loudly (the ones that need the data's shape: read_data)."""
        if self.backend != 'hip':
            warnings.warn("adorym_amd has a single backend ('hip'); backend='%s' is ignored." % self.backend)
        global_settings.backend = 'hip'
        _not_implemented(self.distribution_mode is not None, "distribution_mode='%s'" % self.distribution_mode)
        # conjugate gradient (CGOptimizer: an instance, or optimizer='cg' with device_cg=True) searches along a line with the loss of
        # the minibatch whose gradient it was handed: one rank, an update per minibatch, the object in its own frame, and the object only
        self.is_cg = isinstance(self.optimizer, CGOptimizer) or (self.optimizer == 'cg' and self.device_cg)
        if self.is_cg:
            what = 'CGOptimizer with %s'
            _not_implemented(self.n_ranks > 1, what % 'more than one rank (user-defined object optimizers with more than one rank)')
            # (the reference would judge a gradient accumulated over an angle by the loss of the angle's last minibatch)
            _not_implemented(self.update_scheme == 'per angle', what % "update_scheme='per angle'")
            _not_implemented(bool(self.rotate_out_of_loop), what % 'rotate_out_of_loop')
            _not_implemented(self.update_using_external_algorithm is not None, what % 'update_using_external_algorithm')
        for nm in ('probe', 'probe_defocusing', 'probe_pos_offset', 'prj_pos_offset', 'all_probe_pos', 'slice_pos', 'free_prop', 'prj_affine',
                   'tilt', 'ctf_lg_kappa'):
            # (self.name == 'probe' in the reference's CGOptimizer is dead code in its driver: no small parameter's update hands it a loss)
            _not_implemented(isinstance(getattr(self, 'optimizer_' + nm), CGOptimizer),
                             'CGOptimizer as optimizer_%s (it serves the object only)' % nm)
        if self.cpu_only:
            # (demos/2d_ptychography_w_position_correction.py asks for it; there is no CPU path here and none is substituted)
            warnings.warn('cpu_only=True is ignored: adorym_amd computes on the GPU only.')
        _not_implemented(self.run_bfloat16 or self.run_float64, 'run_bfloat16 / run_float64')
        if self.unknown_type not in ('delta_beta', 'real_imag'):
            raise ValueError("unknown_type must be 'delta_beta' or 'real_imag'")
        if self.unknown_type == 'real_imag':
            # accelerated subset for complex-transmission unknowns: no masks / object-type constraints / binning yet
            _not_implemented(self.finite_support_mask_path is not None, "finite support mask with unknown_type='real_imag'")
            _not_implemented(self.object_type != 'normal', "object_type='%s' with unknown_type='real_imag'" % self.object_type)
            _not_implemented(self.binning != 1, "binning > 1 with unknown_type='real_imag'")
        _not_implemented(self.multiscale_level != 1, 'multiscale_level > 1')
        # 'ctf' (the contrast-transfer-function model) serves multi-distance data only: read_data refuses it elsewhere
        _not_implemented(self.forward_algorithm not in ('fresnel', 'ctf') or (self.forward_algorithm == 'ctf' and bool(self.pure_projection)),
                         "forward_algorithm='%s'" % (self.forward_algorithm,))
        if self.pure_projection:
            # the projection approximation (ProjectionEngine): delta_beta unknowns summed along the beam, rotated inside the loop
            # (the ones that need the data's shape -- sparse multislice, multi-distance data: read_data)
            _not_implemented(self.unknown_type == 'real_imag', "pure_projection with unknown_type='real_imag'")
            _not_implemented(self.is_minus_logged, 'pure_projection with is_minus_logged')
            _not_implemented(bool(self.optimize_prj_pos_offset), 'pure_projection with optimize_prj_pos_offset')
            _not_implemented(bool(self.rotate_out_of_loop), 'pure_projection with rotate_out_of_loop')
        _not_implemented(self.use_epie, 'ePIE')
        _not_implemented(self.is_minus_logged, 'is_minus_logged')
        _not_implemented(not self.common_probe_pos, 'common_probe_pos=False')
        _not_implemented(not self.shared_probe_among_angles, 'shared_probe_among_angles=False')
        ext = self.update_using_external_algorithm
        _not_implemented(ext is not None and not self.ctf_direct_update, 'update_using_external_algorithm')
        # (ctf_direct_update=True: 'ctf' beside the CTF forward model of one slice; what needs the data's shape: read_data)
        self.ctf_direct = ext is not None
        if self.ctf_direct:
            _not_implemented(ext != 'ctf', 'update_using_external_algorithm=%r' % (ext,))
            what = "update_using_external_algorithm='ctf' with %s"
            _not_implemented(self.ctf_tomography, what % 'ctf_tomography')
            _not_implemented(self.forward_algorithm != 'ctf', what % ("forward_algorithm='%s'" % (self.forward_algorithm,)))
            # (the inversion takes its distances from the host, and the raw holograms: the reference hands prj_affine_ls to
            # multidistance_ctf_wrapped, array_ops.py:281-285, which the driver's call of CTFInversion does not)
            _not_implemented(self.ctf_free_prop, what % 'ctf_free_prop')
            _not_implemented(self.ctf_prj_affine, what % 'ctf_prj_affine')
        for nm in ('ctf_free_prop', 'ctf_prj_affine'):
            _not_implemented(getattr(self, nm) and self.forward_algorithm != 'ctf',
                             "%s with forward_algorithm='%s'" % (nm, self.forward_algorithm))
            _not_implemented(getattr(self, nm) and self.n_ranks > 1, '%s with more than one rank' % nm)
        _not_implemented(self.shrink_cycle is not None, 'shrink-wrap mask updates')
        _not_implemented(self.initial_tilt is not None, 'initial_tilt')
        _not_implemented(self.interpolation != 'bilinear', "interpolation='%s'" % self.interpolation)
        for nm in ('optimize_probe_defocusing', 'optimize_probe_pos_offset', 'optimize_tilt'):
            _not_implemented(getattr(self, nm), nm)
        # (the reference threads kappa into multislice_propagate_batch there, forward_model.py:878, 1010: not built)
        # (fresnel_kappa=True: the object is tied in front of the forward model and the gradient folded behind it, HomogeneousObject)
        _not_implemented(bool(self.optimize_ctf_lg_kappa) and self.forward_algorithm != 'ctf' and not self.fresnel_kappa,
                         "optimize_ctf_lg_kappa with forward_algorithm='fresnel'")
        if self.fresnel_kappa:
            if not self.optimize_ctf_lg_kappa:
                # (the reference ties the object only while it refines kappa, forward_model.py:876-878; a fixed kappa is
                # ctf_lg_kappa_learning_rate=0)
                raise ValueError('fresnel_kappa=True needs optimize_ctf_lg_kappa=True (a fixed kappa: ctf_lg_kappa_learning_rate=0)')
            if self.forward_algorithm != 'fresnel':
                raise ValueError("fresnel_kappa=True needs forward_algorithm='fresnel' (the CTF model carries kappa itself)")
            what = "optimize_ctf_lg_kappa with forward_algorithm='fresnel' and %s"
            _not_implemented(self.unknown_type == 'real_imag', what % "unknown_type='real_imag'")
            _not_implemented(bool(self.optimize_all_probe_pos), what % 'optimize_all_probe_pos')
            _not_implemented(self.n_ranks > 1, what % 'more than one rank')
        if self.update_scheme not in ('immediate', 'per angle'):
            raise ValueError("update_scheme must be 'immediate' or 'per angle'")

    def open_device(self):
        """This rank's device context and the run's output folder."""
        comm = self.comm
        stream = comm.stream_handle() if hasattr(comm, 'stream_handle') else None
        dev_index = getattr(comm, 'device_index', None)
        self.ctx = Context(self.gpu_index if dev_index is None else dev_index, stream=stream)
        if hasattr(comm, 'attach'):
            comm.attach(self.ctx)            # RCCL communicator of this rank on the context's stream (adm_comm_init)
        now = str(datetime.datetime.today())
        timestr = now[:now.find('.')].replace(':', '').replace('-', '').replace(' ', '_') if self.rank == 0 else None
        timestr = comm.bcast_object(timestr, root=0)
        if self.output_folder is None:
            self.output_folder = 'recon_{}'.format(timestr)
        if self.save_path != '.':
            self.output_folder = os.path.join(self.save_path, self.output_folder)
        self.stdout_options = {'save_stdout': self.save_stdout, 'output_folder': self.output_folder, 'timestamp': timestr}
        self.sto_rank = 0 if not self.debug else self.rank
        self.log('Output folder is {}'.format(self.output_folder))

    def read_data(self):
        """Data and metadata (ptychography.py:237-346): angles, positions, distances, probe size, minibatch size."""
        t0 = time.time()
        self.f = DataFile(self.fname if not isinstance(self.fname, str) else os.path.join(self.save_path, self.fname))
        prj = self.prj = self.f.data
        obj_size = self.obj_size = [int(v) for v in self.obj_size]
        if obj_size[-1] == 1:
            self.two_d_mode = True
        if self.n_theta is None:
            self.n_theta = prj.shape[0]
        if self.two_d_mode:
            self.n_theta = 1
        try:
            self.theta_ls = np.asarray(self.f.get('metadata/theta'))
        except Exception:
            self.theta_ls = np.linspace(self.theta_st, self.theta_end, self.n_theta, dtype='float32')
        if self.theta_downsample is not None:
            self.theta_ls = self.theta_ls[::self.theta_downsample]
            self.n_theta = len(self.theta_ls)
        probe_pos = self.probe_pos = np.array(self.f.get('metadata/probe_pos_px') if self.probe_pos is None else self.probe_pos).astype(float)
        if self.energy_ev is None:
            self.energy_ev = float(self.f.get('metadata/energy_ev'))
        if self.psize_cm is None:
            self.psize_cm = float(self.f.get('metadata/psize_cm'))
        # sparse multislice (ptychography.py:285-292): a few slices at the depths slice_pos_cm_ls
        self.is_sparse_multislice = self.slice_pos_cm_ls is not None and len(self.slice_pos_cm_ls) > 1
        if self.is_sparse_multislice:
            if len(self.slice_pos_cm_ls) != obj_size[2]:
                raise ValueError('slice_pos_cm_ls holds %d slice positions, the object has %d slices' % (len(self.slice_pos_cm_ls), obj_size[2]))
            _not_implemented(self.binning != 1, 'sparse multislice (slice_pos_cm_ls) with binning = %r' % (self.binning,))
            # the streamed kernels, the one path with a transfer function per gap, take one probe set for all positions
            _not_implemented(self.optimize_all_probe_pos or bool(np.any(probe_pos - np.round(probe_pos) > 1e-3)),
                             'sparse multislice (slice_pos_cm_ls) with sub-pixel probe positions (optimize_all_probe_pos or fractional probe_pos)')
        if self.free_prop_cm is None:
            self.free_prop_cm = self.f.get('metadata/free_prop_cm')
        self.is_multi_dist = np.array(self.free_prop_cm).size != 1          # ptychography.py:296-305
        _not_implemented(self.is_sparse_multislice and self.is_multi_dist, 'sparse multislice (slice_pos_cm_ls) with multi-distance data')
        _not_implemented(self.pure_projection and self.is_sparse_multislice, 'pure_projection with sparse multislice (slice_pos_cm_ls)')
        _not_implemented(self.pure_projection and self.is_multi_dist, 'pure_projection with multi-distance data')
        if self.optimize_prj_pos_offset:
            # per-angle projection alignment (ptychography.py:706, forward_model.py:255-256): the exit wave is shifted by the detector
            # step of the streamed kernels, which take one probe set for all positions and one transfer function for all gaps
            _not_implemented(self.is_sparse_multislice, 'optimize_prj_pos_offset with sparse multislice (slice_pos_cm_ls)')
            _not_implemented(self.is_multi_dist, 'optimize_prj_pos_offset with multi-distance data')
            _not_implemented(self.optimize_all_probe_pos or bool(np.any(probe_pos - np.round(probe_pos) > 1e-3)),
                             'optimize_prj_pos_offset with sub-pixel probe positions (optimize_all_probe_pos or fractional probe_pos)')
            if isinstance(self.free_prop_cm, str) and self.free_prop_cm == 'inf':
                warnings.warn('optimize_prj_pos_offset with a far-field detector: the magnitude of a Fourier transform does not depend on a '
                              'shift of the exit wave, so the gradient is zero and the offsets cannot move.', UserWarning)
        self.is_ctf = self.forward_algorithm == 'ctf'
        _not_implemented(self.is_ctf and not self.is_multi_dist, "forward_algorithm='ctf'")
        self.holo_tiled = self.holo_3d = self.ctf_3d = False
        if self.ctf_direct:
            what = "update_using_external_algorithm='ctf' with %s"
            _not_implemented(not self.two_d_mode, what % 'two_d_mode=False')
            _not_implemented(self.n_ranks > 1, what % 'more than one rank')
            # (the reference masks the object after the inversion, ptychography.py:1210-1215; the fused update here masks before it)
            _not_implemented(self.finite_support_mask_path is not None, what % 'a finite support mask')
        if self.is_multi_dist:
            # config 5 is one object slice and one undivided field of view (n_blocks == 1) without a safe zone
            free_prop_cm = self.free_prop_cm = np.asarray(self.free_prop_cm, dtype=float).reshape(-1)
            n_dists = self.n_dists = len(free_prop_cm)
            safe_zone_width = self.safe_zone_width = int(self.safe_zone_width or 0)
            if prj.shape[1] != n_dists * len(probe_pos):
                raise ValueError('multi-distance data: prj.shape[1] = %d is not n_dists x n_blocks = %d x %d' % (prj.shape[1], n_dists, len(probe_pos)))
            # (ctf_tomography=True: the rotated object summed along the beam is the CTF model's one slice, RotatedProjector + CTFEngine)
            _not_implemented(not self.two_d_mode and self.is_ctf and not self.ctf_tomography, "forward_algorithm='ctf' with two_d_mode=False")
            self.ctf_3d = self.is_ctf and not self.two_d_mode
            if self.ctf_3d:
                what = "forward_algorithm='ctf' with two_d_mode=False and %s"
                _not_implemented(bool(self.rotate_out_of_loop), what % 'rotate_out_of_loop')
                _not_implemented(self.n_ranks > 1, what % 'more than one rank')
                sides = [int(v) for v in obj_size[:2]]
                _not_implemented(any(n < 16 or n > 2048 or n & (n - 1) for n in sides),
                                 what % ('a field of %d x %d (sides: powers of two in [16, 2048])' % tuple(sides)))
            # a 3-D object (holotomography, adorym/forward_model.py:905-914, 971-1019): rotate, ONE slice sweep, the exit wave to
            # every distance (MultisliceEngine(detector_fanout=True)); one undivided field of view, fixed distances, no registration
            self.holo_3d = not self.two_d_mode and not self.is_ctf
            if self.holo_3d:
                what = 'multi-distance holography of a 3-D object with %s'
                _not_implemented(len(probe_pos) > 1 or safe_zone_width > 0, what % 'data divided into sub-tiles or safe_zone_width > 0')
                for nm in ('optimize_free_prop', 'optimize_prj_affine', 'optimize_all_probe_pos', 'rotate_out_of_loop'):
                    # (fanout_free_prop=True: the engine holds the distances as parameters, MultisliceEngine(refine_distances=True))
                    # (fanout_prj_affine=True: the holograms are registered in front of the launch, HologramRegistration)
                    served = (nm == 'optimize_free_prop' and self.fanout_free_prop) or (nm == 'optimize_prj_affine' and self.fanout_prj_affine)
                    _not_implemented(bool(getattr(self, nm)) and not served, what % nm)
                _not_implemented(self.unknown_type == 'real_imag', what % "unknown_type='real_imag'")
                _not_implemented(self.n_ranks > 1, what % 'more than one rank')
            _not_implemented(self.n_probe_modes != 1, "forward_algorithm='ctf' with n_probe_modes != 1" if self.forward_algorithm == 'ctf'
                             else 'several probe modes with multi-distance data')
            _not_implemented(self.loss_function_type != 'lsq', "forward_algorithm='ctf' with loss_function_type='%s'" % self.loss_function_type
                             if self.forward_algorithm == 'ctf' else 'Poisson loss with multi-distance data')
            self.holo_tiled = len(probe_pos) > 1 or safe_zone_width > 0
            _not_implemented(self.fresnel_kappa and self.holo_tiled, "optimize_ctf_lg_kappa with forward_algorithm='fresnel' and data divided "
                             'into sub-tiles or safe_zone_width > 0')
            if self.is_ctf:
                # modulate_and_get_ctf (adorym/propagate.py:467-476): no probe, one slice in delta/beta, one undivided field of view,
                # fixed distances, no registration of the holograms
                # (ctf_free_prop=True: the engine holds the distances as parameters, CTFEngine(refine_distances=True))
                # (ctf_prj_affine=True: the holograms are registered in front of the launch group, HologramRegistration)
                what = "forward_algorithm='ctf' with %s"
                _not_implemented(self.unknown_type == 'real_imag', what % "unknown_type='real_imag'")
                _not_implemented(self.holo_tiled, what % 'data divided into sub-tiles or safe_zone_width > 0')
                for nm in ('optimize_probe', 'optimize_free_prop', 'optimize_prj_affine', 'optimize_all_probe_pos'):
                    served = (nm == 'optimize_free_prop' and self.ctf_free_prop) or (nm == 'optimize_prj_affine' and self.ctf_prj_affine)
                    _not_implemented(bool(getattr(self, nm)) and not served, what % nm)
            if self.holo_tiled:
                # data divided into sub-tiles and / or a safe zone around every tile (adorym/forward_model.py:884-1034)
                tile_size = self.tile_size = [int(v) + 2 * safe_zone_width for v in prj.shape[-2:]]
                _not_implemented(max(tile_size) > 128, 'sub-hologram + 2 safe zones larger than 128 pixels (%d x %d)' % tuple(tile_size))
                _not_implemented(self.optimize_free_prop or self.optimize_prj_affine or self.optimize_probe or self.optimize_all_probe_pos,
                                 'optimize_free_prop / optimize_prj_affine / optimize_probe / optimize_all_probe_pos with multi-distance data divided into sub-tiles')
                _not_implemented(self.beamstop is not None, 'a beamstop with multi-distance data divided into sub-tiles')
                pp_ = np.round(np.asarray(probe_pos)).astype(int)
                if safe_zone_width == 0:
                    # (:921-925 resets pad_arr to zero while the object has been padded: a tile hanging over the edge is misread there)
                    _not_implemented(bool(np.any(pp_ < 0) or np.any(pp_ + np.array(prj.shape[-2:]) > np.array(obj_size[:2]))),
                                     'tiles hanging over the object edge with safe_zone_width = 0')
                if len(probe_pos) > 1:
                    # (:931-943, the branch for a chunk of ONE tile, cuts object and probe to different sizes and fails in the reference)
                    mb_ = self.minibatch_size if self.minibatch_size is not None else len(probe_pos)
                    _not_implemented(mb_ % self.n_dp_batch == 1, 'a minibatch whose last n_dp_batch chunk holds a single tile')
            else:
                _not_implemented(list(prj.shape[-2:]) != list(obj_size[:2]), 'holograms whose size differs from the object size')
                # one (sy, sx) per distance on the measured holograms (forward_model.py:1075-1085): beside the object and the probe only
                _not_implemented(self.optimize_all_probe_pos and (self.optimize_free_prop or self.optimize_prj_affine),
                                 'optimize_all_probe_pos together with optimize_free_prop / optimize_prj_affine')
            self.probe_size = [int(v) for v in obj_size[:2]]          # subdiv_probe (ptychography.py:312-314)
        else:
            _not_implemented(self.optimize_free_prop or self.optimize_prj_affine, 'optimize_free_prop / optimize_prj_affine without multi-distance data')
            _not_implemented(self.fresnel_kappa, "optimize_ctf_lg_kappa with forward_algorithm='fresnel' without multi-distance data")
            if isinstance(self.free_prop_cm, np.ndarray):
                free_prop_cm = self.free_prop_cm.reshape(-1)[0]
                self.free_prop_cm = free_prop_cm if isinstance(free_prop_cm, str) else float(free_prop_cm)
            self.probe_size = [int(v) for v in prj.shape[-2:]]
        self.log('Data reading: {} s'.format(time.time() - t0))
        self.log('Data shape: {}'.format([self.n_theta, *prj.shape[1:]]))

        if self.minibatch_size is None:
            self.minibatch_size = len(probe_pos)
        if self.minibatch_size > 1 and len(probe_pos) == 1:
            warnings.warn('Undivided fullfield data with minibatch > 1: setting minibatch_size to 1 (ptychography.py:342-346).')
            self.minibatch_size = 1
        self.ds_level = 1
        if self.rank == 0:
            os.makedirs(self.output_folder, exist_ok=True)
        self.comm.barrier()

    def create_engines(self):
        """Physics (ptychography.py:388-391) and the multislice / holography engines."""
        ctx, obj_size, probe_size = self.ctx, self.obj_size, self.probe_size
        voxel_nm = np.array([self.psize_cm] * 3) * 1.e7 * self.ds_level
        self.lmbda_nm = 1240. / self.energy_ev
        self.h = get_kernel(voxel_nm[-1] * self.binning, self.lmbda_nm, voxel_nm, probe_size, fresnel_approx=self.fresnel_approx,
                            sign_convention=self.sign_convention) if (self.holo_3d or not self.is_multi_dist) else None
        self.probe_pos_int = np.round(self.probe_pos).astype(int)
        self.holo_engine = self.tile_engine = self.ctf_engine = self.registration = self.ctf_projector = None
        common = dict(sign_convention=self.sign_convention, scale_ri_by_k=self.scale_ri_by_k, unknown_type=self.unknown_type)
        if self.holo_tiled:
            # one engine for all distances: tile = sub-hologram + 2 safe zones at (position - safe zone), every tile listed n_dists
            # times in a row and entry b Fresnel-propagated to distance b % n_dists after the slice (fresnel_propagate,
            # adorym/propagate.py:282-288), loss over the sub-hologram's window only (forward_model.py:1027-1029) -- the detector mask
            # that also serves the beamstop
            szw, tile_size = self.safe_zone_width, self.tile_size
            window = np.zeros(tile_size, np.float32)
            window[szw:tile_size[0] - szw, szw:tile_size[1] - szw] = 1
            self.engine = self.tile_engine = MultisliceEngine(
                ctx, obj_size, tile_size, np.repeat(self.probe_pos_int - szw, self.n_dists, axis=0), self.energy_ev, self.psize_cm,
                free_prop_cm=self.free_prop_cm, max_batch=self.minibatch_size * self.n_dists, beamstop=window, **common)
        elif self.holo_3d:
            # the whole field is the one position; the streamed plan's detector step fans the exit wave out to every distance
            self.engine = MultisliceEngine(
                ctx, obj_size, probe_size, self.probe_pos_int, self.energy_ev, self.psize_cm, free_prop_cm=self.free_prop_cm,
                binning=self.binning, fresnel_approx=self.fresnel_approx, kernel=self.h, max_batch=1, beamstop=self.beamstop,
                transmissions_only=self.forward_model == 'auto', streamed=True, detector_fanout=True,
                refine_distances=bool(self.optimize_free_prop and self.fanout_free_prop), **common)
            if self.optimize_prj_affine and self.fanout_prj_affine:
                from .holography import HologramRegistration
                _not_implemented(self.beamstop is not None, 'multi-distance holography of a 3-D object with optimize_prj_affine and a beamstop')
                self.registration = HologramRegistration(ctx, self.n_dists, probe_size, self.raw_data_type)
        elif self.is_multi_dist:
            if self.is_ctf:
                from .holography import CTFEngine
                refine = bool(self.optimize_free_prop and self.ctf_free_prop)
                register = bool(self.optimize_prj_affine and self.ctf_prj_affine)
                # (registered holograms reach the engine as magnitudes: the registration takes the square root of intensity data)
                self.ctf_engine = CTFEngine(ctx, probe_size, self.n_dists, self.energy_ev, self.psize_cm,
                                            raw_data_type='magnitude' if register else self.raw_data_type, refine_distances=refine,
                                            dists_cm=self.free_prop_cm if refine else None)
                if register:
                    from .holography import HologramRegistration
                    self.registration = HologramRegistration(ctx, self.n_dists, probe_size, self.raw_data_type)
                if self.ctf_direct:
                    from .holography import CTFInversion
                    self.ctf_inversion = CTFInversion(ctx, probe_size, self.n_dists, self.energy_ev, self.psize_cm)
                    self.ctf_direct_data = None       # (the holograms of angle 0, raw, on the device from the first minibatch on)
            else:
                from .holography import HolographyEngine
                self.holo_engine = HolographyEngine(ctx, probe_size, self.n_dists, self.energy_ev, self.psize_cm,
                                                    raw_data_type=self.raw_data_type, **common)
            if self.ctf_3d:
                # the projector rotates and sums the object for the CTF engine and takes the gradient back; its bare plan carries
                # the object geometry for the regulariser kernels and the rotation tables.  No multislice engine, no h.
                from .propagate import RotatedProjector
                self.engine = self.ctf_projector = RotatedProjector(ctx, obj_size)
            else:
                # a minimal multislice plan is still created: it carries the object geometry for the regulariser kernels
                self.engine = MultisliceEngine(ctx, obj_size, (8, 8), np.zeros((1, 2), int), self.energy_ev, self.psize_cm, free_prop_cm=0,
                                               max_batch=1, unknown_type=self.unknown_type)
        else:
            # the projection approximation sums the object along the beam and runs the one-slice problem; an object that HAS one
            # slice is that problem already (the sum of one slice is the slice) and takes the ordinary engine
            cls = ProjectionEngine if (self.pure_projection and obj_size[2] > 1) else MultisliceEngine
            self.engine = cls(
                ctx, obj_size, probe_size, self.probe_pos_int, self.energy_ev, self.psize_cm, free_prop_cm=self.free_prop_cm,
                binning=self.binning, fresnel_approx=self.fresnel_approx, normalize_fft=self.normalize_fft, kernel=self.h,
                n_probe_modes=self.n_probe_modes, max_batch=self.minibatch_size, loss_function_type=self.loss_function_type,
                poisson_multiplier=self.poisson_multiplier, beamstop=self.beamstop,
                # the rotation stores slice transmissions only; rotate_out_of_loop and plugin models read obj_rot
                transmissions_only=(self.forward_model == 'auto' and not self.rotate_out_of_loop),
                # probes too large for one workgroup's LDS (beyond 128 x 128) take the streamed kernels; so does sparse multislice
                # ... and per-angle projection alignment (the exit-wave shift is part of their detector step)
                streamed='auto', slice_pos_cm=self.slice_pos_cm_ls if self.is_sparse_multislice else None,
                exit_shift=bool(self.optimize_prj_pos_offset),
                probe_shift=(self.streamed_probe_shift and not self.is_sparse_multislice and not self.optimize_prj_pos_offset), **common)
            # the rule of _shift_args (forward_model.py): sub-pixel shifts when the corrections are optimised or one exceeds 1e-3
            if self.engine.streamed and not self.engine.probe_shift \
                    and (self.optimize_all_probe_pos or bool(np.any(self.probe_pos - self.probe_pos_int > 1e-3))):
                raise NotImplementedError(
                    'sub-pixel probe positions (optimize_all_probe_pos or fractional probe_pos) with a %d x %d probe (streamed multislice) '
                    'is outside the accelerated path of adorym_amd (see DESIGN.md, out of scope).  The keyword '
                    'streamed_probe_shift=True applies them inside the streamed sweep.' % tuple(probe_size))
        self.homogeneous = None
        if self.fresnel_kappa:
            from .holography import HomogeneousObject
            self.homogeneous = HomogeneousObject(ctx, [*obj_size, 2])
        tables, theta_ls = {}, self.theta_ls

        def rotation_tables(i_theta):
            """Rotation lookup tables: computed like save_rotation_lookup (util.py:492-516), cached on the device per angle (the
            reference caches them as .npy files in ./arrsize_*; no files are written here)."""
            if i_theta not in tables:
                tables[i_theta] = RotationTable(ctx, obj_size, theta_ls[i_theta])
            return tables[i_theta]
        self.rotation_tables = rotation_tables      # (not a method: the model keeps it, and a run it held would outlive the driver)

    def create_object(self):
        """Seed (ptychography.py:410-412), object optimiser (:417-453), object / gradient / moments (:492-576), checkpoint restore."""
        ctx, comm, obj_size = self.ctx, self.comm, self.obj_size
        seed = comm.bcast_object(int(time.time() / 60), root=0)
        np.random.seed(seed)

        optimizer = self.optimizer
        if isinstance(optimizer, Optimizer):
            opt = optimizer
            opt.name = 'obj'
        elif optimizer in ('adam', 'gd', 'momentum'):
            cls, extra = {'adam': (AdamOptimizer, {}), 'gd': (GDOptimizer, dict(dynamic_rate=True, first_downrate_iteration=20)),
                          'momentum': (MomentumOptimizer, {})}[optimizer]
            opt = cls('obj', output_folder=self.output_folder, distribution_mode=self.distribution_mode,
                      options_dict=dict(step_size=self.learning_rate, **extra))
        elif optimizer == 'cg' and self.device_cg:      # (ptychography.py:435-438)
            opt = CGOptimizer('obj', output_folder=self.output_folder, distribution_mode=self.distribution_mode,
                              options_dict=dict(step_size=self.learning_rate))
        elif optimizer in ('curveball', 'cg', 'scipy'):
            raise NotImplementedError("optimizer '%s' is outside the accelerated path" % optimizer)
        else:
            raise ValueError('Invalid optimizer type. Must be "gd" or "adam" or "cg" or "scipy".')
        opt.set_index_in_grad_return(0)
        self.opt = opt
        self.fused = type(opt) in (AdamOptimizer, GDOptimizer, MomentumOptimizer)
        _not_implemented(not self.fused and self.n_ranks > 1, 'user-defined object optimizers with more than one rank')
        self.opt_kind = 'adam' if isinstance(opt, AdamOptimizer) else ('momentum' if isinstance(opt, MomentumOptimizer) else
                                                                     ('cg' if isinstance(opt, CGOptimizer) else 'gd'))

        self.ops = self.ops or HipOps(ctx)
        state = self.state = DataParallelObject(self.ops, comm, [*obj_size, 2], n_moments={'adam': 2, 'momentum': 1, 'gd': 0, 'cg': 2}[self.opt_kind])
        if self.fused:
            if self.opt_kind == 'adam':
                opt.params_whole_array_dict = {'m': state.moments[0], 'v': state.moments[1]}   # shard-sized under DP
            elif self.opt_kind == 'momentum':
                opt.params_whole_array_dict = {'v': state.moments[0]}
        elif self.opt_kind == 'cg':
            # the two state arrays are the run's moment buffers: checkpoints and a resume carry them like Adam's m and v
            opt.whole_object_size, opt.ctx = [*obj_size, 2], ctx
            opt.params_whole_array_dict = {'descent_dir_old': state.moments[0], 's': state.moments[1]}
        else:
            opt.create_container([*obj_size, 2], self.use_checkpoint, ctx)
        obj = self.obj = ObjectFunction([*obj_size, 2], distribution_mode=self.distribution_mode, output_folder=self.output_folder,
                                        ds_level=self.ds_level, object_type=self.object_type, device=ctx)
        init = ObjectFunction.initial_values(obj_size, self.initial_guess, self.random_guess_means_sigmas, self.object_type,
                                             self.non_negativity, unknown_type=self.unknown_type)
        init = comm.bcast_object(init, root=0) if (self.initial_guess is None and self.n_ranks > 1) else init
        obj.arr = state.obj.view(0, (*obj_size, 2))
        obj.arr.set(init)
        del init
        self._resume()
        self.gradient = Gradient(obj)
        self.gradient.arr = state.grad.view(0, (*obj_size, 2))

    def _resume(self):
        """Checkpoint restore (ptychography.py:458-487).  Read into temporaries, agree across ranks, then commit: either every rank
        resumes from the same (epoch, batch) or none does (the reference broadcasts rank 0's counters, :485-487).  The other
        optimisable parameters of the checkpoint (probe, position corrections, distances, affine matrices) are applied once they
        exist (create_probe_and_small_params)."""
        comm, n_ranks, state = self.comm, self.n_ranks, self.state
        self.starting_epoch, self.starting_batch = 0, 0
        self.restored_params = None
        if not self.use_checkpoint:
            return
        loaded, why = None, ''
        try:
            loaded = restore_checkpoint(self.output_folder, len(state.moments), rank=self.rank, n_ranks=n_ranks,
                                        obj_shape=(*self.obj_size, 2), shard_size=state.per)
        except Exception as e:       # missing / partial / mismatching checkpoint
            why = repr(e)
        all_ok = comm.sum_over_ranks(1.0 if loaded is not None else 0.0) >= n_ranks
        if all_ok:
            counters = comm.bcast_object((loaded[0], loaded[1]), root=0)
            all_ok = comm.sum_over_ranks(1.0 if counters == (loaded[0], loaded[1]) else 0.0) >= n_ranks
        if all_ok:
            self.starting_epoch, self.starting_batch, obj_arr, mom, self.restored_params = loaded
            self.obj.arr.set(obj_arr)
            for k_, m_ in enumerate(state.moments):
                m_.set(np.ascontiguousarray(mom[k_]).reshape(-1)[:m_.size] if n_ranks == 1 else mom[k_])
            self.log('Resuming from checkpoint: epoch {}, batch {}.'.format(self.starting_epoch, self.starting_batch))
        else:
            msg = 'Checkpoint not used ({}); starting from epoch 0.'.format(why or 'another rank could not restore, or the ranks disagree')
            if self.force_to_use_checkpoint:
                raise RuntimeError(msg)
            self.log(msg)

    def create_forward_model(self):
        """Forward model (ptychography.py:526-546), regularisers, finite support mask and constraint flags."""
        ctx, unknown_type = self.ctx, self.unknown_type
        common_vars = dict(unknown_type=unknown_type, normalize_fft=self.normalize_fft, sign_convention=self.sign_convention,
                           rotate_out_of_loop=self.rotate_out_of_loop, scale_ri_by_k=self.scale_ri_by_k, is_minus_logged=self.is_minus_logged,
                           forward_algorithm=self.forward_algorithm, pure_projection=bool(self.pure_projection),
                           stdout_options=self.stdout_options, poisson_multiplier=self.poisson_multiplier,
                           common_probe_pos=self.common_probe_pos, binning=self.binning, prj=self.prj, engine=self.engine,
                           holo_engine=self.holo_engine, tile_engine=self.tile_engine, ctf_engine=self.ctf_engine,
                           safe_zone_width=self.safe_zone_width, optimize_probe=self.optimize_probe,
                           n_dp_batch=self.n_dp_batch, optimize_prj_affine=self.optimize_prj_affine, optimize_free_prop=self.optimize_free_prop,
                           optimize_ctf_lg_kappa=self.optimize_ctf_lg_kappa, rotation_tables=self.rotation_tables, two_d_mode=self.two_d_mode,
                           theta_downsample=self.theta_downsample, ds_level=self.ds_level, probe_size=self.probe_size,
                           this_obj_size=self.obj_size, n_theta=self.n_theta, theta_ls=self.theta_ls, energy_ev=self.energy_ev,
                           psize_cm=self.psize_cm, h=self.h, free_prop_cm=self.free_prop_cm, minibatch_size=self.minibatch_size,
                           n_probe_modes=self.n_probe_modes, beamstop=self.beamstop, optimize_probe_defocusing=False,
                           optimize_probe_pos_offset=False, optimize_prj_pos_offset=bool(self.optimize_prj_pos_offset),
                           optimize_all_probe_pos=self.optimize_all_probe_pos,
                           optimize_tilt=False, output_folder=self.output_folder, debug=self.debug)
        if self.registration is not None:
            common_vars['hologram_registration'] = self.registration
        if self.ctf_projector is not None:
            common_vars.update(ctf_projector=self.ctf_projector, n_ranks=self.n_ranks)
        if self.homogeneous is not None:
            common_vars.update(homogeneous_object=self.homogeneous, n_ranks=self.n_ranks)
        fm_args = dict(loss_function_type=self.loss_function_type, distribution_mode=self.distribution_mode, device=ctx,
                       common_vars_dict=common_vars, raw_data_type=self.raw_data_type, run_bfloat16=self.run_bfloat16,
                       run_float64=self.run_float64)
        if self.forward_model == 'auto':
            cls = MultiDistModel if self.is_multi_dist else (SparseMultisliceModel if self.is_sparse_multislice else PtychographyModel)
            self.forward_model = cls(**fm_args)
        else:
            self.forward_model = self.forward_model(**fm_args)
        fm = self.forward_model
        self.builtin_model = type(fm) in (PtychographyModel, MultiDistModel, SparseMultisliceModel)
        if self.opt_kind == 'cg':
            self.gradient.forward_model = fm        # the line search takes its loss function from there (optimizers.py:644-652)
        self.rool = bool(self.rotate_out_of_loop) and not self.two_d_mode and not self.is_multi_dist
        if self.rool:
            _not_implemented(not isinstance(fm, PtychographyModel), 'rotate_out_of_loop with a user-defined forward model')
            self.fuse_per_angle = False
        if self.is_multi_dist:
            # (the multi-distance models evaluate one reference minibatch per call: their loss is a mean over distances x tiles, and
            # 'per angle' adds the minibatches' gradients -- a fused call would average over all of them instead)
            self.fuse_per_angle = False
        self.log('Forward model: {}.'.format(type(fm).__name__))

        regularizers = self.regularizers
        if regularizers is None:
            regularizers = []
            if self.alpha_d not in [0, None]:
                rl1 = ReweightedL1Regularizer if self.reweighted_l1 else L1Regularizer
                regularizers.append(rl1(self.alpha_d, self.alpha_b, unknown_type=unknown_type))
            if self.gamma not in [0, None]:
                regularizers.append(TVRegularizer(self.gamma, unknown_type=unknown_type))
        fm.add_regularizers(regularizers)
        self.reg_rwl1 = None
        for r_ in regularizers:
            if isinstance(r_, ReweightedL1Regularizer):
                self.reg_rwl1 = r_
                self.rwl1_weight = ctx.empty((*self.obj_size, 2))
                self.rwl1_scratch = ctx.empty((2 * 1024 + 2,))

        self.mask = None
        if self.finite_support_mask_path is not None:
            self.mask = Mask(self.obj_size, self.finite_support_mask_path, distribution_mode=self.distribution_mode,
                             output_folder=self.output_folder, ds_level=self.ds_level, device=ctx)
            mask_arr = self.finite_support_mask_path if isinstance(self.finite_support_mask_path, np.ndarray) else read_tiff(self.finite_support_mask_path)
            self.mask.initialize_array_with_values(mask_arr, device=ctx)
        self.flags = constraint_flags(self.non_negativity and unknown_type == 'delta_beta', self.object_type)   # (ptychography.py:1138)

    def create_probe_and_small_params(self):
        """The probe (ptychography.py:607-667), the optimisable parameters and the optimisers of the small ones (:673-735), the
        checkpoint's values of them (load_params_checkpoint, :462), and the gradient's argument list."""
        ctx, comm, n_probe_modes = self.ctx, self.comm, self.n_probe_modes
        if self.rank == 0:
            pk = dict(self.kwargs)
            pk.update(lmbda_nm=self.lmbda_nm, psize_cm=self.psize_cm, normalize_fft=self.normalize_fft, n_probe_modes=n_probe_modes)
            pk.pop('raw_data_type', None)
            pr0, pi0 = initialize_probe(self.probe_size, self.probe_type, pupil_function=self.pupil_function, probe_initial=self.probe_initial,
                                        rescale_intensity=self.rescale_probe_intensity, extra_defocus_cm=self.probe_extra_defocus_cm,
                                        sign_convention=self.sign_convention, raw_data_type=self.raw_data_type,
                                        data_first_angle=np.asarray(self.prj[0:1]) if self.rescale_probe_intensity else None,
                                        data_all=self.prj if self.probe_type == 'ifft' else None, **pk)
            if n_probe_modes == 1:
                probe_real = np.stack([np.squeeze(pr0)]) if pr0.ndim != 3 else pr0[:1]
                probe_imag = np.stack([np.squeeze(pi0)]) if pi0.ndim != 3 else pi0[:1]
            elif pr0.ndim == 3 and len(pr0) > 1:
                probe_real, probe_imag = pr0[:n_probe_modes], pi0[:n_probe_modes]
                if len(probe_real) != n_probe_modes:
                    raise RuntimeError('Length of supplied supplied probe does not match number of probe modes.')
            else:
                # a single supplied / generated probe is spread over the modes with 20 % Gaussian jitter (ptychography.py:641-659)
                pr0, pi0 = np.squeeze(pr0), np.squeeze(pi0)
                probe_real, probe_imag = [], []
                for i_mode in range(n_probe_modes):
                    probe_real.append(np.random.normal(pr0, abs(pr0) * 0.2))
                    probe_imag.append(np.random.normal(pi0, abs(pi0) * 0.2))
                probe_real, probe_imag = np.stack(probe_real), np.stack(probe_imag)
        else:
            probe_real = probe_imag = None
        probe_real = comm.bcast_object(probe_real, root=0)
        probe_imag = comm.bcast_object(probe_imag, root=0)
        self.probe_dev = ctx.array(np.stack([probe_real, probe_imag], -1), np.float32)       # [modes, Py, Px, 2]

        n_theta = self.n_theta
        params = self.optimizable_params = {
            'probe_real': self.probe_dev, 'probe_imag': None, 'probe_defocus_mm': 0.0, 'probe_pos_offset': np.zeros([n_theta, 2]),
            'prj_pos_offset': np.zeros([n_theta, 2]), 'probe_pos_correction': np.tile(self.probe_pos - self.probe_pos_int, [n_theta, 1, 1]),
            'tilt_ls': np.zeros([3, n_theta])}
        if self.is_multi_dist:
            # ptychography.py:685-727, optimizers.py:905-943
            params.update(probe_pos_correction=np.zeros([self.n_dists, 2]), free_prop_cm=self.free_prop_cm,
                          safe_zone_width=self.safe_zone_width, ctf_lg_kappa=self.ctf_lg_kappa,
                          prj_affine_ls=np.tile(np.array([[1., 0, 0], [0, 1., 0]]).reshape([1, 2, 3]), [self.n_dists, 1, 1]))
        if self.is_sparse_multislice:
            # ptychography.py:718-719.  The engine's device array IS the parameter: the optimiser updates it in place
            params['slice_pos_cm_ls'] = self.engine.slice_pos
        self.refine_3d_dists = bool(self.holo_3d and getattr(self.engine, 'refine_distances', False))
        if self.refine_3d_dists:
            # likewise: the engine's distances are the parameter (plain Adam, no pin, no drift guard: optimizers.py:906-917)
            params['free_prop_cm'] = self.engine.dists
        self.refine_ctf_dists = bool(self.is_multi_dist and self.is_ctf and getattr(self.ctf_engine, 'refine_distances', False))
        if self.refine_ctf_dists:
            params['free_prop_cm'] = self.ctf_engine.dists       # (likewise; the CTF kernels read the array in every launch)
        # The optimised ones, in the order of the gradient tuple; one entry each (+ its gradient in the forward model)
        self.small, self.opt_args_ls = [], [0]
        if self.optimize_probe:
            self._add_small('probe_real', self.optimizer_probe, self.probe_learning_rate, name='probe', args=('probe_real', 'probe_imag'),
                            delay=self.probe_update_delay, limit=np.inf if self.probe_update_limit is None else self.probe_update_limit)
        if self.optimize_free_prop:
            self._add_small('free_prop_cm', self.optimizer_free_prop, self.free_prop_learning_rate)
        if self.optimize_prj_affine:
            # (+ "regularize transformation of image 0": matrix 0 is pinned to the identity)
            self._add_small('prj_affine_ls', self.optimizer_prj_affine, self.prj_affine_learning_rate,
                            pin=ctx.array(np.array([[1., 0, 0], [0, 1., 0]]), np.float32))
        if self.optimize_prj_pos_offset:
            # optimizers.py:863-875: plain gradient descent with a constant step unless an optimiser is supplied
            gd = GDOptimizer('prj_pos_offset', output_folder=self.output_folder,
                             options_dict={'step_size': self.prj_pos_offset_learning_rate, 'dynamic_rate': False})
            self._add_small('prj_pos_offset', self.optimizer_prj_pos_offset if self.optimizer_prj_pos_offset is not None else gd,
                            self.prj_pos_offset_learning_rate)
        if self.optimize_all_probe_pos:
            # optimizers.py:877-889: Adam on probe_pos_correction [n_theta, n_pos, 2] (+ "prevent position drifting": subtract the
            # mean over (theta, position))
            self._add_small('probe_pos_correction', self.optimizer_all_probe_pos, self.all_probe_pos_learning_rate, center_cols=2)
        if self.is_sparse_multislice and self.optimize_slice_pos:
            # optimizers.py:891-903, 1051-1060: Adam on the slice positions (+ "prevent position drifting": subtract the first)
            self._add_small('slice_pos_cm_ls', self.optimizer_slice_pos, self.slice_pos_learning_rate, anchor=True)
        if self.is_multi_dist and (self.is_ctf or self.fresnel_kappa):
            # a [1] array like the reference's (ptychography.py:732-733; float32 here), on the device whether it is refined or not:
            # the kernels read it there
            params['ctf_lg_kappa'] = ctx.array(np.array([float(self.ctf_lg_kappa)]), np.float32)
        if self.optimize_ctf_lg_kappa:
            # optimizers.py:945-956, 1077-1083: plain Adam on the [1] array, no pin, no drift guard
            self._add_small('ctf_lg_kappa', self.optimizer_ctf_lg_kappa, self.ctf_lg_kappa_learning_rate)
        self.ctf_lg_kappa_history = None      # (return_state: the value after every update, copied on the device)
        self.slice_pos_history = None         # (return_state: the positions after every update, copied on the device)
        self.prj_pos_offset_history = None    # (likewise: the offsets after every update)
        self.free_prop_cm_history = None      # (likewise: the distances of a 3-D object after every update)
        self.register_3d = bool(self.holo_3d and self.registration is not None)
        self.register_ctf = bool(self.is_multi_dist and self.is_ctf and self.registration is not None)
        self.prj_affine_history = None        # (likewise: the registration matrices of a 3-D object after every update)

        restored = self.restored_params
        if restored is not None:
            if 'probe_real' in restored and 'probe_imag' in restored:
                pr_ = np.stack([np.asarray(restored['probe_real']), np.asarray(restored['probe_imag'])], -1)
                if pr_.shape != self.probe_dev.shape:
                    raise ValueError('checkpointed probe has shape %s, this run uses %s' % (pr_.shape[:-1], self.probe_dev.shape[:-1]))
                self.probe_dev.set(pr_.astype(np.float32))
            for k_ in ('probe_pos_correction', 'free_prop_cm', 'prj_affine_ls', 'probe_defocus_mm', 'probe_pos_offset', 'prj_pos_offset',
                       'tilt_ls', 'slice_pos_cm_ls', 'ctf_lg_kappa'):
                if k_ in restored and k_ in params:
                    if hasattr(params[k_], 'set'):
                        params[k_].set(np.asarray(restored[k_], dtype=np.float32).reshape(params[k_].shape))
                    else:
                        params[k_] = restored[k_]
            if self.is_sparse_multislice:
                self.engine.slice_pos_changed()
            if self.refine_3d_dists or self.refine_ctf_dists:
                if self.refine_3d_dists:
                    self.engine.dists_changed()
                mom_ = self._small_moments('free_prop_cm')
                if mom_ is not None and 'free_prop_cm_moments' in restored:
                    for m_, h_ in zip(mom_, restored['free_prop_cm_moments']):
                        m_.set(np.asarray(h_, dtype=np.float32).reshape(m_.shape))
            if self.ctf_3d or self.refine_ctf_dists or self.register_ctf or self.fresnel_kappa:
                mom_ = self._small_moments('ctf_lg_kappa')
                if mom_ is not None and 'ctf_lg_kappa_moments' in restored:
                    for m_, h_ in zip(mom_, restored['ctf_lg_kappa_moments']):
                        m_.set(np.asarray(h_, dtype=np.float32).reshape(m_.shape))
            if self.register_3d or self.register_ctf:
                mom_ = self._small_moments('prj_affine_ls')
                if mom_ is not None and 'prj_affine_ls_moments' in restored:
                    for m_, h_ in zip(mom_, restored['prj_affine_ls_moments']):
                        m_.set(np.asarray(h_, dtype=np.float32).reshape(m_.shape))

        self.diff = Differentiator()
        self.diff.create_loss_node(self.forward_model.get_loss_function(), self.opt_args_ls)

    def _add_small(self, key, user_opt, learning_rate, name=None, args=None, delay=None, limit=np.inf, **extras):
        """Optimise optimizable_params[key] (moved to the device): the user's optimiser or Adam, its moments, its gradient accumulator
        and its place in the gradient tuple (the probe takes two: probe_real, probe_imag)."""
        name = name or key
        opt = user_opt if user_opt is not None else \
            AdamOptimizer(name, output_folder=self.output_folder, options_dict={'step_size': learning_rate}, forward_model=self.forward_model)
        opt.name = name
        x = self.optimizable_params[key]
        if not isinstance(x, DeviceArray):
            x = self.optimizable_params[key] = self.ctx.array(x, np.float32)
        opt.create_param_arrays(list(x.shape), device=self.ctx)
        opt.set_index_in_grad_return(len(self.opt_args_ls))
        self.opt_args_ls += [self.forward_model.get_argument_index(a) for a in args or (key,)]
        self.small.append(_SmallParam(key, opt, x, opt.index_in_grad_returns, self.other_params_update_delay if delay is None else delay,
                                      limit, **extras))

    def _params_to_host(self):
        """optimizable_params under the reference's keys, as host arrays (pickled whole into params_{rank}, misc.py:179-194)."""
        pa_ = self.probe_dev.get()
        out_ = {'probe_real': pa_[..., 0], 'probe_imag': pa_[..., 1]}
        for k_, v_ in self.optimizable_params.items():
            if k_ not in out_:
                out_[k_] = _host(v_)
        if self.refine_3d_dists or self.refine_ctf_dists:
            # (not part of the reference's format: the moments of the distances' optimiser, so that a resumed run continues the
            # uninterrupted one -- the reference restarts them at zero)
            mom_ = self._small_moments('free_prop_cm')
            if mom_ is not None:
                out_['free_prop_cm_moments'] = [m_.get() for m_ in mom_]
        if self.ctf_3d or self.refine_ctf_dists or self.register_ctf or self.fresnel_kappa:
            mom_ = self._small_moments('ctf_lg_kappa')        # (likewise, for the 3-D CTF run, the CTF runs that refine more and the tied Fresnel runs)
            if mom_ is not None:
                out_['ctf_lg_kappa_moments'] = [m_.get() for m_ in mom_]
        if self.register_3d or self.register_ctf:
            mom_ = self._small_moments('prj_affine_ls')       # (likewise)
            if mom_ is not None:
                out_['prj_affine_ls_moments'] = [m_.get() for m_ in mom_]
        return out_

    def _small_moments(self, key):
        """(m, v) of the built-in Adam that refines optimizable_params[key], or None (not refined, or the caller's optimiser)."""
        for p in self.small:
            d_ = getattr(p.opt, 'params_whole_array_dict', None) if p.key == key else None
            if d_ and isinstance(d_.get('m'), DeviceArray) and isinstance(d_.get('v'), DeviceArray):
                return d_['m'], d_['v']
        return None

    def run_epochs(self):
        """The convergence log and summary.txt, then the epoch loop (ptychography.py:783-1295) with the outputs of every epoch."""
        rank, output_folder = self.rank, self.output_folder
        if rank == 0:
            os.makedirs(os.path.join(output_folder, 'convergence'), exist_ok=True)
        self.comm.barrier()
        self.f_conv = open(os.path.join(output_folder, 'convergence', 'loss_rank_{}.txt'.format(rank)), 'w')
        self.f_conv.write('i_epoch,i_batch,loss,time\n')
        if rank == 0:       # adorym/ptychography.py:776 -> misc.py:149-176
            create_summary(output_folder, dict(self.call_args, output_folder=output_folder, probe_size=list(self.probe_size),
                                               n_theta=self.n_theta, obj_size=list(self.obj_size)), verbose=False)
        self.log('Optimizer started.')
        self.loss_history = []
        self.ckpt_thread = self.pending_log = None
        self.straddle_warned = False
        # Footprint-restricted gradient exchange (opt-in, ADM_RESTRICTED_EXCHANGE=1; DataParallelObject.exchange_and_update(touched=)):
        # only the y-planes the global batch touches are summed over the ranks, the regulariser term -- identical on every rank -- is
        # added R-fold by the shard owners.  Saves 1 - footprint/object of the reduce-scatter (58 % at 2 ranks, 20 % at 8 for
        # config 3's scan); never run on real multi-GPU hardware, hence not the default.
        self.restricted_exchange = (
            os.environ.get('ADM_RESTRICTED_EXCHANGE', '0') == '1' and self.n_ranks > 1 and self.builtin_model and not self.is_multi_dist
            and not self.rool and self.fused and self.optimize_object and self.unknown_type == 'delta_beta'
            and not any(isinstance(r_, ReweightedL1Regularizer) for r_ in self.forward_model.reg_list)
            and (self.update_scheme == 'immediate' or self.fuse_per_angle))
        # A small object (2-D ptychography, holography: a few hundred thousand unknowns) on one rank, plain Adam, no constraint
        # and no mask: its update is one more array of the ONE launch that updates the small parameters (same arithmetic --
        # adam_value in adm_optim.h -- and same step counter) unless the fused holography launch has updated it; these paths are
        # chains of 5-20 us kernels, where a launch saved is 5 % of a minibatch.
        self.obj_with_small = (self.optimize_object and plain_adam([self.opt]) is not None and self.n_ranks == 1 and self.flags == 0
                               and self.mask is None and self.state.n <= (1 << 22) and not self.restricted_exchange
                               and not self.ctf_direct)      # (the inversion sits between the object's step and kappa's)
        self.stage_next_targets = os.environ.get('ADM_STAGE_TARGETS', '1') == '1'

        self.i_epoch = self.starting_epoch
        while True:
            t0 = time.time()
            self.ind_list_rand = epoch_task_list(
                self.i_epoch, self.n_theta, len(self.probe_pos), self.minibatch_size, self.n_ranks, update_scheme=self.update_scheme,
                randomize_probe_pos=self.randomize_probe_pos,
                fixed_theta=(int(np.nonzero(abs(self.theta_ls - self.theta_ls[0]) < 1e-5)[0][0]) if self.two_d_mode else None))
            self.n_batch = len(self.ind_list_rand)
            self.i_opt_batch = self.starting_epoch * self.n_batch + self.starting_batch     # (:848), re-evaluated every epoch like the reference
            self.initialize_gradients = True
            self.pending_ind = []
            self.current_i_theta = -1                                                      # (:855)
            self.zeroed_by_update = set()
            for i_batch in range(self.starting_batch, self.n_batch):
                self.starting_batch = 0
                self.minibatch(i_batch)
            self._flush_log()
            self.state.finish_update()
            last = self.n_epochs != 'auto' and self.i_epoch == self.n_epochs - 1
            self.log('Epoch {} (rank {}); Delta-t = {} s; current time = {} s,'.format(self.i_epoch, rank, time.time() - t0,
                                                                                        time.time() - self.t_zero))
            self.i_epoch += 1
            if rank == 0:       # outputs after an epoch (ptychography.py:1290-1294; util.py:1958-2028)
                _write_images(output_folder, output_folder, '_ds_{}'.format(self.ds_level), self.obj.arr.get(), self.unknown_type,
                              self.probe_dev.get(), complex_probe=True)
            self.log('Current iteration finished.')
            if last:
                return

    def minibatch(self, i_batch):
        """Global batch ``i_batch`` of the epoch: checkpoint, look-ahead, gradient, object update, small-parameter update,
        intermediate output, log."""
        self._checkpoint(i_batch)
        batch = self._start_batch(i_batch)
        if batch is None:
            return          # 'per angle': collected for the angle's one launch
        this_i_theta, this_ind_batch, is_last_batch_of_this_theta, t00 = batch
        # ---- reweighted-L1 weights, refreshed every 10 minibatches (ptychography.py:995-1000) ----
        if self.reg_rwl1 is not None:
            if i_batch % 10 == 0:
                self.state.finish_update()
                _lib.check(self.ctx.lib.adm_rwl1_update(self.engine.plan.handle, self.obj.arr.ptr, self.rwl1_weight.ptr, self.rwl1_scratch.ptr))
            self.reg_rwl1.update_l1_weight(self.rwl1_weight)
        self._look_ahead(i_batch, this_i_theta)
        holo_fused = self._gradient(i_batch, this_i_theta, this_ind_batch)
        if self.update_scheme == 'per angle' and not is_last_batch_of_this_theta:
            self._flush_log()     # keeps at most one evaluation between a loss read-back and its use (two pinned slots)
            return
        self.initialize_gradients = True
        obj_with_small = self._update_object(i_batch, holo_fused)
        if self.ctf_direct:
            self._ctf_direct_update()
        self._update_small_params(i_batch, obj_with_small, holo_fused)

        # ---- intermediate output (ptychography.py:1231-1246; util.py:1958-2028, optimizers.py:1111-1160) ----
        if self.save_intermediate and ((self.save_intermediate_level == 'epoch' and i_batch == self.n_batch - 1)
                                       or self.save_intermediate_level == 'batch'):
            # finish_update() may hold a deferred collective (the rest of the all-gather): every rank calls it (the
            # condition is the same on all ranks)
            if is_last_batch_of_this_theta:
                self.state.finish_update()
                if self.rank == 0:
                    self._write_intermediate(i_batch)
            self.comm.barrier()

        # ---- finishing a batch (ptychography.py:1231-1271) ----
        fm = self.forward_model
        this_log = (self.i_epoch, i_batch, fm.take_loss_thunk() if self.builtin_model else (lambda v=fm.current_loss: v), t00)
        self._flush_log()                     # the PREVIOUS minibatch: its loss is read after this one has been queued
        self.pending_log = this_log
        if self.optimizer_batch_number_increment == 'batch' or (self.optimizer_batch_number_increment == 'angle' and is_last_batch_of_this_theta):
            self.i_opt_batch += 1

    def _checkpoint(self, i_batch):
        """Checkpoint (ptychography.py:879-895): device -> host copy here, file writes on a helper thread."""
        if not (self.store_checkpoint and i_batch % self.n_batch_per_checkpoint == 0):
            return
        if self.ckpt_thread is not None:
            self.ckpt_thread.join()
        self.state.finish_update()
        host_obj = self.obj.arr.get() if self.rank == 0 else None
        host_mom = [m_.get() for m_ in self.state.moments] if (self.rank == 0 or self.n_ranks > 1) else []
        self.ckpt_thread = threading.Thread(target=save_checkpoint, args=(self.i_epoch, i_batch, self.output_folder, host_obj, host_mom),
                                            kwargs=dict(rank=self.rank, n_ranks=self.n_ranks, params=self._params_to_host()))
        self.ckpt_thread.start()

    def _start_batch(self, i_batch):
        """Time limit, this rank's share of global batch ``i_batch`` and the rotate_out_of_loop rotation.  Returns (i_theta, position
        indices, whether the batch is the last of its angle, start time), or None while 'per angle' collects an angle's batches."""
        t_elapsed = (time.time() - self.t_zero) / 60
        if self.t_max_min is not None and self.n_ranks > 1:
            t_elapsed = self.comm.bcast_object(t_elapsed, root=0)     # one decision for all ranks: nobody is left in a collective
        if self.t_max_min is not None and t_elapsed >= self.t_max_min:
            self.log('Terminating program because maximum time limit is reached.')
            sys.exit()
        self.log('Epoch {}, batch {} of {} started.'.format(self.i_epoch, i_batch, self.n_batch))
        t00 = time.time()
        ind_list_rand = self.ind_list_rand
        this_i_theta, this_ind_batch = rank_batch(ind_list_rand, i_batch, self.rank, self.minibatch_size, self.n_ranks)
        # ONE decision for all ranks, taken on the angle the global batch starts with (rank 0's share).  The reference
        # compares with each rank's own angle (adorym/ptychography.py:910): when a global batch straddles two angles its
        # ranks then disagree, their optimiser counters i_opt_batch drift apart (:1266-1271) and the replicated objects
        # stop being identical (golden F14 'immediate' records it; oracle.reconstruct(rank_local_counters=True) restates
        # it).  Here the object is ONE sharded copy, so the step counter must be the same on every shard; the two rules
        # coincide whenever no global batch straddles angles (always in 'per angle' mode).
        is_last_batch_of_this_theta = i_batch == self.n_batch - 1 or ind_list_rand[i_batch + 1][0, 0] != ind_list_rand[i_batch][0, 0]
        if self.n_ranks > 1 and self.rank == 0 and self.i_epoch == self.starting_epoch and not self.straddle_warned and \
                len(np.unique(ind_list_rand[i_batch][:, 0])) > 1:
            self.straddle_warned = True
            self.log('  Note: this global batch holds positions of two angles.  adorym_amd keeps ONE optimiser step counter '
                     'for the sharded object (decided on the angle the batch starts with); the reference keeps one per rank and '
                     'its replicas drift apart in this case (INTEGRATION.md, "Deviations").  Use a position count that is a '
                     'multiple of n_ranks * minibatch_size, or update_scheme="per angle", to reproduce a reference mpirun.')
        self.log('  Current rank is processing angle ID {}.'.format(this_i_theta))

        # 'per angle': the minibatches of one angle see the same object, so they are fused into ONE launch
        # (identical sums; all CUs busy instead of `minibatch_size` of them).  The reference evaluates them
        # one by one and only logs the last (ptychography.py:1095-1099 `continue`).
        # ---- rotate_out_of_loop (ptychography.py:917-947): the object is rotated to the angle OUTSIDE the differentiated
        # block, once per change of angle -- the minibatches of the same angle that follow an 'immediate' update keep seeing
        # the object as it was rotated when the angle began, exactly like the reference ----
        if self.rool and this_i_theta != self.current_i_theta:
            self.state.finish_update()           # the whole object is read
            self.forward_model.rotate_outside(self.obj.arr, this_i_theta)
        self.current_i_theta = this_i_theta

        if self.update_scheme == 'per angle' and self.fuse_per_angle:
            self.pending_ind.append(this_ind_batch)
            if not is_last_batch_of_this_theta:
                return None
            self.forward_model.batch_group = len(self.pending_ind)
            this_ind_batch = np.concatenate(self.pending_ind)
            self.pending_ind = []
        return this_i_theta, this_ind_batch, is_last_batch_of_this_theta, t00

    def _look_ahead(self, i_batch, this_i_theta):
        """What the exchange and the next launches need before this minibatch's gradient is queued."""
        ind_list_rand, n_ranks, minibatch_size, fm = self.ind_list_rand, self.n_ranks, self.minibatch_size, self.forward_model
        # ---- footprint-restricted exchange: the planes the GLOBAL batch (all ranks) touches, the same on every rank ----
        self.touched_planes = None
        if self.restricted_exchange:
            if self.update_scheme == 'per angle':
                self.touched_planes = (0, self.obj_size[0])      # every position of the angle: the whole object
            else:
                gb_ = ind_list_rand[i_batch]
                if len(gb_) < n_ranks * minibatch_size:     # (a short last batch was topped up from batch 0 by rank_batch)
                    gb_ = np.concatenate([gb_, ind_list_rand[0][:n_ranks * minibatch_size - len(gb_)]])
                self.touched_planes = self.engine.y_footprint(self.probe_pos_int[gb_[:, 1]])
        fm.restricted_planes = self.touched_planes

        # ---- the next angle's rotation data, one minibatch ahead: when the NEXT global batch starts a new angle, its lookup table
        # is computed and uploaded now (host work while the GPU still runs the previous minibatch) and its adjoint CSR is built on
        # the side stream beside this minibatch's multislice kernel.  Met cold, the first launch of an angle waited 2 - 2.5 ms for
        # the host (table: NumPy + allocation; CSR: ~25 launches); the tables are kept for the whole reconstruction either way.
        # (The table is computed TWO minibatches ahead, the CSR and -- for datasets small enough to live on the device -- the angle's
        # measured data ONE ahead: the host is at most a minibatch ahead of the GPU and each of these costs it 1 - 2 ms.)
        if self.builtin_model and not self.two_d_mode and not self.is_multi_dist and not self.rool:
            def _angle_of(i_b):
                nb_ = ind_list_rand[i_b]
                return int(nb_[min(self.rank * minibatch_size, len(nb_) - 1), 0])
            if i_batch + 2 < self.n_batch and _angle_of(i_batch + 2) != this_i_theta:
                self.rotation_tables(_angle_of(i_batch + 2))
            if i_batch + 1 < self.n_batch and _angle_of(i_batch + 1) != this_i_theta:
                fm.prefetch_table = self.rotation_tables(_angle_of(i_batch + 1))
                fm.prefetch_data(_angle_of(i_batch + 1))

    def _next_evaluation(self, i_b):
        """(i_theta, position indices) of the evaluation that follows global batch ``i_b`` on this rank within the epoch, or None:
        the next minibatch ('immediate'), or all minibatches of the next angle as the fused 'per angle' launch takes them."""
        ind_list_rand, n_batch = self.ind_list_rand, self.n_batch
        if i_b + 1 >= n_batch:
            return None
        th, ind = rank_batch(ind_list_rand, i_b + 1, self.rank, self.minibatch_size, self.n_ranks)       # (tops up a short last batch now)
        if not (self.update_scheme == 'per angle' and self.fuse_per_angle):
            return th, ind
        group, j = [ind], i_b + 2
        while j < n_batch and ind_list_rand[j][0, 0] == ind_list_rand[i_b + 1][0, 0]:
            group.append(rank_batch(ind_list_rand, j, self.rank, self.minibatch_size, self.n_ranks)[1])
            j += 1
        return th, np.concatenate(group)

    def _gradient(self, i_batch, this_i_theta, this_ind_batch):
        """Gradients (ptychography.py:1017-1066): the object's into its buffer, the small parameters' added to their accumulators.
        Returns the fused holography update's arguments when that launch has also updated them all, else None."""
        ctx, state, fm = self.ctx, self.state, self.forward_model
        t_grad_0 = time.time()
        side_hook, init_grad = None, False
        if self.initialize_gradients:
            if self.builtin_model:
                # queued by the model on the side stream after the rotation: the deferred part of the previous update,
                # then the regulariser kernel in 'set' mode (or a zero fill) initialises the gradient buffer
                side_hook, init_grad = state.finish_update, True
            else:
                state.zero_grad()
            # (an accumulator that the last small-parameter update consumed was zero-filled by that launch)
            for p in self.small:
                if p.key not in self.zeroed_by_update:
                    p.g.zero_()
            self.zeroed_by_update = set()
        given = {'obj': fm.arr_rot if self.rool else self.obj.arr,     # (:1009-1013)
                 'this_i_theta': this_i_theta, 'this_pos_batch': self.probe_pos_int[this_ind_batch], 'this_ind_batch': this_ind_batch,
                 'prj': self.prj}
        grad_func_args = {arg: given[arg] if arg in given else self.optimizable_params[arg] for arg in fm.argument_ls}
        fm.update_loss_args(grad_func_args)
        holo_fused = self._holo_fused(i_batch, init_grad)
        if self.is_multi_dist and self.builtin_model:
            fm.fused_adam = holo_fused
        # which measured data the NEXT evaluation needs, so that the model can send them to the device beside this one's launch
        # (streamed datasets; resident ones are views of device arrays already)
        if self.builtin_model and not self.is_multi_dist and self.stage_next_targets:
            fm.next_batch = self._next_evaluation(i_batch)
        grads = self.diff.get_gradients(_accumulate_into=self.gradient.arr, _side_hook=side_hook, _init_grad=init_grad, **grad_func_args)
        self.log('  Gradient calculation done in {} s.'.format(time.time() - t_grad_0))
        self.initialize_gradients = False
        if self.rool:
            # (:1066-1078) the gradient buffer is in the rotated frame: resample it with the -theta table, after EVERY
            # minibatch and on everything accumulated so far.  In 'per angle' mode earlier contributions are therefore
            # resampled again (the reference's TODO at :1075 says they should not be); kept literally -- golden F15
            # pins it -- and the minibatches of an angle are not fused into one launch in this mode for that reason.
            fm.resample_gradient(self.gradient.arr, this_i_theta)
        if holo_fused is not None:
            for o_ in holo_fused['opts']:
                o_.i_batch += 1
            return holo_fused
        for p in self.small:
            g_ = grads[p.i_grad]            # (the probe's: interleaved (real, imag))
            _lib.check(ctx.lib.adm_axpy(ctx.handle, p.g.ptr, g_.ptr, 1.0, g_.size))
        return None

    def _holo_fused(self, i_batch, init_grad):
        """Multi-distance holography whose update is exactly "Adam on what this minibatch's gradients say" -- one rank, an update per
        minibatch, no regulariser, constraint or mask on the object, plain Adam with common (b1, b2, eps) on the object and on
        whichever of free_prop_cm / prj_affine_ls are optimised: the steps run INSIDE the gradient launch group's last kernel
        (adm_holo_fwd_adj_adam; same arithmetic, same bits), no gradient is stored and no optimiser launch follows."""
        if not (self.is_multi_dist and not self.holo_tiled and not self.holo_3d and not self.is_ctf and self.builtin_model and init_grad and self.update_scheme == 'immediate'
                and self.optimize_object and self.n_ranks == 1 and self.flags == 0 and self.mask is None
                and all(p.key in _HOLO_FUSED_SLOTS for p in self.small) and not self.forward_model.reg_list
                and os.environ.get('ADM_HOLO_FUSED_ADAM', '1') == '1'):
            return None
        betas = plain_adam([self.opt] + [p.opt for p in self.small])
        if betas is None:
            return None
        holo_fused = dict(obj_mv=(self.state.moments[0], self.state.moments[1]), step_obj=float(self.opt.options_dict.get('step_size', 0.001)),
                          i_batch=self.i_opt_batch, b1=betas[0], b2=betas[1], eps=betas[2], dists=None, affine=None, pin=None, opts=[self.opt])
        for p in self.small:
            if p.due(i_batch + self.i_epoch * self.n_batch):
                o_, slot = p.opt, _HOLO_FUSED_SLOTS[p.key]
                holo_fused[slot] = (o_.params_whole_array_dict['m'], o_.params_whole_array_dict['v'], float(o_.options_dict.get('step_size', 0.001)))
                if slot == 'affine':
                    holo_fused['pin'] = p.extras['pin']
                holo_fused['opts'].append(o_)
        self.state.finish_update()
        return holo_fused

    def _update_object(self, i_batch, holo_fused):
        """Exchange + update + constraints + mask (ptychography.py:1113-1158, 1210-1215).  Returns True when the object's update is
        left to the small parameters' launch instead."""
        state, opt, n_ranks, obj_size = self.state, self.opt, self.n_ranks, self.obj_size
        obj_with_small = self.obj_with_small and holo_fused is None
        if not self.optimize_object or obj_with_small or holo_fused is not None:
            return obj_with_small
        mask = self.mask.mask if self.mask is not None else None
        if not self.fused:
            opt.apply_gradient(self.obj.arr, self.gradient, self.i_opt_batch, flags=self.flags, mask=mask, **opt.options_dict)
            return False
        o = dict(opt.options_dict)
        if self.opt_kind == 'gd':
            o['step_size'] = GDOptimizer.scheduled_step(self.i_opt_batch, o.get('step_size', 0.001), o.get('dynamic_rate', True),
                                                        o.get('first_downrate_iteration', 92))
        first = None
        plane = obj_size[1] * obj_size[2] * 2
        if (n_ranks == 1 or state.overlap_gather) and self.builtin_model and not self.is_multi_dist and i_batch + 1 < self.n_batch \
                and not self.rool:
            # one rank: update the y-planes the next minibatch reads first; several ranks: gather the planes the
            # next minibatches of ALL ranks read first (the same range on every rank: it shapes a collective).
            # The rest -- of the element-wise update, or of the all-gather -- is queued by that minibatch on the
            # side stream (DataParallelObject.finish_update), beside its multislice kernel
            rank_batch(self.ind_list_rand, i_batch + 1, 0, self.minibatch_size, n_ranks)    # tops up a short last batch now
            nxt = self.ind_list_rand[i_batch + 1]
            ny0, ny1 = self.engine.y_footprint(self.probe_pos_int[nxt[:n_ranks * self.minibatch_size, 1]])
            if self.update_scheme == 'per angle' and self.fuse_per_angle:
                ny0, ny1 = 0, obj_size[0]
            first = (ny0 * plane, ny1 * plane)
        xkw = {}
        if self.touched_planes is not None:
            ad_, ab_, gm_ = combined_weights(self.forward_model.reg_list)
            mult_ = float(n_ranks * self.forward_model.batch_group)     # every rank adds the term once per fused minibatch

            def _reg_shard(lo_, hi_, alo_, ahi_):
                _lib.check(self.ctx.lib.adm_reg_grad_range(self.engine.plan.handle, self.obj.arr.ptr, ad_ * mult_, ab_ * mult_, gm_ * mult_,
                                                           self.gradient.arr.ptr, lo_, hi_, alo_, ahi_))
            xkw = dict(touched=(self.touched_planes[0] * plane, self.touched_planes[1] * plane), reg_shard=_reg_shard)
        state.exchange_and_update(self.opt_kind, self.i_opt_batch, o, flags=self.flags, mask=mask, first=first, **xkw)
        return False

    def _ctf_direct_update(self):
        """update_using_external_algorithm='ctf' (ptychography.py:1135-1163, array_ops.py:274-286): behind the object's step and its
        constraints the delta channel is overwritten with the direct CTF inversion of angle 0's holograms at the distances given and
        the CURRENT lg_kappa on the device -- as it was before this minibatch's kappa step.  (The reference reads the function
        argument ctf_lg_kappa, a float, with [0] there, and never the refined value.)  Beta is not touched."""
        if self.ctf_direct_data is None:
            self.ctf_direct_data = self.ctx.array(np.ascontiguousarray(np.asarray(self.prj[0]), dtype=np.float32), np.float32)
        self.state.finish_update()
        self.ctf_inversion.retrieve(self.ctf_direct_data, self.free_prop_cm, self.optimizable_params['ctf_lg_kappa'], out=self.obj.arr,
                                    into_object=True)

    def _update_small_params(self, i_batch, obj_with_small, holo_fused):
        """The small parameters (optimizers.py:1022-1083): probe, sub-pixel positions, propagation distances, affine registration.
        Gradients are summed over the ranks on the device, then ONE launch updates them all (per-array Adam, the drift guard of the
        positions, the identity pin of affine matrix 0, and the zero fill of the accumulators for the next minibatch); custom
        optimiser objects fall back to their own apply_gradient."""
        items = []
        if obj_with_small:
            self.state.finish_update()
            items.append(dict(opt=self.opt, x=self.state.obj.view(0, (self.state.n,)), g=self.state.grad.view(0, (self.state.n,))))
        i_global = i_batch + self.i_epoch * self.n_batch
        due = []
        for p in self.small if holo_fused is None else ():     # (the fused holography launch has updated them already)
            if p.due(i_global):
                due.append(p)
            elif p.key == 'probe_real':
                print_flush('  Probe is not updated because current batch is out of the specified range ({}, {}).'.format(p.delay, p.limit),
                            0, self.rank, **self.stdout_options)
        items += [dict(opt=p.opt, x=p.x, g=p.g, zero_grad=True, **p.extras) for p in due]      # (accumulators zero-filled once used)
        if self.n_ranks > 1:
            for it_ in items:
                self.comm.all_reduce_device(it_['g'])
        apply_small_params(self.ctx, items, self.i_opt_batch)
        self.zeroed_by_update = {p.key for p in due}
        if any(p.key == 'slice_pos_cm_ls' for p in due):
            self.engine.slice_pos_changed()       # the gaps' transfer functions are rebuilt in front of the next launch
            if self.return_state and self.n_epochs != 'auto':
                z = self.engine.slice_pos
                if self.slice_pos_history is None:
                    self.slice_pos_history = [self.ctx.zeros((int(self.n_epochs) * self.n_batch, z.size)), 0]
                hist, k = self.slice_pos_history
                if k < hist.shape[0]:
                    _lib.check(self.ctx.lib.adm_d2d(self.ctx.handle, hist.ptr + 4 * z.size * k, z.ptr, z.nbytes))
                    self.slice_pos_history[1] = k + 1
        if (self.refine_3d_dists or self.refine_ctf_dists) and any(p.key == 'free_prop_cm' for p in due):
            if self.refine_3d_dists:
                self.engine.dists_changed()       # the detector planes' kernels are rebuilt in front of the next launch
            if self.return_state and self.n_epochs != 'auto':
                x = self.optimizable_params['free_prop_cm']       # (the engine's own array)
                if self.free_prop_cm_history is None:
                    self.free_prop_cm_history = [self.ctx.zeros((int(self.n_epochs) * self.n_batch, x.size)), 0]
                hist, k = self.free_prop_cm_history
                if k < hist.shape[0]:
                    _lib.check(self.ctx.lib.adm_d2d(self.ctx.handle, hist.ptr + 4 * x.size * k, x.ptr, x.nbytes))
                    self.free_prop_cm_history[1] = k + 1
        if (self.register_3d or self.register_ctf) and any(p.key == 'prj_affine_ls' for p in due) and self.return_state and self.n_epochs != 'auto':
            x = self.optimizable_params['prj_affine_ls']
            if self.prj_affine_history is None:
                self.prj_affine_history = [self.ctx.zeros((int(self.n_epochs) * self.n_batch,) + tuple(x.shape)), 0]
            hist, k = self.prj_affine_history
            if k < hist.shape[0]:
                _lib.check(self.ctx.lib.adm_d2d(self.ctx.handle, hist.ptr + 4 * x.size * k, x.ptr, x.nbytes))
                self.prj_affine_history[1] = k + 1
        if any(p.key == 'ctf_lg_kappa' for p in due) and self.return_state and self.n_epochs != 'auto':
            x = self.optimizable_params['ctf_lg_kappa']
            if self.ctf_lg_kappa_history is None:
                self.ctf_lg_kappa_history = [self.ctx.zeros((int(self.n_epochs) * self.n_batch,)), 0]
            hist, k = self.ctf_lg_kappa_history
            if k < hist.shape[0]:
                _lib.check(self.ctx.lib.adm_d2d(self.ctx.handle, hist.ptr + 4 * k, x.ptr, x.nbytes))
                self.ctf_lg_kappa_history[1] = k + 1
        if any(p.key == 'prj_pos_offset' for p in due) and self.return_state and self.n_epochs != 'auto':
            x = self.optimizable_params['prj_pos_offset']
            if self.prj_pos_offset_history is None:
                self.prj_pos_offset_history = [self.ctx.zeros((int(self.n_epochs) * self.n_batch,) + tuple(x.shape)), 0]
            hist, k = self.prj_pos_offset_history
            if k < hist.shape[0]:
                _lib.check(self.ctx.lib.adm_d2d(self.ctx.handle, hist.ptr + 4 * x.size * k, x.ptr, x.nbytes))
                self.prj_pos_offset_history[1] = k + 1

    def _write_intermediate(self, i_batch):
        """output_object(full_output=False) + output_intermediate_parameters of the reference: object TIFFs under
        intermediate/object (named by (epoch, batch) when save_history, else overwritten), and one file set per optimised
        parameter under intermediate/<what>."""
        i_epoch, params, folder = self.i_epoch, self.optimizable_params, os.path.join(self.output_folder, 'intermediate')
        tag = '_{}_{}'.format(i_epoch, i_batch) if self.save_history else ''
        probe = self.probe_dev.get() if self.optimize_probe else None
        _write_images(os.path.join(folder, 'object'), os.path.join(folder, 'probe'), tag, self.obj.arr.get(), self.unknown_type, probe)
        for p in self.small:
            if p.key == 'probe_real':
                continue
            d_ = os.path.join(folder, {'probe_pos_correction': 'probe_pos', 'prj_affine_ls': 'prj_affine'}.get(p.key, p.key))
            os.makedirs(d_, exist_ok=True)
            if p.key == 'ctf_lg_kappa':
                continue          # (the reference creates the folder, optimizers.py:1092-1109, and writes nothing into it, :1111-1160)
            v_ = np.asarray(_host(params[p.key]))
            if p.key == 'probe_pos_correction' and self.is_multi_dist:
                np.savetxt(os.path.join(d_, 'probe_pos_correction_{}_{}.txt'.format(i_epoch, i_batch)), v_)
            elif p.key == 'probe_pos_correction':
                for i_t in range(self.n_theta):
                    np.savetxt(os.path.join(d_, 'probe_pos_correction_{}_{}_{}.txt'.format(i_epoch, i_batch, i_t)), v_[i_t])
            elif p.key == 'prj_affine_ls':
                np.savetxt(os.path.join(d_, 'prj_affine_{}.txt'.format(i_epoch)), np.concatenate(v_, 0))
            elif p.key == 'prj_pos_offset':         # one line per output, appended (optimizers.py:1135-1138)
                with open(os.path.join(d_, 'prj_pos_offset.txt'), 'a' if i_batch > 0 or i_epoch > 0 else 'w') as f_:
                    f_.write('{:4d}, {:4d}, {}\n'.format(i_epoch, i_batch, [float(x_) for x_ in v_.flatten()]))
            else:
                np.savetxt(os.path.join(d_, '{}_{}.txt'.format(p.key, i_epoch)), np.atleast_1d(v_))

    def _flush_log(self):
        if self.pending_log is None:
            return
        e_, b_, thunk, t_start = self.pending_log
        self.pending_log = None
        current_loss = thunk()
        self.loss_history.append(current_loss)
        self.log('Minibatch/angle done in {} s; loss (rank 0) is {}.'.format(time.time() - t_start, current_loss))
        self.log('Throughput: {} angles/sec'.format(self.minibatch_size / (time.time() - t_start)))
        self.f_conv.write('{},{},{},{}\n'.format(e_, b_, current_loss, time.time() - self.t_zero))
        self.f_conv.flush()

    def finish(self):
        """Outputs: the checkpoint writer is waited for, the files are closed, and with return_state the final arrays returned."""
        if self.ckpt_thread is not None:
            self.ckpt_thread.join()
        self.comm.barrier()
        self.f_conv.close()
        self.f.close()
        if not self.return_state:
            return None
        arr, pa, params = self.obj.arr.get(), self.probe_dev.get(), self.optimizable_params
        return {'delta': arr[..., 0], 'beta': arr[..., 1], 'probe_real': pa[..., 0], 'probe_imag': pa[..., 1],
                'probe_pos_correction': np.asarray(_host(params['probe_pos_correction'])),
                'free_prop_cm': _host(params.get('free_prop_cm', self.free_prop_cm)), 'prj_affine_ls': _host(params.get('prj_affine_ls')),
                'free_prop_cm_history': (None if self.free_prop_cm_history is None
                                         else self.free_prop_cm_history[0].get()[:self.free_prop_cm_history[1]]),
                'prj_affine_history': None if self.prj_affine_history is None else self.prj_affine_history[0].get()[:self.prj_affine_history[1]],
                'slice_pos_cm_ls': _host(params.get('slice_pos_cm_ls')),
                'slice_pos_history': None if self.slice_pos_history is None else self.slice_pos_history[0].get()[:self.slice_pos_history[1]],
                'prj_pos_offset': np.asarray(_host(params['prj_pos_offset'])),
                'prj_pos_offset_history': (None if self.prj_pos_offset_history is None
                                           else self.prj_pos_offset_history[0].get()[:self.prj_pos_offset_history[1]]),
                'ctf_lg_kappa': None if 'ctf_lg_kappa' not in params else np.asarray(_host(params['ctf_lg_kappa'])).reshape(-1),
                'ctf_lg_kappa_history': (None if self.ctf_lg_kappa_history is None
                                         else self.ctf_lg_kappa_history[0].get()[:self.ctf_lg_kappa_history[1]]),
                'losses': self.loss_history, 'output_folder': self.output_folder,
                # which multislice path served the run
                # (a 3-D CTF run has no multislice engine: its projector answers False to both)
                'engine_streamed': bool(getattr(self.engine, 'streamed', False)),
                'engine_probe_shift': bool(getattr(self.engine, 'probe_shift', False))}
