"""
Forward models with the reference's plugin interface (adorym/forward_model.py:28-175, 164-401):
``predict`` / ``get_data`` / ``loss`` / ``get_loss_function`` keep their names, argument order and
meaning; the arithmetic runs in libadm's HIP kernels through a MultisliceEngine.

Differences that follow from having no autograd: the closure returned by ``get_loss_function`` carries
a reference to its model (``calculate_loss.forward_model``) so that ``Differentiator.get_gradients`` can
call the hand-derived adjoint (``loss_and_gradients``) instead of ``torch.autograd.grad``.
"""
import inspect
import os
import numpy as np

from ._lib import check
from .device import DeviceArray
from .propagate import RotationTable, ProjectionEngine
from .regularizers import combined_weights


class ForwardModel(object):
    """adorym/forward_model.py:28-161."""

    def __init__(self, loss_function_type='lsq', distribution_mode=None, device=None, common_vars_dict=None,
                 raw_data_type='magnitude', simulation_mode=False):
        if distribution_mode is not None:
            raise NotImplementedError("distribution_mode '%s' is outside the accelerated path (DP only)" % distribution_mode)
        if loss_function_type not in ('lsq', 'poisson'):
            raise ValueError("loss_function_type must be 'lsq' or 'poisson'")
        if raw_data_type not in ('magnitude', 'intensity'):
            raise ValueError("raw_data_type must be 'magnitude' or 'intensity'")
        self.loss_function_type = loss_function_type
        self.argument_ls = []
        self.regularizer_dict = {}
        self.distribution_mode = distribution_mode
        self.device = device                      # adorym_amd.Context
        self.simulation_mode = simulation_mode
        self._current_loss = 0
        self._loss_thunk = None
        self.raw_data_type = raw_data_type
        self.i_call = 0
        self.common_vars = common_vars_dict
        if common_vars_dict is not None:
            for k in ('unknown_type', 'normalize_fft', 'sign_convention', 'rotate_out_of_loop', 'scale_ri_by_k',
                      'is_minus_logged', 'forward_algorithm', 'stdout_options', 'poisson_multiplier', 'common_probe_pos',
                      'binning', 'prj'):
                setattr(self, k, common_vars_dict.get(k))
        self.loss_args = {}
        self.reg_list = []

    @property
    def current_loss(self):
        """Loss of the last evaluation (adorym/forward_model.py:141-146).  The GPU path queues its read-back without
        blocking; the value is fetched the first time it is looked at."""
        if self._loss_thunk is not None:
            t, self._loss_thunk = self._loss_thunk, None
            self._current_loss = float(t())
        return self._current_loss

    @current_loss.setter
    def current_loss(self, v):
        self._loss_thunk = None
        self._current_loss = v

    def take_loss_thunk(self):
        """Detach the pending loss read-back (a callable returning the float) so that the caller can resolve it later,
        after more work has been queued; returns None if the loss is already on the host."""
        t, self._loss_thunk = self._loss_thunk, None
        if t is None:
            v = self._current_loss
            return lambda: v
        return t

    def update_loss_args(self, kwargs):
        self.loss_args = kwargs

    def add_regularizers(self, reg_list):
        self.reg_list = reg_list

    def get_argument_index(self, arg):
        for i, a in enumerate(self.argument_ls):
            if a == arg:
                return i
        raise ValueError('{} is not in the argument list.'.format(arg))

    # ---- the plugin contract's last-layer pieces (adorym/forward_model.py:75-147) -------------------------------------
    # A forward-model plugin whose predict() returns magnitudes on the HOST combines them with these exactly as the
    # reference's ForwardModel does.  The built-in models do not go through them: their loss is evaluated inside the
    # multislice kernel (loss_term, adm_ms_math.h) and the regulariser inside reg_grad_kernel.
    def get_regularization_value(self, obj, device=None):
        """Sum of the registered regularisers' values for ``obj`` (DeviceArray [Y,X,Z,2]); adorym/forward_model.py:75-80."""
        reg = float(self._regularize(obj, None)) if hasattr(self, '_regularize') else 0.0
        return reg

    def get_mismatch_loss(self, this_pred_batch, this_prj_batch):
        """LSQ / Poisson mismatch of predicted magnitudes and measured data (host arrays), adorym/forward_model.py:88-103."""
        pred = np.asarray(this_pred_batch, dtype=np.float32)
        meas = np.abs(np.asarray(this_prj_batch)).astype(np.float32)
        pm = np.float32(getattr(self, 'poisson_multiplier', None) or 1.)
        if self.loss_function_type == 'lsq':
            if self.raw_data_type == 'intensity':
                meas = np.sqrt(meas)
            return np.mean((pred - meas) ** 2)
        if self.raw_data_type == 'magnitude':
            meas = meas ** 2
        return np.mean(pred ** 2 * pm - meas * pm * np.log(pred ** 2 * pm))

    def loss(self, this_pred_batch, this_prj_batch, obj):
        """(Regularised) loss from predicted MAGNITUDES, with the beamstop selection of adorym/forward_model.py:121-147;
        stores ``current_loss``."""
        pred = np.asarray(this_pred_batch)
        meas = np.asarray(this_prj_batch)
        beamstop = self.common_vars.get('beamstop') if self.common_vars else None
        if beamstop is not None:
            keep = np.asarray(beamstop) >= 1e-5
            pred = pred[:, keep]
            meas = meas[:, keep]
        val = float(self.get_mismatch_loss(pred, meas))
        if len(self.reg_list) > 0:
            val += float(self.get_regularization_value(obj, device=self.device))
        self.current_loss = val
        return val

    def get_data(self, this_i_theta, this_ind_batch, theta_downsample=None, ds_level=1):
        """abs(prj[i_theta*theta_downsample, ind_batch]) (forward_model.py:113-119); sqrt of it for intensity
        data (the sqrt of get_mismatch_loss, :92-93, folded in here).  Returns a float32 host array."""
        if theta_downsample is None:
            theta_downsample = 1
        if ds_level not in (1, None):
            raise NotImplementedError('multiscale (ds_level > 1) is outside the accelerated path')
        t = np.abs(np.asarray(self.prj[int(this_i_theta) * theta_downsample, np.asarray(this_ind_batch)]))
        if self.loss_function_type == 'lsq':
            if self.raw_data_type == 'intensity':
                t = np.sqrt(t)
        else:   # Poisson compares intensities (forward_model.py:94-102): |prj|^2 for magnitude data, |prj| for intensity data
            if self.raw_data_type == 'magnitude':
                t = t ** 2
        return np.ascontiguousarray(t, dtype=np.float32)

    def predict(self, *args, **kwargs):
        raise NotImplementedError

    def get_loss_function(self):
        raise NotImplementedError


class PtychographyModel(ForwardModel):
    """
    adorym/forward_model.py:164-401.  Also serves the reference's SingleBatchFullfieldModel and
    SingleBatchPtychographyModel (:404-586): they compute the same function with fewer stacking steps.
    """

    def __init__(self, loss_function_type='lsq', distribution_mode=None, device=None, common_vars_dict=None,
                 raw_data_type='magnitude', simulation_mode=False, run_bfloat16=False, run_float64=False):
        super(PtychographyModel, self).__init__(loss_function_type, distribution_mode, device, common_vars_dict,
                                                raw_data_type, simulation_mode=simulation_mode)
        if run_bfloat16 or run_float64:
            raise NotImplementedError('the HIP path computes in fp32 (the reference default); bf16/fp64 runs are not provided')
        args = inspect.getfullargspec(self.predict).args
        args.pop(0)
        self.argument_ls = args
        self.engine = common_vars_dict['engine'] if common_vars_dict else None
        self.pure_projection = bool(common_vars_dict.get('pure_projection')) if common_vars_dict else False
        if self.pure_projection:
            self._check_projection()
        self._probe_dev = None
        self._grad_probe_dev = None
        self._reg_val = None
        # >1 when the driver fuses the minibatches of one angle ('per angle' update scheme) into one launch:
        # the batch then holds `batch_group` reference minibatches whose losses are summed
        self.batch_group = 1

    # ------------------------------------------------------------------ helpers
    # flags of the reference that this model refuses by name (optimize_prj_pos_offset is served: _offset_args)
    REFUSED_FLAGS = ('optimize_probe_defocusing', 'optimize_probe_pos_offset', 'optimize_tilt')
    GRADIENTS = ('obj', 'probe_real', 'probe_imag', 'probe_pos_correction', 'prj_pos_offset')     # (of loss_and_gradients; any other is refused)

    PROJECTION_MODEL = 'the projection approximation'      # (the subclasses that cannot serve it say what they are instead)

    def _check_projection(self):
        """pure_projection=True (adorym/propagate.py:158-193): the engine is a ProjectionEngine -- rotate() sums the rotated object
        along the beam, the launch is the one-slice problem, rotate_adjoint() copies its gradient to every slice -- and nothing
        else changes here; an object that has one slice runs on the ordinary engine.  ``binning`` has no effect on this model."""
        cv = self.common_vars
        refused = (
            (self.PROJECTION_MODEL != PtychographyModel.PROJECTION_MODEL, self.PROJECTION_MODEL),
            (cv.get('unknown_type', 'delta_beta') == 'real_imag', "unknown_type='real_imag'"),
            (bool(cv.get('is_minus_logged')), 'is_minus_logged'),
            (cv.get('forward_algorithm', 'fresnel') not in (None, 'fresnel'), "forward_algorithm='%s'" % cv.get('forward_algorithm')),
            (bool(cv.get('optimize_prj_pos_offset')), 'optimize_prj_pos_offset'),
            (bool(cv.get('rotate_out_of_loop')), 'rotate_out_of_loop'))
        for cond, what in refused:
            if cond:
                raise NotImplementedError('pure_projection with %s is outside the accelerated path of adorym_amd' % what)
        if self.engine is not None and not isinstance(self.engine, ProjectionEngine) and self.engine.obj_size[2] > 1:
            raise ValueError('pure_projection needs an adorym_amd.ProjectionEngine for an object of %d slices' % self.engine.obj_size[2])

    def _check_static(self, probe_defocus_mm, probe_pos_offset, probe_pos_correction, prj_pos_offset):
        cv = self.common_vars
        for flag in self.REFUSED_FLAGS:
            if cv.get(flag):
                raise NotImplementedError('%s is outside the accelerated path (SURVEY section 8 f2)' % flag)

    def _offset_args(self, prj_pos_offset, this_i_theta, B):
        """forward_model.py:255-256, 352: with optimize_prj_pos_offset every position of the minibatch carries the offset of its
        angle, prj_pos_offset[this_i_theta], applied to the exit wave (MultisliceEngine.multislice(exit_shifts=...)).  Returns
        (offsets DeviceArray [n_theta, 2], index DeviceArray int32 [B], all this_i_theta) or (None, None)."""
        if not self.common_vars.get('optimize_prj_pos_offset'):
            return None, None
        if prj_pos_offset is None:
            raise ValueError('optimize_prj_pos_offset is set but no prj_pos_offset was passed')
        if not getattr(self.engine, 'exit_shift', False):
            raise ValueError('optimize_prj_pos_offset needs an engine built with exit_shift=True')
        if isinstance(prj_pos_offset, DeviceArray):
            dev = prj_pos_offset
        else:
            host = np.ascontiguousarray(np.asarray(prj_pos_offset, dtype=np.float32).reshape(-1, 2))
            key = (host.shape, host.tobytes())
            if getattr(self, '_offset_key', None) != key:
                self._offset_dev = self.device.array(host)
                self._offset_key = key
            dev = self._offset_dev
        if not 0 <= int(this_i_theta) < dev.size // 2:
            raise ValueError('prj_pos_offset holds %d angles, angle %d was asked for' % (dev.size // 2, int(this_i_theta)))
        # one resident index array per angle (constant this_i_theta), grown when a larger batch comes: no upload in the minibatch
        cache = self.__dict__.setdefault('_offset_idx', {})
        idx = cache.get(int(this_i_theta))
        if idx is None or idx.size < B:
            idx = cache[int(this_i_theta)] = self.device.array(np.full(max(B, 64), int(this_i_theta), dtype=np.int32))
        return dev, idx.view(0, (B,))

    def _shift_args(self, probe_pos_correction, this_i_theta, this_ind_batch):
        """forward_model.py:297-311: the probes are Fourier-shifted per position when the corrections are being optimised or
        any of them exceeds 1e-3 (sic: positive values only).  Returns (shifts DeviceArray [n_theta*n_pos, 2], index
        DeviceArray int32 [B]) or (None, None)."""
        if probe_pos_correction is None:
            return None, None
        if isinstance(probe_pos_correction, DeviceArray):
            dev = probe_pos_correction
            active = bool(self.common_vars.get('optimize_all_probe_pos')) or getattr(self, '_static_shift_active', None)
            if active is None:
                active = self._static_shift_active = bool(np.any(dev.get() > 1e-3))
        else:
            host = np.ascontiguousarray(np.asarray(probe_pos_correction, dtype=np.float32))
            active = bool(self.common_vars.get('optimize_all_probe_pos')) or bool(np.any(host > 1e-3))
            if not active:
                return None, None
            key = (host.shape, host.tobytes())
            if getattr(self, '_corr_key', None) != key:
                self._corr_dev = self.device.array(host)
                self._corr_key = key
            dev = self._corr_dev
        if not active:
            return None, None
        n_pos = dev.shape[-2] if len(dev.shape) >= 2 else dev.size // 2
        idx = (int(this_i_theta) * n_pos + np.asarray(this_ind_batch, dtype=np.int64)).astype(np.int32)
        if len(idx) > 0 and int(idx[-1]) - int(idx[0]) == len(idx) - 1 and np.all(np.diff(idx) == 1):
            # a run of consecutive entries (the reference sorts a minibatch's indices, adorym/ptychography.py:907): a view of a
            # resident 0, 1, 2, ... array -- no upload, no copy kernel in the minibatch
            n_all = dev.size // 2
            if getattr(self, '_idx_all', None) is None or self._idx_all.size < n_all:
                self._idx_all = self.device.array(np.arange(n_all, dtype=np.int32))
            return dev, self._idx_all.view(int(idx[0]), (len(idx),))
        if getattr(self, '_idx_dev', None) is None or self._idx_dev.size < len(idx):
            self._idx_dev = DeviceArray(self.device, (max(len(idx), 64),), np.int32)
        view = self._idx_dev.view(0, (len(idx),))
        self.device.uploader().upload(view, idx)     # asynchronous (pinned ring): a blocking copy here drained the stream every minibatch
        return dev, view

    def _coords(self, this_i_theta):
        cv = self.common_vars
        if cv.get('two_d_mode') or self.rotate_out_of_loop:
            return None
        return cv['rotation_tables'](int(this_i_theta))

    # ------------------------------------------------------------------ rotate_out_of_loop (adorym/ptychography.py:917-947, 1063-1078)
    def rotate_outside(self, obj, this_i_theta):
        """obj.rotate_array(coords(theta), apply_to_arr_rot=False) of the reference: the WHOLE object is rotated to the angle
        outside the differentiated block.  Fills the engine's slice-major rotated buffer (what the multislice kernel reads,
        with its transmission cache) and ``arr_rot``, the same voxels in the object's own layout [Y,X,Z,2] (what the
        regularisers see and what the driver passes as ``obj``, like the reference's obj.arr_rot)."""
        eng = self.engine
        eng.rotate(obj, self.common_vars['rotation_tables'](int(this_i_theta)), None)
        if getattr(self, 'arr_rot', None) is None or self.arr_rot.shape != obj.shape:
            self.arr_rot = self.device.empty(obj.shape)
        self.arr_rot.zero_()
        check(self.device.lib.adm_rotate_adj(eng.plan.handle, eng.obj_rot.ptr, None, self.arr_rot.ptr, 0, eng.obj_size[0]))
        return self.arr_rot

    def resample_gradient(self, grad, this_i_theta):
        """gradient.rotate_array(coords(-theta), overwrite_arr=True): the accumulated gradient buffer, which is in the rotated
        frame, is resampled with the lookup table of -theta -- a bilinear interpolation like the forward rotation, not its
        transpose -- and overwritten.  Through a cache-less twin of the plan so that the slice-transmission cache of the
        rotated object stays valid; the engine's rotated-gradient buffer is free at this point and serves as scratch."""
        eng = self.engine
        key = int(this_i_theta)
        inv = self.__dict__.setdefault('_inv_tables', {})
        if key not in inv:
            inv[key] = RotationTable(self.device, eng.obj_size, -self.common_vars['theta_ls'][key])
        aux = eng.cacheless_plan()
        lib = self.device.lib
        check(lib.adm_rotate_fwd(aux.handle, grad.ptr, inv[key].ptr, eng.grad_rot.ptr, 0, eng.obj_size[0]))
        grad.zero_()
        check(lib.adm_rotate_adj(aux.handle, eng.grad_rot.ptr, None, grad.ptr, 0, eng.obj_size[0]))

    def _probe(self, probe_real, probe_imag):
        """probe_real/imag: host arrays [n_modes,Py,Px] or a DeviceArray [n_modes,Py,Px,2] passed as probe_real."""
        if isinstance(probe_real, DeviceArray):
            return probe_real
        pr = np.asarray(probe_real, dtype=np.float32)
        pi = np.asarray(probe_imag, dtype=np.float32)
        host = np.ascontiguousarray(np.stack([pr, pi], -1))
        if self._probe_dev is None or self._probe_dev.shape != host.shape:
            self._probe_dev = self.device.empty(host.shape)
        self._probe_dev.set(host)
        return self._probe_dev

    def _small_grad(self, name, shape, refit=False, owner=None):
        """The small gradient array kept as attribute ``name`` of this model (of ``owner``, if given): allocated on first use, and
        again when ``refit`` is set and the shape differs.  Not initialised: the caller zero-fills it where its kernel accumulates."""
        owner = self if owner is None else owner
        arr = getattr(owner, name, None)
        if arr is None or (refit and arr.shape != shape):
            arr = self.device.empty(shape)
            setattr(owner, name, arr)
        return arr

    def _ordered_grads(self, opt_args_ls, table, prefix=''):
        """The gradients ordered like ``opt_args_ls`` out of ``table``, {argument name: array}; an argument it does not hold is refused by name."""
        names = [self.argument_ls[i] for i in opt_args_ls]
        for name in names:
            if name not in table:
                raise NotImplementedError("%sgradient w.r.t. '%s' is outside the accelerated path" % (prefix, name))
        return tuple(table[name] for name in names)

    def _run(self, obj, probe_real, probe_imag, this_i_theta, this_pos_batch, target, want_grad, grad_obj=None,
             want_probe_grad=False, want_pred=False, probe_pos_correction=None, this_ind_batch=None, want_shift_grad=False,
             side_hook=None, regularize=True, init_grad=False, want_slice_pos_grad=False, prj_pos_offset=None, want_offset_grad=False,
             more_grads=None):
        """One evaluation.  Stream plan (same as bench.py): rotation on the main stream; then, on the context's side
        stream, ``side_hook()`` (the driver zeroes the gradient buffer / finishes the previous update there) and the
        regulariser gradient -- they only need the object -- while the multislice chain, which occupies `minibatch` of
        the 256 CUs, runs on the main stream; joined before the back-rotation adds into ``grad_obj``.  ``more_grads``: further
        small gradients of a subclass's engine, {keyword of MultisliceEngine.multislice: array}, zero-filled here with the others."""
        eng = self.engine
        ctx = self.device
        probe = self._probe(probe_real, probe_imag)
        coords = self._coords(this_i_theta)
        eng.set_batch(this_pos_batch, target)
        yr = eng.y_footprint(this_pos_batch)
        rool = bool(self.rotate_out_of_loop) and not self.common_vars.get('two_d_mode')
        if not (rool and obj is getattr(self, 'arr_rot', None)):
            # (rotate_out_of_loop: ``obj`` IS the rotated object; the driver hands over arr_rot, whose slice-major twin the
            # engine already holds from rotate_outside(); any other array is loaded as it is, coords = None)
            eng.rotate(obj, coords, yr)
        ctx.fork()
        eng.flush_loss_copy()       # the previous minibatch's loss read-back: on the side stream, beside this kernel
        self._flush_reg_copy()      # ... and its regulariser value (before the kernel below overwrites it)
        if side_hook is not None:
            side_hook()
        # init_grad: grad_obj is uninitialised -- the regulariser kernel writes it (one pass) or it is zero-filled
        rx = getattr(self, 'restricted_planes', None) if want_grad else None
        if rx is not None and not init_grad:
            # the restricted exchange defers the regulariser gradient to the shard owners (R-fold, after the reduction): an
            # evaluation that ACCUMULATES into a buffer initialised elsewhere would add it here as well and count it twice
            raise RuntimeError('restricted_planes is set but the gradient buffer is not initialised by this evaluation '
                               '(init_grad=False): the regulariser term would be counted twice')
        if rx is not None:
            # footprint-restricted exchange (DataParallelObject.exchange_and_update(touched=...)): the gradient buffer carries
            # the DATA term only, on the planes the global batch touches -- zero those; the regulariser's gradient is added by
            # the shard owners after the reduction, only its VALUE (for the loss log) is evaluated here
            plane = int(np.prod(eng.obj_size[1:])) * 2 * 4
            check(ctx.lib.adm_memset(ctx.handle, grad_obj.ptr + rx[0] * plane, 0, (rx[1] - rx[0]) * plane))
            self._reg_pending = self._regularize_launch(obj, None, False, value_only=True) if regularize else False
        else:
            self._reg_pending = self._regularize_launch(obj, grad_obj if want_grad else None, init_grad and want_grad) if regularize else False
            if init_grad and want_grad and not regularize:
                grad_obj.zero_()
        if want_grad and isinstance(coords, RotationTable):
            # first minibatch of an angle: its rotation-adjoint tables are built here, on the side stream beside the
            # multislice kernel (0.4 ms of emit + sort), not on the main stream when the back-rotation asks for them
            coords.csr(eng.plan)
        nxt = self.__dict__.pop('prefetch_table', None)
        if want_grad and isinstance(nxt, RotationTable):
            # ... and the NEXT angle's (the driver hands its table over during the current angle's last minibatch): built here, beside
            # this kernel, instead of in front of the next angle's first launch with the GPU idle behind the host
            nxt.csr(eng.plan)
        B = len(np.asarray(this_pos_batch).reshape(-1, 2))
        early_cover = want_grad and B <= eng.N_CU
        if early_cover:
            eng.build_cover()       # the overlap-add's cover lists only need the positions: built beside the kernel
        nb = self.__dict__.pop('next_batch', None)
        if nb is not None and want_grad:
            # the NEXT evaluation's measured data (the driver says which): host -> device now, beside this kernel
            t_next = self._target(nb[0], nb[1])
            if isinstance(t_next, np.ndarray):
                self._staged = ((int(nb[0]), np.asarray(nb[1]).tobytes()), eng.stage_target(t_next))
        ctx.end_fork()
        gp = self._small_grad('_grad_probe_dev', probe.shape, refit=True).zero_() if want_probe_grad else None
        shifts, idx = self._shift_args(probe_pos_correction, this_i_theta, this_ind_batch)
        if want_shift_grad and shifts is None:
            raise RuntimeError('gradient w.r.t. probe_pos_correction requested but no corrections were passed')
        gsh = self._small_grad('_grad_shift_dev', shifts.shape, refit=True).zero_() if want_shift_grad else None
        # (SparseMultisliceModel: dL/d slice_pos_cm_ls, left in self._grad_slice_pos_dev)
        gz = self._small_grad('_grad_slice_pos_dev', eng.slice_pos.shape).zero_() if want_slice_pos_grad else None
        more_grads = more_grads or {}
        for g in more_grads.values():
            g.zero_()
        offs, oidx = self._offset_args(prj_pos_offset, this_i_theta, B)
        if want_offset_grad and offs is None:
            raise RuntimeError('gradient w.r.t. prj_pos_offset requested but optimize_prj_pos_offset is not set')
        # (dL/d prj_pos_offset, dense [n_theta, 2], left in self._grad_offset_dev)
        goff = self._small_grad('_grad_offset_dev', offs.shape, refit=True).zero_() if want_offset_grad else None
        mb = B // self.batch_group
        # each reference minibatch is a mean over ITS positions (their detector planes, with a fan-out) and the kept detector pixels
        gs = 2.0 / (mb * eng.det_per_pos * eng.n_det)
        if want_grad and shifts is None and B > eng.N_CU and gz is None and offs is None and not more_grads:
            # no join here: the overlapped launch forks again, and the side stream is in order, so its overlap-adds queue
            # behind the regulariser kernel while the first round of workgroups already runs beside it
            eng.multislice_overlapped(probe, grad_probe=gp, grad_scale=gs, want_pred=want_pred)
        else:
            eng.multislice(probe, grad_probe=gp, want_grad=want_grad, want_pred=want_pred, grad_scale=gs, shifts=shifts,
                           shift_index=idx, grad_shifts=gsh, accumulate=False, grad_slice_pos=gz, exit_shifts=offs,
                           exit_shift_index=oidx, grad_exit_shifts=goff, **more_grads)
            ctx.join()              # (the side stream's work is a fraction of the kernel's time: the join does not wait)
            if want_grad:
                eng.accumulate_tiles()
        self._last_mb = mb
        if want_grad:
            eng.rotate_adjoint(grad_obj, coords, yr)
        return gp, gsh

    def _regularize_launch(self, obj, grad_obj, init_grad=False, value_only=False):
        """Queue the regulariser kernels (value into a device scalar, gradient added to grad_obj if given) on the
        current stream.  ``init_grad``: grad_obj holds garbage and is initialised here (regulariser kernel in 'set' mode,
        or a zero fill).  ``value_only``: no gradient at all (plain L1 / TV).  Returns True if a value is pending."""
        from .regularizers import ReweightedL1Regularizer
        self._flush_reg_copy()      # the previous value leaves before this launch overwrites it
        ad, ab, gm = combined_weights(self.reg_list)
        rw = [r for r in self.reg_list if isinstance(r, ReweightedL1Regularizer)]
        plain = ad != 0 or ab != 0 or gm != 0
        if init_grad and not plain:
            grad_obj.zero_()
        if not plain and not rw:
            return False
        if self._reg_val is None:
            self._reg_val = self.device.zeros((1,))
        self._reg_val.zero_()
        if value_only:
            if rw:
                raise NotImplementedError('value-only regulariser evaluation with a reweighted L1 term')
            k = float(self.batch_group)
            check(self.device.lib.adm_reg_grad(self.engine.plan.handle, obj.ptr, ad * k, ab * k, gm * k, None, self._reg_val.ptr))
            return True
        if grad_obj is None:
            if getattr(self, '_scratch_grad', None) is None or self._scratch_grad.size != obj.size:
                self._scratch_grad = self.device.empty((obj.size,))
            grad_obj = self._scratch_grad
        k = float(self.batch_group)     # every fused minibatch adds the regulariser once (forward_model.py:138-139)
        if plain:
            fn = self.device.lib.adm_reg_grad_set if init_grad else self.device.lib.adm_reg_grad
            check(fn(self.engine.plan.handle, obj.ptr, ad * k, ab * k, gm * k, grad_obj.ptr, self._reg_val.ptr))
        for r in rw:
            if r.weight_l1 is None:
                raise RuntimeError('ReweightedL1Regularizer: update_l1_weight() has not been called')
            check(self.device.lib.adm_reg_grad_weighted(self.engine.plan.handle, obj.ptr, r.weight_l1.ptr, float(r.alpha_d or 0.) * k,
                                                        float(r.alpha_b or 0.) * k, grad_obj.ptr, self._reg_val.ptr))
        return True

    def _reg_value_async(self, pending):
        """Register the read-back of the regulariser value; returns a callable giving the float.  Like the data term's sums
        (MultisliceEngine.loss_async) the 4-byte copy itself is DEFERRED: it is queued by the next evaluation inside its
        side-stream region, before the regulariser kernel that overwrites the value -- on the main stream it sat between the
        back-rotation and the optimiser kernel with its dependency gap (~12 us per minibatch) -- or by the callable, whichever
        comes first."""
        if not pending:
            return lambda: 0.0
        from .device import PinnedArray, Event
        if getattr(self, '_reg_pinned', None) is None:
            self._reg_pinned = [PinnedArray(self.device, (1,)) for _ in range(2)]
            self._reg_events = [Event(self.device) for _ in range(2)]
            self._reg_slot = 0
        self._flush_reg_copy()
        self._reg_slot ^= 1
        k = self._reg_slot
        self._reg_deferred = k
        g = float(self.batch_group)

        def value():
            if getattr(self, '_reg_deferred', None) == k:
                self._flush_reg_copy()
            self._reg_events[k].synchronize()
            return float(self._reg_pinned[k].array[0]) / g
        return value

    def _flush_reg_copy(self):
        """Queue the deferred regulariser-value read-back, if any, on the stream the context is enqueuing on right now."""
        k = getattr(self, '_reg_deferred', None)
        if k is not None:
            self._reg_deferred = None
            self._reg_pinned[k].copy_from_async(self._reg_val, 4)
            self._reg_events[k].record()

    def _regularize(self, obj, grad_obj):
        """Adds the regulariser gradient to grad_obj (if given) and returns the regulariser value (blocking)."""
        return self._reg_value_async(self._regularize_launch(obj, grad_obj))()

    def _queue_loss(self, data_loss_fn=None):
        """current_loss <- data term + regulariser, both read back lazily."""
        tok = self.engine.loss_async(last=self._last_mb) if data_loss_fn is None else None
        regv = self._reg_value_async(getattr(self, '_reg_pending', False))
        eng = self.engine
        self._loss_thunk = (lambda: eng.loss_result(tok) + regv()) if data_loss_fn is None else (lambda: data_loss_fn() + regv())

    def _resident_enabled(self):
        if getattr(self, '_resident', None) is None:
            shp = getattr(self.prj, 'shape', None)
            limit = float(os.environ.get('ADM_RESIDENT_DATA_MB', '1024')) * 2 ** 20
            self._resident = {} if (shp is not None and len(shp) == 4 and 4.0 * np.prod(shp) <= limit) else False
        return self._resident is not False

    def prefetch_data(self, i_theta):
        """Resident datasets only: the processed data of angle ``i_theta`` on the device, uploaded ASYNCHRONOUSLY through a pinned
        staging ring the first time the angle is asked for (a blocking copy here drains the stream: 1.3 ms of idle GPU at every
        first-touch angle).  The driver asks one minibatch before the angle begins, so the host-side preparation (|prj|, a copy
        into pinned memory: ~2 ms for 529 x 72 x 72 values) overlaps the current angle's last launch.  Returns the DeviceArray,
        or None when the dataset is streamed."""
        if not self._resident_enabled():
            return None
        td = self.common_vars.get('theta_downsample') or 1
        key = int(i_theta) * td
        dev = self._resident.get(key)
        if dev is None:
            host = self.get_data(i_theta, np.arange(self.prj.shape[1]), theta_downsample=td, ds_level=self.common_vars.get('ds_level', 1))
            up = getattr(self.device, 'array_async', None) or self.device.array
            dev = up(np.ascontiguousarray(host, dtype=np.float32))
            self._resident[key] = dev
        return dev

    def _target(self, this_i_theta, this_ind_batch):
        """The minibatch's measured data as the loss wants it (get_data).  Small datasets -- 2-D ptychography above all, where every
        epoch revisits the same angle -- are kept RESIDENT on the device, one processed [n_pos, Py, Px] array per angle uploaded the
        first time the angle is met; a minibatch that is a run of consecutive positions (the reference sorts a minibatch's indices,
        adorym/ptychography.py:907) is then a view of it: no host work, no copy.  Larger datasets (config 3: 5.5 GB) keep streaming
        their minibatches through the pinned ring, where the host work hides behind a 2 ms GPU step.  ADM_RESIDENT_DATA_MB (1024)."""
        td = self.common_vars.get('theta_downsample') or 1
        ind = np.asarray(this_ind_batch)
        if self._resident_enabled() and len(ind) > 0 and int(ind[-1]) - int(ind[0]) == len(ind) - 1 and np.all(np.diff(ind) == 1):
            key = int(this_i_theta) * td
            dev = self._resident.get(key)
            if dev is None:
                dev = self.prefetch_data(this_i_theta)
            n_px = dev.shape[1] * dev.shape[2]
            return dev.view(int(ind[0]) * n_px, (len(ind), dev.shape[1], dev.shape[2]))
        return self.get_data(this_i_theta, this_ind_batch, theta_downsample=td, ds_level=self.common_vars.get('ds_level', 1))

    # ------------------------------------------------------------------ reference interface
    def predict(self, obj, probe_real, probe_imag, probe_defocus_mm, probe_pos_offset, this_i_theta, this_pos_batch, prj,
                probe_pos_correction, this_ind_batch, tilt_ls, prj_pos_offset):
        """Predicted detector magnitudes [minibatch, Py, Px] (host float32), adorym/forward_model.py:179-387."""
        self._check_static(probe_defocus_mm, probe_pos_offset, probe_pos_correction, prj_pos_offset)
        B = len(this_pos_batch)
        zeros = np.zeros((B,) + tuple(self.engine.probe_size), np.float32)
        self._run(obj, probe_real, probe_imag, this_i_theta, this_pos_batch, zeros, want_grad=False, want_pred=True,
                  probe_pos_correction=probe_pos_correction, this_ind_batch=this_ind_batch, regularize=False, prj_pos_offset=prj_pos_offset)
        self.i_call += 1
        return self.engine.pred()

    def get_loss_function(self):
        def calculate_loss(obj, probe_real, probe_imag, probe_defocus_mm, probe_pos_offset, this_i_theta, this_pos_batch, prj,
                           probe_pos_correction, this_ind_batch, tilt_ls, prj_pos_offset):
            self._check_static(probe_defocus_mm, probe_pos_offset, probe_pos_correction, prj_pos_offset)
            target = self._target(this_i_theta, this_ind_batch)
            self._run(obj, probe_real, probe_imag, this_i_theta, this_pos_batch, target, want_grad=False,
                      probe_pos_correction=probe_pos_correction, this_ind_batch=this_ind_batch, prj_pos_offset=prj_pos_offset)
            self._queue_loss()
            return self.current_loss
        calculate_loss.forward_model = self
        return calculate_loss

    def loss_and_gradients(self, opt_args_ls, grad_obj, obj, probe_real, probe_imag, probe_defocus_mm, probe_pos_offset,
                           this_i_theta, this_pos_batch, prj, probe_pos_correction, this_ind_batch, tilt_ls, prj_pos_offset,
                           _side_hook=None, _init_grad=False):
        """
        The hand-derived replacement of ``torch.autograd.grad(loss, [args in opt_args_ls])``
        (adorym/wrappers.py:300-331): accumulates d loss/d obj into ``grad_obj`` (DeviceArray) and returns
        the gradients ordered like opt_args_ls: index 0 -> grad_obj, probe_real/probe_imag indices -> host arrays.
        """
        self._check_static(probe_defocus_mm, probe_pos_offset, probe_pos_correction, prj_pos_offset)
        staged = self.__dict__.pop('_staged', None)
        if staged is not None and staged[0] == (int(this_i_theta), np.asarray(this_ind_batch).tobytes()):
            target = staged[1]          # uploaded during the previous evaluation (PtychographyModel._run, next_batch)
        else:
            target = self._target(this_i_theta, this_ind_batch)
        wanted = set(self.argument_ls[i] for i in opt_args_ls).intersection(self.GRADIENTS)
        gp, gsh = self._run(obj, probe_real, probe_imag, this_i_theta, this_pos_batch, target, want_grad=True, grad_obj=grad_obj,
                            want_probe_grad='probe_real' in wanted or 'probe_imag' in wanted, probe_pos_correction=probe_pos_correction,
                            this_ind_batch=this_ind_batch, want_shift_grad='probe_pos_correction' in wanted, side_hook=_side_hook,
                            init_grad=_init_grad, prj_pos_offset=prj_pos_offset, want_offset_grad='prj_pos_offset' in wanted,
                            want_slice_pos_grad='slice_pos_cm_ls' in wanted)
        self._queue_loss()          # self.current_loss fetches it on first access
        # probe_real and probe_imag reference ONE interleaved device array [n_modes,Py,Px,2] (real, imag): no host round trip;
        # probe_pos_correction: DeviceArray, dense like the parameter (zero outside this minibatch); prj_pos_offset: DeviceArray
        # [n_theta, 2], zero outside this angle; slice_pos_cm_ls (SparseMultisliceModel): DeviceArray float32 [S], dL/dz in 1/cm
        table = dict(obj=grad_obj, probe_real=gp, probe_imag=gp, probe_pos_correction=gsh, prj_pos_offset=getattr(self, '_grad_offset_dev', None),
                     slice_pos_cm_ls=getattr(self, '_grad_slice_pos_dev', None))
        return self._ordered_grads(opt_args_ls, {name: table[name] for name in self.GRADIENTS})


SingleBatchFullfieldModel = PtychographyModel
SingleBatchPtychographyModel = PtychographyModel


class SparseMultisliceModel(PtychographyModel):
    """
    adorym/forward_model.py:589-806: a few thin slices at arbitrary depths ``slice_pos_cm_ls`` (cm), every gap propagated with
    its own Fresnel-approximation kernel (sparse_multislice_propagate_batch, adorym/propagate.py:479-534).  The argument list is
    PtychographyModel's with ``slice_pos_cm_ls`` where that has ``tilt_ls``; everything else -- rotation, resident data, staged
    targets, regularisers, probe gradient -- is PtychographyModel's machinery.  ``common_vars_dict['engine']`` is a
    MultisliceEngine built with ``slice_pos_cm`` (a streamed engine); its ``slice_pos`` device array IS the parameter: a
    DeviceArray handed in must be that array (the driver's optimiser updates it in place and tells the engine), host values are
    uploaded into it when they differ from the ones last seen.  Sub-pixel probe positions are refused (the streamed path takes one
    probe set for all positions).
    """

    def __init__(self, loss_function_type='lsq', distribution_mode=None, device=None, common_vars_dict=None,
                 raw_data_type='magnitude', simulation_mode=False, run_bfloat16=False, run_float64=False):
        super(SparseMultisliceModel, self).__init__(loss_function_type, distribution_mode, device, common_vars_dict, raw_data_type,
                                                    simulation_mode=simulation_mode, run_bfloat16=run_bfloat16, run_float64=run_float64)
        if self.engine is not None and getattr(self.engine, 'slice_pos', None) is None:
            raise ValueError('SparseMultisliceModel needs an engine built with slice_pos_cm (the slice positions in cm)')
        self._slice_pos_host = None

    REFUSED_FLAGS = PtychographyModel.REFUSED_FLAGS + ('optimize_prj_pos_offset',)      # (no exit-wave shifts on a sparse plan)
    GRADIENTS = ('obj', 'probe_real', 'probe_imag', 'slice_pos_cm_ls')
    PROJECTION_MODEL = 'sparse multislice (SparseMultisliceModel)'

    def _set_slice_pos(self, slice_pos_cm_ls):
        eng = self.engine
        if isinstance(slice_pos_cm_ls, DeviceArray):
            if slice_pos_cm_ls.ptr != eng.slice_pos.ptr:
                raise ValueError('slice_pos_cm_ls on the device must be the engine\'s own slice_pos array')
            return
        host = np.ascontiguousarray(np.asarray(slice_pos_cm_ls, dtype=np.float32).reshape(-1))
        if host.size != eng.slice_pos.size:
            raise ValueError('slice_pos_cm_ls: %d slice positions for an object of %d slices' % (host.size, eng.slice_pos.size))
        if self._slice_pos_host is None or not np.array_equal(self._slice_pos_host, host):
            eng.slice_pos.set(host)
            eng.slice_pos_changed()
            self._slice_pos_host = host

    def predict(self, obj, probe_real, probe_imag, probe_defocus_mm, probe_pos_offset, this_i_theta, this_pos_batch, prj,
                probe_pos_correction, this_ind_batch, slice_pos_cm_ls, prj_pos_offset):
        """Predicted detector magnitudes [minibatch, Py, Px] (host float32), adorym/forward_model.py:602-792."""
        self._set_slice_pos(slice_pos_cm_ls)
        return super(SparseMultisliceModel, self).predict(obj, probe_real, probe_imag, probe_defocus_mm, probe_pos_offset, this_i_theta,
                                                          this_pos_batch, prj, probe_pos_correction, this_ind_batch, None, prj_pos_offset)

    def get_loss_function(self):
        dense = super(SparseMultisliceModel, self).get_loss_function()

        def calculate_loss(obj, probe_real, probe_imag, probe_defocus_mm, probe_pos_offset, this_i_theta, this_pos_batch, prj,
                           probe_pos_correction, this_ind_batch, slice_pos_cm_ls, prj_pos_offset):
            self._set_slice_pos(slice_pos_cm_ls)
            return dense(obj, probe_real, probe_imag, probe_defocus_mm, probe_pos_offset, this_i_theta, this_pos_batch, prj,
                         probe_pos_correction, this_ind_batch, None, prj_pos_offset)
        calculate_loss.forward_model = self
        return calculate_loss

    def loss_and_gradients(self, opt_args_ls, grad_obj, obj, probe_real, probe_imag, probe_defocus_mm, probe_pos_offset,
                           this_i_theta, this_pos_batch, prj, probe_pos_correction, this_ind_batch, slice_pos_cm_ls, prj_pos_offset,
                           _side_hook=None, _init_grad=False):
        """PtychographyModel.loss_and_gradients with ``slice_pos_cm_ls`` served (GRADIENTS): its gradient is a DeviceArray float32
        [S], dL/dz in 1/cm."""
        self._set_slice_pos(slice_pos_cm_ls)
        return super(SparseMultisliceModel, self).loss_and_gradients(
            opt_args_ls, grad_obj, obj, probe_real, probe_imag, probe_defocus_mm, probe_pos_offset, this_i_theta, this_pos_batch, prj,
            probe_pos_correction, this_ind_batch, None, prj_pos_offset, _side_hook=_side_hook, _init_grad=_init_grad)


# multi-distance holography has a module of its own; its model is still importable from here (behind the classes it builds on)
from .multidist_model import MultiDistModel     # noqa: E402
