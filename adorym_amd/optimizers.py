"""
Optimisers with the reference's plugin contract (adorym/optimizers.py:32-126, 242-252, 275-337, 432-464):

    opt = AdamOptimizer(name, output_folder, distribution_mode, options_dict)
    opt.create_container(whole_object_size, use_checkpoint, device_obj)
    x = opt.apply_gradient(x, gradient, i_batch, **opt.options_dict)

``x`` / ``gradient`` are DeviceArrays (flat views are fine); the update runs in the fused HIP kernel
adm_adam_step / adm_gd_step in place and returns ``x``.  The moment arrays live in
``params_whole_array_dict`` like the reference's.
"""
import numpy as np

from ._lib import check
from .device import DeviceArray
from .array_ops import Gradient
from .linesearch import BackTrackingLineSearch, AdaptiveLineSearch


class Optimizer(object):
    """adorym/optimizers.py:32-126 (distribution_mode=None subset)."""

    def __init__(self, name, output_folder='.', params_list=(), distribution_mode=None, options_dict=None, forward_model=None):
        if distribution_mode is not None:
            raise NotImplementedError("distribution_mode '%s' is outside the accelerated path (DP only)" % distribution_mode)
        self.name = name
        self.forward_model = forward_model
        self.output_folder = output_folder
        self.params_list = params_list
        self.params_whole_array_dict = {}
        self.i_batch = 0
        self.index_in_grad_returns = None
        self.distribution_mode = distribution_mode
        self.options_dict = options_dict if options_dict is not None else {}
        self.grads = None
        self.whole_object_size = None
        self.ctx = None

    def __str__(self):
        s = self.__class__.__name__ + '; '
        for k in self.options_dict.keys():
            s = s + k + ': ' + str(self.options_dict[k]) + '; '
        return s

    def create_container(self, whole_object_size, use_checkpoint=False, device_obj=None, use_numpy=False, dtype='float32'):
        """``device_obj`` is an adorym_amd.Context."""
        self.whole_object_size = whole_object_size
        self.ctx = device_obj
        self.create_param_arrays(whole_object_size, device=device_obj)

    def create_param_arrays(self, whole_object_size, device=None, use_numpy=False):
        self.whole_object_size = whole_object_size
        for param_name in self.params_list:
            self.params_whole_array_dict[param_name] = device.zeros(tuple(whole_object_size))

    def set_index_in_grad_return(self, ind):
        self.index_in_grad_returns = ind

    def convert_gradient(self, gradient):
        return gradient.arr if isinstance(gradient, Gradient) else gradient


class AdamOptimizer(Optimizer):
    """adorym/optimizers.py:265-337: m/v moments, bias correction with (i_batch+1), eps=1e-7."""

    def __init__(self, name, output_folder='.', distribution_mode=None, options_dict=None, forward_model=None):
        super(AdamOptimizer, self).__init__(name, output_folder=output_folder, params_list=['m', 'v'],
                                            distribution_mode=distribution_mode, options_dict=options_dict,
                                            forward_model=forward_model)

    def apply_gradient(self, x, gradient, i_batch, step_size=0.001, b1=0.9, b2=0.999, eps=1e-7, flags=0, mask=None,
                       update_batch_count=True, **kwargs):
        g = self.convert_gradient(gradient)
        m, v = self.params_whole_array_dict['m'], self.params_whole_array_dict['v']
        ctx = x.ctx
        check(ctx.lib.adm_adam_step(ctx.handle, x.ptr, g.ptr, m.ptr, v.ptr, 0, x.size, int(i_batch), float(step_size),
                                    float(b1), float(b2), float(eps), int(flags), mask.ptr if mask is not None else None))
        if update_batch_count:
            self.i_batch += 1
        return x


class GDOptimizer(Optimizer):
    """adorym/optimizers.py:432-464 (step halving schedule :452-460)."""

    def __init__(self, name, output_folder='.', distribution_mode=None, options_dict=None, forward_model=None):
        super(GDOptimizer, self).__init__(name, output_folder=output_folder, params_list=[], distribution_mode=distribution_mode,
                                          options_dict=options_dict, forward_model=forward_model)

    @staticmethod
    def scheduled_step(i_batch, step_size, dynamic_rate=True, first_downrate_iteration=92):
        if dynamic_rate:
            threshold_iteration = first_downrate_iteration
            i = 1
            while threshold_iteration < i_batch:
                threshold_iteration += first_downrate_iteration * 2 ** i
                i += 1
                step_size /= 2.
        return step_size

    def apply_gradient(self, x, gradient, i_batch, step_size=0.001, dynamic_rate=True, first_downrate_iteration=92, flags=0,
                       mask=None, **kwargs):
        g = self.convert_gradient(gradient)
        step = self.scheduled_step(i_batch, step_size, dynamic_rate, first_downrate_iteration)
        ctx = x.ctx
        check(ctx.lib.adm_gd_step(ctx.handle, x.ptr, g.ptr, 0, x.size, float(step), int(flags),
                                  mask.ptr if mask is not None else None))
        return x


class MomentumOptimizer(Optimizer):
    """adorym/optimizers.py:366-411: v = gamma*v + step*g; x = x - v."""

    def __init__(self, name, output_folder='.', distribution_mode=None, options_dict=None, forward_model=None):
        super(MomentumOptimizer, self).__init__(name, output_folder=output_folder, params_list=['v'],
                                                distribution_mode=distribution_mode, options_dict=options_dict,
                                                forward_model=forward_model)

    def apply_gradient(self, x, gradient, i_batch, step_size=0.001, gamma=0.9, flags=0, mask=None, **kwargs):
        g = self.convert_gradient(gradient)
        v = self.params_whole_array_dict['v']
        ctx = x.ctx
        check(ctx.lib.adm_momentum_step(ctx.handle, x.ptr, g.ptr, v.ptr, 0, x.size, float(step_size), float(gamma), int(flags),
                                        mask.ptr if mask is not None else None))
        return x


class CGOptimizer(Optimizer):
    """adorym/optimizers.py:594-704: Polak-Ribiere conjugate gradient with a backtracking line search, for the object.

    One update is: adm_cg_beta (beta stays on the device), adm_cg_direction (s, descent_dir_old and the sums the search starts
    from), one read of the page-locked sums block, adm_cg_fallback when the direction does not descend; then per trial one
    adm_cg_trial launch into a buffer of the optimiser's and one loss-only evaluation of the forward model
    (``forward_model.get_loss_function()`` on ``forward_model.loss_args`` with the trial point in the place of ``name``); then
    adm_cg_accept, which applies the constraints and the support mask to the accepted point -- or to ``x`` itself when the search
    found nothing.  A new line-search object is built in every call, as in the reference, so every search starts from
    ``step_size / |s|``.  ``beta`` is 0 when ``i_batch`` is 0 whatever the state holds; where the reference divides by a zero
    ``sum descent_dir_old^2`` and carries a NaN, beta is 0 here.  ``_diag_precondition_t`` is never set in the reference: there is
    no preconditioner.  The record of the last update (beta, the descent check, f0, df0, the norm, every trial) is ``self.last``."""

    linesearch_map = {'backtracking': BackTrackingLineSearch, 'adaptive': AdaptiveLineSearch}

    def __init__(self, name, output_folder='.', distribution_mode=None, options_dict=None, forward_model=None):
        super(CGOptimizer, self).__init__(name, output_folder=output_folder, params_list=['descent_dir_old', 's'],
                                          distribution_mode=distribution_mode, options_dict=options_dict, forward_model=forward_model)
        self.i_line_search_step = 0
        self._diag_precondition_t = None
        self._linesearch = None
        self._x_trial = self._scratch = self._sums = None
        self.last = None

    def _buffers(self, x):
        from ._lib import CG_SCRATCH_DOUBLES
        from .device import MappedArray
        ctx = x.ctx
        if self._x_trial is None or self._x_trial.size != x.size or self._x_trial.ctx is not ctx:
            self._x_trial = ctx.empty((x.size,))
            self._scratch = ctx.empty((CG_SCRATCH_DOUBLES,), np.float64)
            self._sums = MappedArray(ctx, (8,), np.float64)
        return self._x_trial, self._scratch, self._sums

    def apply_gradient(self, x, gradient, i_batch=None, step_size=1., linesearch_type='adaptive', max_backtracking_iter=None,
                       normalize_alpha=True, flags=0, mask=None, **kwargs):
        from . import _lib as L
        from .forward_model import ForwardModel
        g = self.convert_gradient(gradient)
        forward_model = getattr(gradient, 'forward_model', None)
        if forward_model is None:
            forward_model = self.forward_model
        if not isinstance(forward_model, ForwardModel):
            raise ValueError('ForwardModel must be supplied either through Gradient object or upon optimizer instantiation.')
        if self.name not in forward_model.loss_args:
            raise ValueError("CGOptimizer: '%s' is not an argument of the forward model's loss (only the object is searched)" % self.name)
        loss_kwargs = forward_model.loss_args
        loss_fn = forward_model.get_loss_function()
        f0 = float(forward_model.current_loss)
        ctx, lib, n = x.ctx, x.ctx.lib, x.size
        d_old, s = self.params_whole_array_dict['descent_dir_old'], self.params_whole_array_dict['s']
        x_trial, scratch, sums = self._buffers(x)
        self._linesearch = self.linesearch_map[linesearch_type](maxiter=max_backtracking_iter, initial_stepsize=step_size,
                                                                normalize_alpha=normalize_alpha)
        this_i_batch = int(i_batch if i_batch is not None else self.i_batch)
        check(lib.adm_cg_beta(ctx.handle, g.ptr, d_old.ptr, n, this_i_batch, scratch.ptr, sums.ptr))
        check(lib.adm_cg_direction(ctx.handle, g.ptr, s.ptr, d_old.ptr, n, scratch.ptr, sums.ptr))
        v = sums.get()                      # the one read of an update: waits for the stream
        a_sum, b_sum, beta = float(v[L.CG_SUM_A]), float(v[L.CG_SUM_B]), float(v[L.CG_SUM_BETA])
        df0, norm2 = float(v[L.CG_SUM_C]), float(v[L.CG_SUM_E])
        descends = df0 < 0
        if not descends:                    # (optimizers.py:672-674)
            check(lib.adm_cg_fallback(ctx.handle, g.ptr, s.ptr, n))
            df0, norm2 = -float(v[L.CG_SUM_D]), float(v[L.CG_SUM_D])
        view = x_trial.view(0, x.shape)

        def trial(alpha):
            check(lib.adm_cg_trial(ctx.handle, x.ptr, s.ptr, float(alpha), x_trial.ptr, n))
            return float(loss_fn(**{**loss_kwargs, self.name: view})), x_trial

        out = self._linesearch.search_values(trial, f0, df0, float(np.sqrt(norm2)), x0=x)
        check(lib.adm_cg_accept(ctx.handle, x.ptr, out.newx.ptr, 0, n, int(flags), mask.ptr if mask is not None else None))
        self.last = dict(i_batch=this_i_batch, beta_raw=(a_sum / b_sum if (this_i_batch > 0 and b_sum > 0) else 0.), beta=beta,
                         descent_check=float(v[L.CG_SUM_C]), descends=bool(descends), f0=f0, df0=df0, norm=float(np.sqrt(norm2)),
                         trials=list(self._linesearch.trials), alpha=float(out.alpha), newf=float(out.newf),
                         step_count=int(out.step_count), sums=np.array(v))
        self.i_batch += 1
        self.i_line_search_step += out.step_count
        return x


def plain_adam(opts):
    """The (b1, b2, eps) that ``opts`` share when every one of them is a plain AdamOptimizer (no option beyond step_size, b1, b2,
    eps), else None.  Under this rule alone a fused launch that updates several arrays gives the bits of their own apply_gradient."""
    if not all(type(o) is AdamOptimizer and set(o.options_dict) <= {'step_size', 'b1', 'b2', 'eps'} for o in opts):
        return None
    keys = {(float(o.options_dict.get('b1', 0.9)), float(o.options_dict.get('b2', 0.999)), float(o.options_dict.get('eps', 1e-7)))
            for o in opts}
    return next(iter(keys)) if len(keys) == 1 else None


def apply_small_params(ctx, items, i_batch):
    """The small optimisable parameters of one minibatch (adorym/optimizers.py:1022-1083: probe, probe_pos_correction,
    free_prop_cm, prj_affine_ls) in ONE launch (adm_adam_step_small) when every one of them is driven by a plain AdamOptimizer with
    the same (b1, b2, eps); otherwise one by one through the optimisers' own apply_gradient.  ``items``: dicts with
    opt, x, g (DeviceArrays), and optionally center_cols (drift guard, :1046-1048), pin (DeviceArray copied over the first
    entries of x, :1067-1073), zero_grad (the gradient accumulator is zero-filled once used), anchor (x <- x - x[0] after the
    update: the slice positions of sparse multislice, :1059; its own launch in both branches).  Same arithmetic either way."""
    from ._lib import SmallParam, SMALL_PARAMS_MAX
    if not items:
        return
    betas = plain_adam([it['opt'] for it in items])
    if betas is not None and len(items) <= SMALL_PARAMS_MAX:
        # the descriptor array is the same minibatch after minibatch (same buffers, same step sizes): build it once per combination
        sig = tuple((it['x'].ptr, it['g'].ptr, it['opt'].params_whole_array_dict['m'].ptr, it['opt'].params_whole_array_dict['v'].ptr,
                     it['x'].size, float(it['opt'].options_dict.get('step_size', 0.001)), int(it.get('center_cols', 0)),
                     bool(it.get('zero_grad')), it['pin'].ptr if it.get('pin') is not None else 0) for it in items)
        cache = ctx.__dict__.setdefault('_small_param_descs', {})
        arr = cache.get(sig)
        if arr is None:
            if len(cache) > 64:
                cache.clear()
            arr = (SmallParam * len(items))()
            for k, it in enumerate(items):
                o = it['opt']
                pin = it.get('pin')
                arr[k] = SmallParam(x=it['x'].ptr, g=it['g'].ptr, m=o.params_whole_array_dict['m'].ptr, v=o.params_whole_array_dict['v'].ptr,
                                    n=it['x'].size, step_size=float(o.options_dict.get('step_size', 0.001)),
                                    center_cols=int(it.get('center_cols', 0)), zero_grad=1 if it.get('zero_grad') else 0,
                                    pin=pin.ptr if pin is not None else None, pin_n=pin.size if pin is not None else 0)
            cache[sig] = arr
        for it in items:
            it['opt'].i_batch += 1
        b1, b2, eps = betas
        check(ctx.lib.adm_adam_step_small(ctx.handle, arr, len(items), int(i_batch), b1, b2, eps))
        for it in items:
            if it.get('anchor'):
                check(ctx.lib.adm_slice_positions_anchor(ctx.handle, it['x'].ptr, it['x'].size))
        return
    for it in items:
        it['opt'].apply_gradient(it['x'], it['g'], i_batch, **it['opt'].options_dict)
        if it.get('center_cols'):
            check(ctx.lib.adm_center_rows(ctx.handle, it['x'].ptr, it['x'].size // it['center_cols'], it['center_cols']))
        if it.get('pin') is not None:
            check(ctx.lib.adm_d2d(ctx.handle, it['x'].ptr, it['pin'].ptr, it['pin'].nbytes))
        if it.get('anchor'):
            check(ctx.lib.adm_slice_positions_anchor(ctx.handle, it['x'].ptr, it['x'].size))
        if it.get('zero_grad'):
            it['g'].zero_()


def _unsupported(name):
    class _U(Optimizer):
        def __init__(self, *a, **k):
            raise NotImplementedError('%s is outside the accelerated path (SURVEY section 2, component 5)' % name)
    _U.__name__ = name
    return _U


CurveballOptimizer = _unsupported('CurveballOptimizer')
ScipyOptimizer = _unsupported('ScipyOptimizer')
