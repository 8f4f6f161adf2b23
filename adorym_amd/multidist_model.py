"""Multi-distance holography behind the reference's plugin interface (adorym/forward_model.py:809-1092): MultiDistModel, the one public
class, and the four forward paths it chooses from -- small classes that hold their engine, their helpers and their device caches."""
import os
import numpy as np

from .device import DeviceArray
from .forward_model import PtychographyModel
from .util import calculate_pad_len


def _refuse(what, cv, flags, served, message):
    """Refusal by name: the first refused thing wins -- ``what``, if the caller has found something already, else the first flag
    of ``flags`` that is set and not among those the path serves."""
    for flag in flags:
        if what is None and cv.get(flag) and flag not in served:
            what = flag
    if what is not None:
        raise NotImplementedError(message % what)


KAPPA_REFUSED = "optimize_ctf_lg_kappa with forward_algorithm='fresnel' and %s is outside the accelerated path"


def _served(path, free_prop, prj_affine):
    """What a path serves of the two: the former if its engine refines the distances, the latter if the caller brought a registration."""
    return ((free_prop,) if path.refine else ()) + ((prj_affine,) if path.m.registration is not None else ())


def _check_fresnel(m, safe_zone_width, probe_pos_correction, served=None):
    """What the three Fresnel paths refuse alike.  ``served``: what a fan-out engine serves of REFUSED_3D_FLAGS; None on a path
    that takes no 3-D object at all."""
    cv = m.common_vars
    if cv.get('optimize_ctf_lg_kappa'):
        # (the reference threads kappa into multislice_propagate_batch there, forward_model.py:878, 1010: beta = kappa delta)
        if cv.get('homogeneous_object') is None:
            raise NotImplementedError("optimize_ctf_lg_kappa with forward_algorithm='fresnel' is outside the accelerated path")
        # served by the HomogeneousObject the caller brought, on the undivided 2-D field and on the fan-out path, on one rank
        what = None
        if m.tile_engine is not None or safe_zone_width not in (0, None) or int(cv.get('safe_zone_width') or 0) > 0:
            what = 'data divided into sub-tiles or safe_zone_width > 0'
        elif cv.get('unknown_type', 'delta_beta') == 'real_imag':
            what = "unknown_type='real_imag'"             # (the reference ignores kappa there without a word)
        elif cv.get('optimize_all_probe_pos'):
            what = 'optimize_all_probe_pos'
        elif int(cv.get('n_ranks') or 1) > 1:
            what = 'more than one rank'
        if what is not None:
            raise NotImplementedError(KAPPA_REFUSED % what)
    if cv.get('optimize_all_probe_pos'):
        # one (sy, sx) per distance applied to the measured holograms (forward_model.py:1075-1085)
        if cv.get('optimize_prj_affine'):
            raise NotImplementedError('optimize_all_probe_pos together with optimize_prj_affine is outside the accelerated path')
        if m.tile_engine is not None:
            raise NotImplementedError('optimize_all_probe_pos with multi-distance data divided into sub-tiles is outside the accelerated path')
        if probe_pos_correction is None:
            raise ValueError('optimize_all_probe_pos needs probe_pos_correction [n_dists, 2]')
    if cv.get('two_d_mode'):
        return
    what = None
    if m.tile_engine is not None or safe_zone_width not in (0, None) or int(cv.get('safe_zone_width') or 0) > 0:
        what = 'data divided into sub-tiles or safe_zone_width > 0'
    elif cv.get('unknown_type', 'delta_beta') == 'real_imag':
        what = "unknown_type='real_imag'"
    _refuse(what, cv, m.REFUSED_3D_FLAGS, served or (), 'multi-distance holography of a 3-D object with %s is outside the accelerated path')
    if served is None:
        raise ValueError('MultiDistModel with two_d_mode=False needs common_vars_dict[\'engine\'] built with detector_fanout=True '
                         '(an adorym_amd.MultisliceEngine for the sequence of distances)')


class MultiDistModel(PtychographyModel):
    """adorym/forward_model.py:809-1092: the object is illuminated by the probe and propagated to every distance of ``free_prop_cm``;
    the loss compares with the measured holograms.  The constructor picks ONE forward path from what the caller brought, in this
    order, and predict / the loss function / loss_and_gradients check and hand over to it: ``forward_algorithm == 'ctf'`` -> the
    CTF model (_CTFPath); else an ``engine`` built with detector_fanout -> a 3-D object (_FanoutPath); else a ``tile_engine`` ->
    sub-tiles with a safe zone (_TiledPath); else one undivided field of view in 2-D on ``holo_engine`` (_FieldPath)."""

    PROJECTION_MODEL = 'multi-distance data (MultiDistModel)'
    # what a 3-D object refuses by name: distances and registration are fixed, the field of view is undivided
    REFUSED_3D_FLAGS = ('optimize_free_prop', 'optimize_prj_affine', 'optimize_all_probe_pos', 'rotate_out_of_loop')
    # what the CTF model refuses by name: it has no probe, one slice and one undivided field of view; distances are fixed unless its
    # engine refines them, and holograms are taken as registered unless the caller brought a HologramRegistration
    CTF_REFUSED_FLAGS = ('optimize_probe', 'optimize_free_prop', 'optimize_prj_affine', 'optimize_all_probe_pos')

    def __init__(self, loss_function_type='lsq', distribution_mode=None, device=None, common_vars_dict=None,
                 raw_data_type='magnitude', simulation_mode=False, run_bfloat16=False, run_float64=False):
        super(MultiDistModel, self).__init__(loss_function_type, distribution_mode, device, common_vars_dict, raw_data_type,
                                             simulation_mode=simulation_mode, run_bfloat16=run_bfloat16, run_float64=run_float64)
        if loss_function_type != 'lsq':
            raise NotImplementedError('MultiDistModel: only the LSQ loss is on the accelerated path')
        cv = common_vars_dict or {}
        self.tile_engine, self.ctf = cv.get('tile_engine'), cv.get('ctf_engine')
        self._data_key, self._data_dev, self._small = None, None, {}
        is_ctf = cv.get('forward_algorithm') == 'ctf'
        fanout = not is_ctf and bool(getattr(self.engine, 'detector_fanout', False))
        # the holograms are registered by kernels of their own when the caller brought that engine; only these two paths look at it
        self.registration = cv.get('hologram_registration') if (fanout or is_ctf) else None
        self.register_3d = fanout and self.registration is not None
        # the single-material constraint of the Fresnel model (beta = kappa delta, kappa = 10^ctf_lg_kappa[0]: the OPPOSITE sense of
        # the CTF model's cos(xi) / kappa, as in the reference) wraps the object of the paths that serve it, when, and only when,
        # the caller brought the HomogeneousObject and the parameter is refined; _check_fresnel refuses it anywhere else
        self.homogeneous = cv.get('homogeneous_object') if (not is_ctf and cv.get('optimize_ctf_lg_kappa')) else None
        if is_ctf and self.ctf is None:
            raise ValueError("MultiDistModel with forward_algorithm='ctf' needs common_vars_dict['ctf_engine'] (an adorym_amd.CTFEngine)")
        self._path = (_CTFPath(self, self.ctf, cv.get('ctf_projector')) if is_ctf else _FanoutPath(self, self.engine) if fanout
                      else _TiledPath(self, self.tile_engine) if self.tile_engine is not None
                      else _FieldPath(self, cv['holo_engine'] if common_vars_dict else None))

    def _check(self, safe_zone_width, ctf_lg_kappa, probe_pos_correction):
        for flag in ('optimize_probe_defocusing', 'optimize_probe_pos_offset', 'optimize_prj_pos_offset'):
            if self.common_vars.get(flag):
                raise NotImplementedError('%s with MultiDistModel is outside the accelerated path' % flag)
        self._path.check(safe_zone_width, ctf_lg_kappa, probe_pos_correction)

    # ------------------------------------------------------------------ what more than one path uses
    def _dev(self, name, value, shape):
        """Small parameter arrays: pass DeviceArrays through, upload (and cache) host values."""
        if isinstance(value, DeviceArray):
            return value
        host = np.ascontiguousarray(np.asarray(value, dtype=np.float32).reshape(shape))
        cur = self._small.get(name)
        if cur is None or cur[0].tobytes() != host.tobytes():
            self._small[name] = (host, self.device.array(host))
        return self._small[name][1]

    def _data(self, this_i_theta):
        """All holograms of this angle, raw (the sqrt for intensity data happens after the affine registration)."""
        td = self.common_vars.get('theta_downsample') or 1
        key = int(this_i_theta) * td
        if self._data_key != key:
            t = np.ascontiguousarray(np.abs(np.asarray(self.prj[key])), dtype=np.float32)
            self._data_dev = self.device.array(t)
            self._data_key = key
        return self._data_dev

    def _tied(self, a):
        """The arguments the forward path runs on: ``a`` itself, or -- on a model that carries the single-material constraint -- a
        copy whose 'obj' is the tied object (delta, kappa delta) made in front of the launch (adm_kappa_tie; 3-D: in front of the
        rotation, which is linear), with the device copy of ctf_lg_kappa under '_lg_kappa'.  Regularisers keep seeing a['obj']."""
        h = self.homogeneous
        if h is None:
            return a
        if a['ctf_lg_kappa'] is None:
            raise ValueError("optimize_ctf_lg_kappa with forward_algorithm='fresnel' needs ctf_lg_kappa")
        lgk = self._dev('ctf_lg_kappa', a['ctf_lg_kappa'], (1,))
        return dict(a, obj=h.tie(a['obj'], lgk), _lg_kappa=lgk)

    def _fold_tied(self, a, t, grad_obj, grads, wanted, init_grad):
        """Behind a data term that left dL/d(tied object) in homogeneous.tied_grad(): the regulariser of the USER's object (its free
        beta channel included, like the reference's) and the fold (adm_kappa_fold) into ``grad_obj`` and, if wanted, into the [1]
        gradient w.r.t. ctf_lg_kappa, which joins ``grads``.  grad_obj's beta channel receives what the regulariser gives it and
        nothing from the data term.  ``init_grad``: grad_obj holds garbage -- without a regulariser the fold writes it ('set', beta =
        0: no zero fill), with one the regulariser initialises it and the fold adds.  Returns whether a regulariser value is pending."""
        h = self.homogeneous
        gk = self._small_grad('_grad_lg_kappa_dev', (1,)) if 'ctf_lg_kappa' in wanted else None
        if gk is not None:
            grads['ctf_lg_kappa'] = gk
        if init_grad and not self.reg_list:
            h.fold(a['obj'], t['_lg_kappa'], grad_obj, gk, overwrite=True)
            return False
        if gk is not None:
            gk.zero_()
        pending = self._regularize_launch(a['obj'], grad_obj, init_grad=bool(init_grad))
        h.fold(a['obj'], t['_lg_kappa'], grad_obj, gk)
        return pending

    def _check_registration(self, n_dists, field):
        """The HologramRegistration the caller brought fits the engine's distances and ``field`` (ny, nx), and the run's data."""
        reg = self.registration
        if (reg.n_dists, reg.ny, reg.nx) != (n_dists,) + tuple(field) or reg.raw_data_type != self.raw_data_type:
            raise ValueError('MultiDistModel: hologram_registration was built for another field, number of distances or raw_data_type')

    def _register(self, this_i_theta, prj_affine_ls, n_dists, want_pred, want_affine_grad):
        """forward_model.py:1066-1072 on a model that registers (see _served) with optimize_prj_affine: the raw holograms of this angle
        (cached on the device) registered by ``prj_affine_ls`` are the launch's target, made on the stream that is current here.  Returns
        (target, want_pred, finish): ``target`` None when the model does not register; ``finish`` None unless ``want_affine_grad`` -- then
        the launch keeps its predictions on the device (``want_pred`` True) and finish(them) leaves dL/d prj_affine_ls in _grad_affine_dev."""
        if self.registration is None or not self.common_vars.get('optimize_prj_affine'):
            if want_affine_grad:
                raise RuntimeError('gradient w.r.t. prj_affine_ls requested but the model registers no holograms')
            return None, want_pred, None
        raw = self._data(this_i_theta)
        aff = self._dev('prj_affine_ls', prj_affine_ls, (n_dists, 2, 3))
        target = self.registration.targets(raw, aff)
        if not want_affine_grad:
            return target, want_pred, None
        return target, True, lambda pred: self.registration.grad(raw, aff, pred, self._small_grad('_grad_affine_dev', (n_dists, 2, 3)).zero_())

    # ---- reference interface: check, then the path (``a``: the 15 arguments by name -- locals() before anything else is bound)
    def predict(self, obj, probe_real, probe_imag, probe_defocus_mm, probe_pos_offset, this_i_theta, this_pos_batch, prj,
                probe_pos_correction, this_ind_batch, free_prop_cm, safe_zone_width, prj_affine_ls, ctf_lg_kappa, prj_pos_offset):
        """Detected magnitudes [n_dists, ny, nx] (host float32), adorym/forward_model.py:819-1034."""
        a = locals()
        self._check(safe_zone_width, ctf_lg_kappa, probe_pos_correction)
        self.i_call += 1
        return self._path.predict(a)

    def get_loss_function(self):
        def calculate_loss(obj, probe_real, probe_imag, probe_defocus_mm, probe_pos_offset, this_i_theta, this_pos_batch, prj,
                           probe_pos_correction, this_ind_batch, free_prop_cm, safe_zone_width, prj_affine_ls, ctf_lg_kappa,
                           prj_pos_offset):
            a = locals()
            self._check(safe_zone_width, ctf_lg_kappa, probe_pos_correction)
            return self._path.loss(a)
        calculate_loss.forward_model = self
        return calculate_loss

    def loss_and_gradients(self, opt_args_ls, grad_obj, obj, probe_real, probe_imag, probe_defocus_mm, probe_pos_offset,
                           this_i_theta, this_pos_batch, prj, probe_pos_correction, this_ind_batch, free_prop_cm, safe_zone_width,
                           prj_affine_ls, ctf_lg_kappa, prj_pos_offset, _side_hook=None, _init_grad=False):
        """Replacement of torch.autograd.grad over MultiDistModel's loss: gradients ordered like opt_args_ls; index 0 ->
        grad_obj (accumulated in place), probe_real/probe_imag -> one interleaved DeviceArray, free_prop_cm -> DeviceArray
        [n_dists], prj_affine_ls -> DeviceArray [n_dists,2,3]."""
        a = locals()
        self._check(safe_zone_width, ctf_lg_kappa, probe_pos_correction)
        return self._path.loss_and_gradients(opt_args_ls, grad_obj, a, _side_hook, _init_grad)


class _FieldPath(object):
    """One undivided field of view in 2-D (the reference's n_blocks == 1 branch, config 5): the S = 1 object is illuminated by the
    (plane) probe and Fresnel-propagated to every distance of ``free_prop_cm`` (fresnel_propagate_wrapped); the loss compares with
    the measured holograms, optionally registered by the affine matrices ``prj_affine_ls`` (w.affine_transform).  Gradients w.r.t.
    obj, probe, free_prop_cm and prj_affine_ls come from the hand-derived adjoint in adm_holo_fwd_adj.
    ``common_vars_dict['holo_engine']`` is an adorym_amd.HolographyEngine."""
    def __init__(self, model, holo):
        self.m, self.holo, self._spec_key = model, holo, None

    def check(self, safe_zone_width, ctf_lg_kappa, probe_pos_correction):
        _check_fresnel(self.m, safe_zone_width, probe_pos_correction)
        if safe_zone_width not in (0, None):
            raise NotImplementedError('safe_zone_width > 0 needs the tile engine (the driver builds it)')

    def _spectrum(self, this_i_theta):
        """FFT2(|data_d|) of this angle's holograms, kept on the device beside them (the shift refinement multiplies it with a
        phase ramp per distance and minibatch)."""
        data = self.m._data(this_i_theta)
        if self._spec_key != self.m._data_key:
            self._spec_dev = self.holo.data_spectrum(data)
            self._spec_key = self.m._data_key
        return self._spec_dev

    def _run(self, a, want_grad, grad_obj=None, grads=None, want_pred=False, overwrite=False):      # (grads: by argument name)
        m, holo, g = self.m, self.holo, grads or {}
        nd = holo.n_dists
        probe = m._probe(a['probe_real'], a['probe_imag'])          # [1, ny, nx, 2]
        dists = m._dev('free_prop_cm', a['free_prop_cm'], (nd,))
        if m.common_vars.get('optimize_all_probe_pos'):   # forward_model.py:1075-1085
            if g.get('free_prop_cm') is not None:
                raise NotImplementedError('optimize_all_probe_pos together with optimize_free_prop is outside the accelerated path')
            shifts = m._dev('probe_pos_correction', a['probe_pos_correction'], (nd, 2))
            holo.forward_adjoint_shifted(a['obj'], probe, dists, self._spectrum(a['this_i_theta']), shifts, want_grad=want_grad, grad_obj=grad_obj,
                                         grad_probe=g.get('probe_real'), grad_shifts=g.get('probe_pos_correction'), want_pred=want_pred,
                                         overwrite=overwrite)
            return
        aff = None
        if m.common_vars.get('optimize_prj_affine'):      # forward_model.py:1063-1070
            aff = m._dev('prj_affine_ls', a['prj_affine_ls'], (nd, 2, 3))
        holo.forward_adjoint(a['obj'], probe, dists, m._data(a['this_i_theta']), affine=aff, want_grad=want_grad, grad_obj=grad_obj,
                             grad_probe=g.get('probe_real'), grad_dists=g.get('free_prop_cm'),
                             grad_affine=g.get('prj_affine_ls') if aff is not None else None, want_pred=want_pred, overwrite=overwrite)

    def predict(self, a):
        self._run(self.m._tied(a), want_grad=False, want_pred=True)
        return self.holo.pred()

    def loss(self, a):
        self._run(self.m._tied(a), want_grad=False)
        self.m.current_loss = float(self.holo.loss() + self.m._regularize(a['obj'], None))
        return self.m.current_loss

    def loss_and_gradients(self, opt_args_ls, grad_obj, a, side_hook, init_grad):
        m, holo = self.m, self.holo
        if side_hook is not None:
            side_hook()
        nd = holo.n_dists
        fa = getattr(m, 'fused_adam', None)
        h = m.homogeneous
        if fa is not None and h is not None:
            raise RuntimeError('fused holography update: it cannot carry ctf_lg_kappa (a run with the single-material constraint '
                               'takes the separate launches)')
        if fa is not None:
            # the driver has established that this minibatch's update is plain Adam on exactly these gradients (one rank, no
            # regulariser / constraint / mask): gradient launch group and optimiser steps are ONE call, nothing is returned
            free_prop_cm, prj_affine_ls = a['free_prop_cm'], a['prj_affine_ls']
            probe = m._probe(a['probe_real'], a['probe_imag'])
            dists = m._dev('free_prop_cm', free_prop_cm, (nd,))
            aff = m._dev('prj_affine_ls', prj_affine_ls, (nd, 2, 3)) if m.common_vars.get('optimize_prj_affine') else None
            if (fa['dists'] is not None and not isinstance(free_prop_cm, DeviceArray)) or \
                    (fa['affine'] is not None and not isinstance(prj_affine_ls, DeviceArray)):
                raise RuntimeError('fused holography update: the optimised parameters must live on the device')
            holo.forward_adjoint_adam(a['obj'], probe, dists, m._data(a['this_i_theta']), fa['obj_mv'], fa['step_obj'], fa['i_batch'], affine=aff,
                                      dists_mv=fa['dists'][:2] if fa['dists'] else None, step_dists=fa['dists'][2] if fa['dists'] else 0.,
                                      affine_mv=fa['affine'][:2] if fa['affine'] else None, step_affine=fa['affine'][2] if fa['affine'] else 0.,
                                      affine_pin=fa['pin'], b1=fa['b1'], b2=fa['b2'], eps=fa['eps'])
            datav = holo.loss_async()
            m._loss_thunk = lambda: datav()
            return tuple(None for _ in opt_args_ls)
        # init_grad: the object-gradient buffer holds garbage -> the engine overwrites every gradient ('=' instead of '+=': no
        # zero fills on a path that is bound by the number of launches); otherwise it accumulates into zeroed small buffers
        wanted = set(m.argument_ls[i] for i in opt_args_ls)
        grads = dict(obj=grad_obj)
        if 'probe_real' in wanted or 'probe_imag' in wanted:
            probe = m._probe(a['probe_real'], a['probe_imag'])
            grads['probe_real'] = grads['probe_imag'] = m._small_grad('_grad_probe_dev', probe.shape, refit=True)
        for name, attr, shape in (('free_prop_cm', '_gd', (nd,)), ('prj_affine_ls', '_ga', (nd, 2, 3))):
            if name in wanted:
                g = m._small_grad(attr, shape, owner=self)
                grads[name] = g if init_grad else g.zero_()
        if 'probe_pos_correction' in wanted:
            grads['probe_pos_correction'] = m._small_grad('_gs', (nd, 2), owner=self).zero_()           # (adm_holo_shift_grad accumulates)
        if h is None:
            self._run(a, want_grad=True, grad_obj=grad_obj, grads=grads, overwrite=bool(init_grad))
            pending = m._regularize_launch(a['obj'], grad_obj)
        else:
            # the data term on the tied object, into the tied-gradient buffer (grad_obj may hold earlier minibatches); then the fold
            t, gt = m._tied(a), h.tied_grad()
            self._run(t, want_grad=True, grad_obj=gt if init_grad else gt.zero_(), grads=grads, overwrite=bool(init_grad))
            pending = m._fold_tied(a, t, grad_obj, grads, wanted, init_grad)
        # loss and regulariser value are read back lazily (the driver looks at them after the next minibatch has been queued)
        regv = m._reg_value_async(pending)
        datav = holo.loss_async()
        m._loss_thunk = lambda: datav() + regv()
        return m._ordered_grads(opt_args_ls, grads)


class _TiledPath(object):
    """Data divided into sub-tiles and / or propagated with a safe zone (n_blocks > 1 or safe_zone_width > 0, forward_model.py:884-1034):
    ``common_vars_dict['tile_engine']`` is a MultisliceEngine built for the sequence of distances -- tile = sub-hologram + 2 safe
    zones, one detector-plane Fresnel kernel per distance in the plan (adm_plan_set_detector_kernels), detector mask = the
    sub-hologram's window -- and a minibatch of tiles at all distances is ONE launch of the multislice kernel with one probe
    window per entry (adm_multislice_fwd_adj_pp); object gradient only.
    One engine serves all distances: its plan holds the n_dists detector-plane kernels and a launch lists every tile of the
    minibatch n_dists times in a row ("tile-major": tile j at every distance, then tile j + 1), so entry b belongs to tile
    b // n_dists and distance b % n_dists.  The reference's order -- predictions and data -- is distance-major
    [i_dist * n_blocks + tile] (:1019-1021, 1051-1054); only predict() has to put its output back into it."""
    def __init__(self, model, engine):
        self.m, self.eng, self._probe_ident, self._tiles_resident = model, engine, None, None

    def check(self, safe_zone_width, ctf_lg_kappa, probe_pos_correction):
        cv = self.m.common_vars
        _check_fresnel(self.m, safe_zone_width, probe_pos_correction)
        if int(safe_zone_width or 0) != int(cv.get('safe_zone_width') or 0):
            raise ValueError('safe_zone_width differs from the width the tile engine was built for')
        for flag in ('optimize_free_prop', 'optimize_prj_affine'):
            if cv.get(flag):
                raise NotImplementedError('%s with multi-distance data divided into sub-tiles is outside the accelerated path' % flag)

    def _tile_probes(self, probe_real, probe_imag, pos):
        """One probe window [1, T, T] per launch entry, cut from the full-field probe padded with 1 + 0i
        (forward_model.py:916-925, 944-994).  Line :1005 passes ``subprobe_imag_ls_ls[k][i_mode, :, :]`` (no leading ':'): with
        one mode that is the IMAGINARY window of the first tile of the n_dp_batch chunk, used for the whole chunk -- kept, it is
        what the reference computes (golden F18 pins it with a probe that varies over the field).  The probe is not optimised on
        this path, so the windows of a batch are built once per distinct batch and stay on the device."""
        cv = self.m.common_vars
        szw = int(cv.get('safe_zone_width') or 0)
        T, nd = self.eng.probe_size, self.eng.n_dists
        # which probe the cached windows were cut from: a device array by identity (nothing updates it on this path: the driver
        # refuses optimize_probe with tiles), host arrays by content
        if isinstance(probe_real, DeviceArray):
            ident = ('dev', probe_real.ptr, tuple(probe_real.shape))
        else:
            host = np.stack([np.asarray(probe_real, np.float32), np.asarray(probe_imag, np.float32)], -1)
            ident = ('host', host.shape, host.tobytes())
        if self._probe_ident != ident:
            if isinstance(probe_real, DeviceArray):
                host = probe_real.get()
            self._probe_host = host.reshape(host.shape[-3], host.shape[-2], 2)
            self._probe_cache = {}
            self._probe_ident = ident
        key = pos.tobytes()
        dev = self._probe_cache.get(key)
        if dev is None:
            pr, pi = self._probe_host[..., 0], self._probe_host[..., 1]
            pad = np.zeros((2, 2), int)
            if szw > 0:
                pad = calculate_pad_len(pr.shape, pos - szw, T)
                pr = np.pad(pr, [tuple(pad[0]), tuple(pad[1])], mode='constant', constant_values=1)
                pi = np.pad(pi, [tuple(pad[0]), tuple(pad[1])], mode='constant', constant_values=0)
            n_dp = int(cv.get('n_dp_batch') or len(pos))
            host = np.empty((len(pos), 1, T[0], T[1], 2), np.float32)
            for j, p in enumerate(pos):
                y, x = int(p[0] + pad[0, 0] - szw), int(p[1] + pad[1, 0] - szw)
                j0 = (j // n_dp) * n_dp
                y0, x0 = int(pos[j0, 0] + pad[0, 0] - szw), int(pos[j0, 1] + pad[1, 0] - szw)
                host[j, 0, :, :, 0] = pr[y:y + T[0], x:x + T[1]]
                host[j, 0, :, :, 1] = pi[y0:y0 + T[0], x0:x0 + T[1]]
            if len(self._probe_cache) > 4096:
                self._probe_cache.clear()
            dev = self._probe_cache[key] = self.m.device.array(np.repeat(host, nd, axis=0))
        return dev

    def _tile_frames(self, this_i_theta, tiles):
        """The measured holograms of ``tiles`` at every distance, tile-major, each inside a zero frame of the tile's size (the
        safe zone carries no data and no weight in the loss): |prj[theta, i_dist * n_blocks + tile]| through get_data
        (forward_model.py:1049-1056)."""
        m, cv = self.m, self.m.common_vars
        szw = int(cv.get('safe_zone_width') or 0)
        T, nd = self.eng.probe_size, self.eng.n_dists
        n_blocks = m.prj.shape[1] // nd
        tiles = np.asarray(tiles)
        ind = (tiles[:, None] + n_blocks * np.arange(nd)[None, :]).reshape(-1)
        t = m.get_data(this_i_theta, ind, theta_downsample=cv.get('theta_downsample') or 1, ds_level=cv.get('ds_level', 1))
        if szw == 0:
            return t
        full = np.zeros((len(ind), T[0], T[1]), np.float32)
        full[:, szw:szw + t.shape[1], szw:szw + t.shape[2]] = t
        return full

    def _tile_targets(self, this_i_theta, this_ind_batch):
        """Datasets whose framed copy fits ADM_RESIDENT_DATA_MB live on the device, one tile-major [n_blocks * n_dists, Ty, Tx] array
        per angle: a minibatch that is a run of consecutive tiles (the reference sorts a minibatch's indices,
        adorym/ptychography.py:907) is a view of it -- no host work, no copy."""
        prj = self.m.prj
        T, nd = self.eng.probe_size, self.eng.n_dists
        n_blocks = prj.shape[1] // nd
        ind = np.asarray(this_ind_batch)
        if self._tiles_resident is None:
            limit = float(os.environ.get('ADM_RESIDENT_DATA_MB', '1024')) * 2 ** 20
            self._tiles_resident = {} if 4.0 * prj.shape[0] * prj.shape[1] * T[0] * T[1] <= limit else False
        if self._tiles_resident is not False and len(ind) > 0 and int(ind[-1]) - int(ind[0]) == len(ind) - 1 and np.all(np.diff(ind) == 1):
            key = int(this_i_theta)
            dev = self._tiles_resident.get(key)
            if dev is None:
                dev = self._tiles_resident[key] = self.m.device.array(self._tile_frames(this_i_theta, np.arange(n_blocks)))
            return dev.view(int(ind[0]) * nd * T[0] * T[1], (len(ind) * nd, T[0], T[1]))
        return self._tile_frames(this_i_theta, ind)

    def _run(self, a, want_grad, grad_obj=None, want_pred=False):
        """ONE launch over (tiles of the minibatch) x (distances).  The loss is the mean over distances x tiles x sub-hologram
        pixels (forward_model.py:1019-1029, 1087) -- the engine's mean over its n_dists * B entries and the kept detector pixels."""
        m, eng = self.m, self.eng
        szw = int(m.common_vars.get('safe_zone_width') or 0)
        nd = eng.n_dists
        pos = np.ascontiguousarray(np.round(np.asarray(a['this_pos_batch'])).astype(np.int64).reshape(-1, 2))
        B = len(pos)
        probes_b = self._tile_probes(a['probe_real'], a['probe_imag'], pos)
        tpos = np.repeat(pos - szw, nd, axis=0)
        eng.set_batch(tpos, self._tile_targets(a['this_i_theta'], a['this_ind_batch']))
        yr = eng.y_footprint(tpos)
        eng.rotate(a['obj'], None, yr)
        if want_grad:
            # the overlap-add's cover lists only need the positions: built on the side stream, beside the launch
            m.device.fork()
            eng.flush_loss_copy()
            eng.build_cover()
            m.device.end_fork()
        eng.multislice(None, want_grad=want_grad, want_pred=want_pred, probes_b=probes_b, accumulate=False)
        if want_grad:
            m.device.join()
            eng.accumulate_tiles()
            eng.rotate_adjoint(grad_obj, None, yr)
        if want_pred:
            sy, sx = m.prj.shape[-2:]
            p = eng.pred()[:, szw:szw + sy, szw:szw + sx]
            return np.ascontiguousarray(p.reshape(B, nd, sy, sx).transpose(1, 0, 2, 3).reshape(nd * B, sy, sx))
        tok = eng.loss_async()
        return lambda: eng.loss_result(tok)

    def predict(self, a):
        return self._run(a, want_grad=False, want_pred=True)

    def loss(self, a):
        datav = self._run(a, want_grad=False)
        self.m.current_loss = float(datav() + self.m._regularize(a['obj'], None))
        return self.m.current_loss

    def loss_and_gradients(self, opt_args_ls, grad_obj, a, side_hook, init_grad):
        m = self.m
        if side_hook is not None:
            side_hook()
        if list(opt_args_ls) != [0]:
            raise NotImplementedError('multi-distance data divided into sub-tiles: only the object gradient is on the accelerated path')
        # the regulariser kernel initialises the gradient buffer ('set' mode, or a zero fill), the launches add to it
        regv = m._reg_value_async(m._regularize_launch(a['obj'], grad_obj, init_grad=bool(init_grad)))
        datav = self._run(a, want_grad=True, grad_obj=grad_obj)
        m._loss_thunk = lambda: datav() + regv()
        return (grad_obj,)


class _FanoutPath(object):
    """A 3-D object (``two_d_mode=False``: holotomography, forward_model.py:905-914, 971-1019), one undivided field of view without a
    safe zone, ``forward_algorithm='fresnel'``: ``common_vars_dict['engine']`` is a MultisliceEngine built with
    ``detector_fanout=True`` for the sequence of distances and the whole field as its one position (0, 0).  The object is rotated
    with the angle's table as PtychographyModel does, ONE launch runs the slice sweep once and sends the exit wave to every distance
    (adm_plan_set_detector_fanout), and the rotation adjoint takes the gradient back; gradients w.r.t. obj and the probe.  An engine
    built with ``refine_distances=True`` also serves ``optimize_free_prop``: ``free_prop_cm`` is then the engine's device array
    ``engine.dists`` (the kernels follow it, adm_plan_set_fanout_distances) and the gradient w.r.t. it comes from the same launch.
    ``common_vars_dict['hologram_registration']`` (an adorym_amd.HologramRegistration) also serves ``optimize_prj_affine``: the raw
    holograms registered by ``prj_affine_ls`` are the launch's target (adm_register_targets) and the gradient w.r.t. the matrices is
    formed from the launch's predictions (adm_register_grad)."""
    def __init__(self, model, engine):
        self.m, self.eng, self.refine = model, engine, bool(getattr(engine, 'refine_distances', False))

    def check(self, safe_zone_width, ctf_lg_kappa, probe_pos_correction):
        m, eng, cv = self.m, self.eng, self.m.common_vars
        _check_fresnel(m, safe_zone_width, probe_pos_correction, _served(self, 'optimize_free_prop', 'optimize_prj_affine'))
        if cv.get('two_d_mode'):
            raise ValueError('MultiDistModel in two_d_mode takes a HolographyEngine (holo_engine), not an engine with detector_fanout')
        if m.registration is not None and cv.get('optimize_prj_affine'):
            m._check_registration(eng.n_dists, eng.probe_size)
            if eng.n_det != eng.probe_size[0] * eng.probe_size[1]:
                raise NotImplementedError('multi-distance holography of a 3-D object with optimize_prj_affine and a beamstop is outside '
                                          'the accelerated path')

    def _run(self, a, target, want_grad, want_affine_grad=False, **kw):
        """PtychographyModel._run on the whole field as the one position (0, 0): rotate, one fan-out launch, rotation adjoint.
        ``target`` None: this angle's holograms [n_dists, Y, X] (resident datasets: a view of the device copy)."""
        m, eng = self.m, self.eng
        finish = None
        if target is None:
            # the registered target is made on the main stream, in front of the rotation: the side stream is joined BEHIND the
            # launch, which would not wait for a target made there.  (The predictions stay on the device: engine.pred_device().)
            target, kw['want_pred'], finish = m._register(a['this_i_theta'], a['prj_affine_ls'], eng.n_dists, kw.get('want_pred', False),
                                                          want_affine_grad)
        if target is None:
            target = m._target(a['this_i_theta'], np.arange(eng.n_dists))
        fp = a['free_prop_cm']
        if self.refine and isinstance(fp, DeviceArray) and fp.ptr != eng.dists.ptr:
            raise ValueError('multi-distance holography of a 3-D object with refined distances: free_prop_cm on the device must be '
                             'the engine\'s own array (engine.dists)')
        out = PtychographyModel._run(m, a['obj'], a['probe_real'], a['probe_imag'], a['this_i_theta'], np.zeros((1, 2), int), target, want_grad, **kw)
        if finish is not None:
            finish(eng.pred_device())       # (the launch's grad_scale is 2 / (D Py Px), the kernel's own factor)
        return out

    def predict(self, a):
        # (distance-major like the reference's; for one block that is the launch's order)
        zeros = np.zeros((self.eng.n_dists,) + tuple(self.eng.probe_size), np.float32)
        self._run(self.m._tied(a), zeros, want_grad=False, want_pred=True, regularize=False)
        return self.eng.pred()

    def loss(self, a):
        m = self.m
        if m.homogeneous is None:
            self._run(a, None, want_grad=False)
        else:
            # (the data term on the tied object, the regulariser on the user's)
            self._run(m._tied(a), None, want_grad=False, regularize=False)
            m._reg_pending = m._regularize_launch(a['obj'], None)
        m._queue_loss()
        return m.current_loss

    def loss_and_gradients(self, opt_args_ls, grad_obj, a, side_hook, init_grad):
        m, h = self.m, self.m.homogeneous
        served = ('obj', 'probe_real', 'probe_imag') + _served(self, 'free_prop_cm', 'prj_affine_ls') + (('ctf_lg_kappa',) if h is not None else ())
        m._ordered_grads(opt_args_ls, dict.fromkeys(served), 'multi-distance holography of a 3-D object: the ')      # (in front of the launch)
        wanted = set(m.argument_ls[i] for i in opt_args_ls)
        more = dict(grad_dists=m._small_grad('_grad_dists_dev', self.eng.dists.shape)) if 'free_prop_cm' in wanted else None
        kw = dict(want_probe_grad='probe_real' in wanted or 'probe_imag' in wanted, side_hook=side_hook, more_grads=more,
                  want_affine_grad='prj_affine_ls' in wanted)
        grads = {}
        if h is None:
            gp, _ = self._run(a, None, want_grad=True, grad_obj=grad_obj, init_grad=init_grad, **kw)
        else:
            # the data term alone on the tied object (tied BEFORE the rotation, which is linear), zero-filled tied-gradient buffer
            # and no regulariser; then the regulariser of the user's object and the fold, behind the back-rotation
            t = m._tied(a)
            gp, _ = self._run(t, None, want_grad=True, grad_obj=h.tied_grad(), init_grad=True, regularize=False, **kw)
            m._reg_pending = m._fold_tied(a, t, grad_obj, grads, wanted, init_grad)
        m._queue_loss()          # m.current_loss fetches it on first access
        return m._ordered_grads(opt_args_ls, dict(grads, obj=grad_obj, probe_real=gp, probe_imag=gp, free_prop_cm=getattr(m, '_grad_dists_dev', None),
                                                  prj_affine_ls=getattr(m, '_grad_affine_dev', None)))


class _CTFPath(object):
    """``common_vars_dict['forward_algorithm'] == 'ctf'`` (forward_model.py:1011-1014, modulate_and_get_ctf): the contrast-transfer-function
    model of a weak, homogeneous object, I_d = 1 + Re IFFT2(2 (sin xi_d + cos xi_d / kappa) FFT2(delta)) with kappa = 10^ctf_lg_kappa[0].
    ``common_vars_dict['ctf_engine']`` is an adorym_amd.CTFEngine; gradients w.r.t. obj (beta's is exactly zero) and ctf_lg_kappa
    come from adm_ctf_fwd_adj.  Neither the probe nor beta enters the model; one undivided field of view only.  A 3-D object under
    this model (``two_d_mode=False``: :905-914 rotates it, propagate.py:467-476 sums it along the beam) is served when, and only
    when, ``common_vars_dict['ctf_projector']`` is an adorym_amd.RotatedProjector: the angle's projection (adm_rotate_project_fwd) is
    the engine's one slice and its gradient is back-projected into grad_obj (adm_rotate_project_adj); no rotated-frame buffer.
    Capability decides here as well, in 2-D and with a projector: a ``ctf_engine`` built with ``refine_distances=True`` serves
    ``optimize_free_prop`` (``free_prop_cm`` is then the engine's device array ``ctf_engine.dists`` or host values uploaded into
    it, and the gradient w.r.t. it comes from the same launch group, adm_ctfd_fwd_adj), and
    ``common_vars_dict['hologram_registration']`` serves ``optimize_prj_affine`` as on the fan-out path; the registered targets are
    magnitudes already, so that run's ``ctf_engine`` is built with raw_data_type='magnitude' and the registration carries the run's
    raw type."""
    REFUSED = "forward_algorithm='ctf' with %s is outside the accelerated path"

    def __init__(self, model, ctf, projector):
        # a 3-D object when the caller brought the projector that rotates and sums it (what the caller brought decides)
        self.m, self.ctf, self.projector, self.refine = model, ctf, projector, bool(getattr(ctf, 'refine_distances', False))
        if projector is not None and model.engine is None:
            model.engine = projector          # (its plan carries the object geometry for the regulariser kernels)

    def check(self, safe_zone_width, ctf_lg_kappa, probe_pos_correction):
        m, ctf, cv = self.m, self.ctf, self.m.common_vars
        what = None
        if cv.get('unknown_type', 'delta_beta') == 'real_imag':
            what = "unknown_type='real_imag'"
        elif int(cv.get('n_probe_modes') or 1) != 1:
            what = 'n_probe_modes != 1'
        elif not cv.get('two_d_mode') and self.projector is None:
            what = 'two_d_mode=False'
        elif m.tile_engine is not None or safe_zone_width not in (0, None) or int(cv.get('safe_zone_width') or 0) > 0:
            what = 'data divided into sub-tiles or safe_zone_width > 0'
        elif m.loss_function_type != 'lsq':
            what = "loss_function_type='%s'" % m.loss_function_type
        _refuse(what, cv, m.CTF_REFUSED_FLAGS, _served(self, 'optimize_free_prop', 'optimize_prj_affine'), self.REFUSED)
        if ctf_lg_kappa is None:
            raise ValueError("forward_algorithm='ctf' needs ctf_lg_kappa")
        if m.registration is not None and cv.get('optimize_prj_affine'):
            m._check_registration(ctf.n_dists, (ctf.ny, ctf.nx))
            if getattr(ctf, 'raw_data_type', None) != 'magnitude':
                raise ValueError("MultiDistModel: forward_algorithm='ctf' with optimize_prj_affine needs a ctf_engine built with "
                                 "raw_data_type='magnitude' (the registered holograms are magnitudes already)")
        if not cv.get('two_d_mode'):
            # a 3-D object: rotated inside the loop by the projector, on one rank, on a field the CTF engine takes
            sides = (ctf.ny, ctf.nx)
            if cv.get('rotate_out_of_loop'):
                what = 'two_d_mode=False and rotate_out_of_loop'
            elif int(cv.get('n_ranks') or 1) > 1:
                what = 'two_d_mode=False and more than one rank'
            elif any(n < 16 or n > 2048 or n & (n - 1) for n in sides) or tuple(self.projector.obj_size[:2]) != sides:
                what = 'two_d_mode=False and a field of %d x %d on a %d x %d x %d object (sides: powers of two in [16, 2048])' % (
                    sides + tuple(self.projector.obj_size))
            if what is not None:
                raise NotImplementedError(self.REFUSED % what)

    def _run(self, a, want_grad, grad_obj=None, grad_lg_kappa=None, want_pred=False, overwrite=False, grad_dists=None,
             prj_affine_ls=None, want_affine_grad=False):
        """One launch group of adm_ctf_fwd_adj: the distances go in as host doubles.  An engine that refines them (adm_ctfd_fwd_adj)
        takes its own device array, or host values that it uploads into it.  ``prj_affine_ls``, ``want_affine_grad``: see _register."""
        m, ctf = self.m, self.ctf
        obj, this_i_theta, free_prop_cm = a['obj'], a['this_i_theta'], a['free_prop_cm']
        nd = ctf.n_dists
        if self.refine:
            if isinstance(free_prop_cm, DeviceArray) and free_prop_cm.ptr != ctf.dists.ptr:
                raise ValueError("forward_algorithm='ctf' with refined distances: free_prop_cm on the device must be the engine's own "
                                 "array (ctf_engine.dists)")
            dists = free_prop_cm
        else:
            if grad_dists is not None:
                raise RuntimeError('gradient w.r.t. free_prop_cm requested but the CTF engine does not refine its distances')
            dists = free_prop_cm.get() if isinstance(free_prop_cm, DeviceArray) else free_prop_cm
            dists = np.asarray(dists, dtype=np.float64).reshape(nd)
        lgk = m._dev('ctf_lg_kappa', a['ctf_lg_kappa'], (1,))
        data = m._data(this_i_theta)
        target, want_pred, finish = m._register(this_i_theta, prj_affine_ls, nd, want_pred, want_affine_grad)
        if target is not None:
            data = target
        if self.projector is not None and not m.common_vars.get('two_d_mode'):
            # forward_model.py:905-914 + propagate.py:467-476: the rotated object summed along the beam is the model's one slice.
            # The launch group overwrites the slice's gradient (and kappa's and the distances': one launch per evaluation), the
            # back-projection adds it to grad_obj, which is zero-filled first where it holds garbage (``overwrite``).
            rp = self.projector
            table = m.common_vars['rotation_tables'](int(this_i_theta))
            proj = rp.project(obj, table)
            gproj = m._small_grad('_gproj', tuple(proj.shape), owner=self) if want_grad else None
            ctf.forward_adjoint(proj, dists, lgk, data, want_grad=want_grad, grad_obj=gproj, grad_lg_kappa=grad_lg_kappa, want_pred=want_pred,
                                overwrite=True, grad_dists=grad_dists)
            if want_grad:
                if overwrite:
                    grad_obj.zero_()
                rp.backproject(gproj, table, grad_obj)
        else:
            ctf.forward_adjoint(obj, dists, lgk, data, want_grad=want_grad, grad_obj=grad_obj, grad_lg_kappa=grad_lg_kappa, want_pred=want_pred,
                                overwrite=overwrite, grad_dists=grad_dists)
        if finish is not None:
            finish(ctf.pred_device())

    def predict(self, a):
        self._run(a, want_grad=False, want_pred=True)
        return self.ctf.pred()

    def loss(self, a):
        self._run(a, want_grad=False, prj_affine_ls=a['prj_affine_ls'])
        self.m.current_loss = float(self.ctf.loss() + self.m._regularize(a['obj'], None))
        return self.m.current_loss

    def loss_and_gradients(self, opt_args_ls, grad_obj, a, side_hook, init_grad):
        m = self.m
        if side_hook is not None:
            side_hook()
        served = ('obj', 'ctf_lg_kappa') + _served(self, 'free_prop_cm', 'prj_affine_ls')
        m._ordered_grads(opt_args_ls, dict.fromkeys(served), "forward_algorithm='ctf': the ")        # (the rest: refused in front of the launch)
        wanted = set(m.argument_ls[i] for i in opt_args_ls)
        # as on the undivided Fresnel path: '=' into a buffer that holds garbage, '+=' otherwise; the regulariser adds
        grads = dict(obj=grad_obj)
        for name, attr, shape in (('ctf_lg_kappa', '_gk', (1,)), ('free_prop_cm', '_gd', (self.ctf.n_dists,))):
            if name in wanted:
                g = m._small_grad(attr, shape, owner=self)
                grads[name] = g if init_grad else g.zero_()
        self._run(a, want_grad=True, grad_obj=grad_obj, grad_lg_kappa=grads.get('ctf_lg_kappa'), overwrite=bool(init_grad),
                  grad_dists=grads.get('free_prop_cm'), prj_affine_ls=a['prj_affine_ls'], want_affine_grad='prj_affine_ls' in wanted)
        regv = m._reg_value_async(m._regularize_launch(a['obj'], grad_obj))
        datav = self.ctf.loss_async()
        m._loss_thunk = lambda: datav() + regv()
        return m._ordered_grads(opt_args_ls, dict(grads, prj_affine_ls=getattr(m, '_grad_affine_dev', None)))
