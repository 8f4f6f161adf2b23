"""
Multi-distance near-field holography on the GPU: the engine behind MultiDistModel
(adorym/forward_model.py:809-1092) for one undivided field of view and one object slice.  See include/adm.h
(adm_holo_*) and csrc/adm_holo.hip.
"""
import ctypes as C
import numpy as np

from ._lib import HoloDesc, KAPPA_SCRATCH_DOUBLES, check
from .constants import PI
from .device import DeviceArray


class HolographyEngine(object):
    def __init__(self, ctx, field_size, n_dists, energy_ev, psize_cm, sign_convention=1, unknown_type='real_imag',
                 raw_data_type='intensity', scale_ri_by_k=True):
        self.ctx = ctx
        self.ny, self.nx = int(field_size[0]), int(field_size[1])
        self.n_dists = int(n_dists)
        lmbda_nm = 1240. / energy_ev
        voxel_nm = psize_cm * 1e7
        k1 = 2. * PI * voxel_nm / lmbda_nm if scale_ri_by_k else 1.
        desc = HoloDesc(ny=self.ny, nx=self.nx, n_dists=self.n_dists, lambda_nm=lmbda_nm, voxel_nm_y=voxel_nm, voxel_nm_x=voxel_nm,
                        sign_convention=int(sign_convention), unknown_type=1 if unknown_type == 'real_imag' else 0,
                        raw_intensity=1 if raw_data_type == 'intensity' else 0, k1=float(k1))
        h = C.c_void_p()
        check(ctx.lib.adm_holo_create(ctx.handle, C.byref(desc), C.byref(h)))
        self.handle = h
        # the per-distance loss sums are written by the last kernel of a launch group straight into page-locked HOST memory (two
        # slots, alternating): no device-to-host copy is queued, the host reads the slot once an event recorded behind the launch
        # has happened (the 4.6 us blit kernel and its dependency gap were 5 % of a config-5 minibatch)
        from .device import PinnedArray, Event
        self._pinned = [PinnedArray(ctx, (max(self.n_dists, 16),)) for _ in range(2)]
        self._events = [Event(ctx) for _ in range(2)]
        self._slot = 0
        self._pred = None

    def __del__(self):
        try:
            if getattr(self, 'handle', None) and self.ctx.handle:
                # (the handle keeps a pointer to the context: destroying it after Context.close() would touch freed memory)
                self.ctx.lib.adm_holo_destroy(self.handle)
                self.handle = None
        except Exception:
            pass

    def forward_adjoint(self, obj, probe, dists_cm, data, affine=None, want_grad=True, grad_obj=None, grad_probe=None,
                        grad_dists=None, grad_affine=None, want_pred=False, overwrite=False):
        """All arguments are DeviceArrays: obj [ny,nx,(1,)2], probe [ny,nx,2], dists_cm [n_dists], data [n_dists,ny,nx] (raw),
        affine [n_dists,2,3] or None.  Gradients are accumulated (+=) except grad_probe (overwritten); ``overwrite=True``:
        all of them are overwritten (no zero fills needed)."""
        if want_pred and self._pred is None:
            self._pred = DeviceArray(self.ctx, (self.n_dists, self.ny, self.nx), np.float32)
        p = lambda a: a.ptr if a is not None else None
        self._slot ^= 1
        check(self.ctx.lib.adm_holo_fwd_adj(self.handle, obj.ptr, probe.ptr, dists_cm.ptr, p(affine), data.ptr, (2 if overwrite else 1) if want_grad else 0,
                                            p(grad_obj), p(grad_probe), p(grad_dists), p(grad_affine),
                                            self._pred.ptr if want_pred else None, self._pinned[self._slot].handle))

    def forward_adjoint_adam(self, obj, probe, dists_cm, data, obj_mv, step_obj, i_batch, affine=None, dists_mv=None, step_dists=0.,
                             affine_mv=None, step_affine=0., affine_pin=None, b1=0.9, b2=0.999, eps=1e-7, want_pred=False):
        """forward_adjoint(overwrite=True) FUSED with the Adam steps of the object (always), the distances (``dists_mv`` = (m, v)
        DeviceArrays, or None) and the affine matrices (``affine_mv``, with ``affine_pin`` = DeviceArray copied over the first
        entries afterwards): adm_holo_fwd_adj_adam.  obj / dists_cm / affine are updated in place; no gradient is stored."""
        from ._lib import HoloAdam
        if want_pred and self._pred is None:
            self._pred = DeviceArray(self.ctx, (self.n_dists, self.ny, self.nx), np.float32)
        p = lambda a: a.ptr if a is not None else None
        o = HoloAdam(m_obj=obj_mv[0].ptr, v_obj=obj_mv[1].ptr, step_obj=float(step_obj),
                     m_dists=p(dists_mv[0]) if dists_mv else None, v_dists=p(dists_mv[1]) if dists_mv else None, step_dists=float(step_dists),
                     m_affine=p(affine_mv[0]) if affine_mv else None, v_affine=p(affine_mv[1]) if affine_mv else None,
                     step_affine=float(step_affine), affine_pin=p(affine_pin), affine_pin_n=affine_pin.size if affine_pin is not None else 0,
                     i_batch=int(i_batch), b1=float(b1), b2=float(b2), eps=float(eps))
        self._slot ^= 1
        check(self.ctx.lib.adm_holo_fwd_adj_adam(self.handle, obj.ptr, probe.ptr, dists_cm.ptr, p(affine), data.ptr, C.byref(o),
                                                 self._pred.ptr if want_pred else None, self._pinned[self._slot].handle))

    # ---- per-distance shift refinement of the measured holograms (optimize_all_probe_pos, adorym/forward_model.py:1075-1085) ----
    def data_spectrum(self, data):
        """FFT2(|data_d|) of the raw holograms [n_dists, ny, nx] (DeviceArray), transposed ([d][kx][ky]); once per dataset."""
        spec = DeviceArray(self.ctx, (self.n_dists, self.nx, self.ny, 2), np.float32)
        check(self.ctx.lib.adm_holo_data_spectrum(self.handle, data.ptr, spec.ptr))
        return spec

    def forward_adjoint_shifted(self, obj, probe, dists_cm, spectrum, shifts, want_grad=True, grad_obj=None, grad_probe=None,
                                grad_shifts=None, want_pred=False, overwrite=False):
        """forward_adjoint() against the holograms Fourier-shifted by ``shifts`` [n_dists, 2] = (sy, sx) (realign_image_fourier, real
        part kept): the registered targets are formed from ``spectrum`` (data_spectrum) in front of the launch group and, with
        ``grad_shifts`` (+=), dL/dshifts behind it."""
        if getattr(self, '_targets', None) is None:
            self._targets = DeviceArray(self.ctx, (self.n_dists, self.ny, self.nx), np.float32)
            self._cot = DeviceArray(self.ctx, (self.n_dists, self.ny, self.nx), np.float32)
        lib = self.ctx.lib
        check(lib.adm_holo_shift_targets(self.handle, spectrum.ptr, shifts.ptr, self._targets.ptr))
        want_sg = want_grad and grad_shifts is not None
        check(lib.adm_holo_set_registration(self.handle, self._cot.ptr if want_sg else None, 1))
        try:
            self.forward_adjoint(obj, probe, dists_cm, self._targets, want_grad=want_grad, grad_obj=grad_obj, grad_probe=grad_probe,
                                 want_pred=want_pred, overwrite=overwrite)
        finally:
            check(lib.adm_holo_set_registration(self.handle, None, 0))
        if want_sg:
            check(lib.adm_holo_shift_grad(self.handle, self._cot.ptr, spectrum.ptr, shifts.ptr, grad_shifts.ptr))

    def shifted_targets(self):
        """The registered holograms T_d of the last forward_adjoint_shifted() (host copy; tests)."""
        return self._targets.get()

    def loss(self):
        """mean over (distance, pixel) of the squared residual of the last launch -- blocks."""
        return self.loss_async()()

    def loss_async(self):
        """Record an event behind the last launch and return a callable that gives its loss: the host does not wait, the driver
        resolves it after the next minibatch has been queued (the next launch writes the OTHER slot)."""
        k = self._slot
        self._events[k].record()
        norm = float(self.n_dists * self.ny * self.nx)

        def value():
            self._events[k].synchronize()
            return float(self._pinned[k].array[:self.n_dists].astype(np.float64).sum() / norm)
        return value

    def pred(self):
        return self._pred.get()


class CTFEngine(object):
    """The contrast-transfer-function model of multi-distance holography (forward_algorithm='ctf'; adorym/propagate.py:467-476,
    590-606) for one undivided field of view and one object slice in 'delta_beta'.  See include/adm.h (adm_ctf_*) and
    csrc/adm_holo_ctf.hip.  No probe enters; the gradient w.r.t. beta is exactly zero.

    ``refine_distances=True``: the distances are parameters (the reference's optimize_free_prop under 'ctf').  ``self.dists``
    (DeviceArray float32 [n_dists], cm; ``dists_cm`` fills it) is the parameter itself: the kernels read it in every launch, so an
    optimiser moves it in place, and forward_adjoint takes ``grad_dists`` (adm_ctfd_fwd_adj, csrc/adm_ctf_dist.hip)."""

    def __init__(self, ctx, field_size, n_dists, energy_ev, psize_cm, raw_data_type='intensity', refine_distances=False, dists_cm=None):
        from ._lib import CtfDesc
        from .device import PinnedArray, Event
        self.ctx = ctx
        self.ny, self.nx = int(field_size[0]), int(field_size[1])
        self.n_dists = int(n_dists)
        desc = CtfDesc(ny=self.ny, nx=self.nx, n_dists=self.n_dists, raw_intensity=1 if raw_data_type == 'intensity' else 0,
                       energy_ev=float(energy_ev), psize_cm=float(psize_cm))
        h = C.c_void_p()
        check(ctx.lib.adm_ctf_create(ctx.handle, C.byref(desc), C.byref(h)))
        self.handle = h
        self.raw_data_type = raw_data_type
        self.refine_distances = bool(refine_distances)
        self.dists = None
        if self.refine_distances:
            self.dists = DeviceArray(ctx, (self.n_dists,), np.float32)
            self.dists.set(self._host_dists(np.zeros(self.n_dists) if dists_cm is None else dists_cm).astype(np.float32))
        elif dists_cm is not None:
            raise ValueError('CTFEngine: dists_cm belongs to refine_distances=True (otherwise every call names its distances)')
        # the per-distance loss sums go straight into page-locked host memory, two alternating slots (see HolographyEngine)
        self._pinned = [PinnedArray(ctx, (max(self.n_dists, 16),)) for _ in range(2)]
        self._events = [Event(ctx) for _ in range(2)]
        self._slot = 0
        self._pred = None

    def __del__(self):
        try:
            if getattr(self, 'handle', None) and self.ctx.handle:
                self.ctx.lib.adm_ctf_destroy(self.handle)
                self.handle = None
        except Exception:
            pass

    def _host_dists(self, dists_cm):
        d = np.ascontiguousarray(np.asarray(dists_cm, dtype=np.float64).reshape(-1))
        if d.size != self.n_dists:
            raise ValueError('CTFEngine: %d distances given, %d expected' % (d.size, self.n_dists))
        return d

    def forward_adjoint(self, obj, dists_cm, lg_kappa, data, want_grad=True, grad_obj=None, grad_lg_kappa=None, want_pred=False,
                        overwrite=False, grad_dists=None):
        """obj [ny,nx,(1,)2], lg_kappa [1], data [n_dists,ny,nx] (raw) are DeviceArrays; dists_cm is a HOST sequence of n_dists
        distances in cm.  grad_obj's delta channel and grad_lg_kappa are accumulated (+=; the beta channel is left alone), or
        overwritten with ``overwrite=True`` (beta channel = 0).
        An engine with ``refine_distances``: dists_cm is ``self.dists`` itself, or host values that are uploaded into it first;
        ``grad_dists`` (DeviceArray float32 [n_dists]) takes dL/d dists in 1/cm like the other gradients."""
        if want_pred and self._pred is None:
            self._pred = DeviceArray(self.ctx, (self.n_dists, self.ny, self.nx), np.float32)
        p = lambda a: a.ptr if a is not None else None
        mode = (2 if overwrite else 1) if want_grad else 0
        if not self.refine_distances:
            if grad_dists is not None:
                raise ValueError('grad_dists: the engine was built without refine_distances=True')
            if isinstance(dists_cm, DeviceArray):
                raise ValueError('CTFEngine: distances on the device need refine_distances=True')
            d = self._host_dists(dists_cm)
            self._slot ^= 1
            check(self.ctx.lib.adm_ctf_fwd_adj(self.handle, obj.ptr, d.ctypes.data_as(C.POINTER(C.c_double)), lg_kappa.ptr, data.ptr,
                                               mode, p(grad_obj), p(grad_lg_kappa),
                                               self._pred.ptr if want_pred else None, self._pinned[self._slot].handle))
            return
        if isinstance(dists_cm, DeviceArray):
            if dists_cm.ptr != self.dists.ptr:
                raise ValueError("CTFEngine: with refine_distances the distances on the device are the engine's own array (engine.dists)")
        else:
            self.dists.set(self._host_dists(dists_cm).astype(np.float32))
        if grad_dists is not None and (not isinstance(grad_dists, DeviceArray) or grad_dists.size != self.n_dists or grad_dists.dtype != np.float32):
            raise ValueError('grad_dists must be a float32 DeviceArray [%d]' % self.n_dists)
        self._slot ^= 1
        check(self.ctx.lib.adm_ctfd_fwd_adj(self.handle, obj.ptr, self.dists.ptr, lg_kappa.ptr, data.ptr, mode, p(grad_obj), p(grad_lg_kappa),
                                            p(grad_dists), self._pred.ptr if want_pred else None, self._pinned[self._slot].handle))

    def loss(self):
        """mean over (distance, pixel) of the squared residual of the last launch -- blocks."""
        return self.loss_async()()

    def loss_async(self):
        """Record an event behind the last launch and return a callable that gives its loss (see HolographyEngine.loss_async)."""
        k = self._slot
        self._events[k].record()
        norm = float(self.n_dists * self.ny * self.nx)

        def value():
            self._events[k].synchronize()
            return float(self._pinned[k].array[:self.n_dists].astype(np.float64).sum() / norm)
        return value

    def pred(self):
        return self._pred.get()

    def pred_device(self):
        """The predictions of the last launch with want_pred, on the device [n_dists, ny, nx]."""
        return self._pred


class CTFInversion(object):
    """The direct inversion of the CTF model (update_using_external_algorithm='ctf'; adorym/conventional.py:112-152,
    multidistance_ctf_wrapped): the phase map of an angle from its multi-distance holograms in closed form,
        phase = Re IFFT2( sum_d w_d FFT2(I_d - 1) / (sum_d 2 w_d^2 + alpha) ),   w_d = sin xi_d + cos xi_d / kappa.
    See include/adm.h (adm_ctfinv_*) and csrc/adm_ctf_invert.hip.  ``alpha``: None (the reference's 1e-10), a scalar, or an
    [ny, nx] array in the order of np.fft.fftfreq (the frequency-dependent regulariser of adorym/util.py:1601-1626, which the
    caller builds); every entry finite and > 0.  ``max_batch``: the angles one launch group takes."""

    def __init__(self, ctx, field_size, n_dists, energy_ev, psize_cm, max_batch=1, alpha=None):
        from ._lib import CtfInvDesc
        self.ctx = ctx
        self.ny, self.nx = int(field_size[0]), int(field_size[1])
        self.n_dists, self.max_batch = int(n_dists), int(max_batch)
        desc = CtfInvDesc(ny=self.ny, nx=self.nx, n_dists=self.n_dists, max_batch=self.max_batch, energy_ev=float(energy_ev),
                          psize_cm=float(psize_cm))
        table = None
        if alpha is not None:
            a = np.asarray(alpha, dtype=np.float32)
            if a.ndim == 0:
                a = np.full((self.ny, self.nx), a, dtype=np.float32)
            if a.shape != (self.ny, self.nx):
                raise ValueError('CTFInversion: alpha must be a scalar or %r, got %r' % ([self.ny, self.nx], list(a.shape)))
            table = np.ascontiguousarray(a)
        h = C.c_void_p()
        check(ctx.lib.adm_ctfinv_create(ctx.handle, C.byref(desc), table.ctypes.data if table is not None else None, C.byref(h)))
        self.handle = h
        self._registration = None
        self._out = None

    def __del__(self):
        try:
            if getattr(self, 'handle', None) and self.ctx.handle:
                self.ctx.lib.adm_ctfinv_destroy(self.handle)
                self.handle = None
        except Exception:
            pass

    def _checked(self, a, shapes, name):
        if not isinstance(a, DeviceArray):
            raise TypeError('CTFInversion: %s must be a DeviceArray' % name)
        if a.dtype != np.float32 or tuple(a.shape) not in shapes:
            raise ValueError('CTFInversion: %s must be float32 %s, got %s %r'
                             % (name, ' or '.join(repr(list(s)) for s in shapes), np.dtype(a.dtype).name, list(a.shape)))
        return a

    def retrieve(self, data, dists_cm, lg_kappa, out=None, into_object=False, affine=None):
        """data [B, D, ny, nx] or [D, ny, nx] raw holograms (used as given: I - 1) and lg_kappa [1] are DeviceArrays; dists_cm is a
        HOST sequence of D distances in cm.  Returns the phase maps [B, ny, nx]: ``out`` when given, else the engine's own
        DeviceArray, overwritten by the next call.  B may exceed max_batch: the angles go in rounds of max_batch.
        ``into_object=True`` (B = 1): ``out`` is an object [ny, nx, (1,) 2] whose delta channel is overwritten; the beta channel is
        not touched.  ``affine`` [D, 2, 3] (DeviceArray, B = 1): the holograms first pass through a HologramRegistration built with
        raw_data_type='magnitude' -- bilinear samples of |data| replace the reference's signed sample (holograms are positive).
        Everything is queued on the stream the context is enqueuing on."""
        ny, nx, D = self.ny, self.nx, self.n_dists
        d = np.ascontiguousarray(np.asarray(dists_cm, dtype=np.float64).reshape(-1))
        if d.size != D:
            raise ValueError('CTFInversion: %d distances given, %d expected' % (d.size, D))
        B = int(data.shape[0]) if isinstance(data, DeviceArray) and len(data.shape) == 4 and data.shape[0] >= 1 else 1
        self._checked(data, [(B, D, ny, nx), (D, ny, nx)], 'data')
        self._checked(lg_kappa, [(1,)], 'lg_kappa')
        if affine is not None:
            if B != 1:
                raise ValueError('CTFInversion: affine registration takes one angle (B = 1), got B = %d' % B)
            self._checked(affine, [(D, 2, 3)], 'affine')
            if self._registration is None:
                self._registration = HologramRegistration(self.ctx, D, (ny, nx), raw_data_type='magnitude')
            data = self._registration.targets(data.view(0, (D, ny, nx)), affine)
        if into_object:
            if B != 1:
                raise ValueError('CTFInversion: into_object takes one angle (B = 1), got B = %d' % B)
            if out is None:
                raise ValueError('CTFInversion: into_object needs the object as out')
            self._checked(out, [(ny, nx, 2), (ny, nx, 1, 2)], 'out')
        elif out is None:
            if self._out is None or self._out.shape[0] != B:
                self._out = DeviceArray(self.ctx, (B, ny, nx), np.float32)
            out = self._out
        else:
            self._checked(out, [(B, ny, nx)] + ([(ny, nx)] if B == 1 else []), 'out')
        dp = d.ctypes.data_as(C.POINTER(C.c_double))
        n = ny * nx
        for b0 in range(0, B, self.max_batch):
            nb = min(self.max_batch, B - b0)
            check(self.ctx.lib.adm_ctfinv_run(self.handle, data.ptr + 4 * b0 * D * n, nb, dp, lg_kappa.ptr, out.ptr + 4 * b0 * n,
                                              2 if into_object else 1))
        return out


class HologramRegistration(object):
    """The affine registration of measured holograms as kernels of its own (optimize_prj_affine, adorym/forward_model.py:1066-1072;
    w.affine_transform, wrappers.py:1159-1174) for forward models that are not HolographyEngine's: multi-distance holography of a
    3-D object, where the registered holograms are the ``target`` of the fan-out launch and its predictions feed the gradient
    w.r.t. the matrices.  See include/adm.h (adm_register_*) and csrc/adm_register.hip.  Any field from 2 x 2 to 2048 x 2048,
    1 to 64 distances."""

    def __init__(self, ctx, n_dists, field_size, raw_data_type='magnitude'):
        if raw_data_type not in ('magnitude', 'intensity'):
            raise ValueError("raw_data_type must be 'magnitude' or 'intensity'")
        self.ctx = ctx
        self.n_dists = int(n_dists)
        self.ny, self.nx = int(field_size[0]), int(field_size[1])
        self.raw_data_type = raw_data_type
        h = C.c_void_p()
        check(ctx.lib.adm_register_create(ctx.handle, self.n_dists, self.ny, self.nx, 1 if raw_data_type == 'intensity' else 0, C.byref(h)))
        self.handle = h
        self._target = DeviceArray(ctx, (self.n_dists, self.ny, self.nx), np.float32)

    def __del__(self):
        try:
            if getattr(self, 'handle', None) and self.ctx.handle:
                self.ctx.lib.adm_register_destroy(self.handle)
                self.handle = None
        except Exception:
            pass

    def _checked(self, a, shape, name):
        if not isinstance(a, DeviceArray):
            raise TypeError('HologramRegistration: %s must be a DeviceArray' % name)
        if a.dtype != np.float32 or a.size != int(np.prod(shape)):
            raise ValueError('HologramRegistration: %s must be float32 %r, got %s %r' % (name, list(shape), np.dtype(a.dtype).name, list(a.shape)))
        return a.ptr

    def targets(self, data, affine):
        """data [D, Py, Px] raw holograms (taken as |data|), affine [D, 2, 3]: DeviceArrays.  Returns the engine's own DeviceArray
        [D, Py, Px] of registered magnitudes, overwritten by the next call; queued on the stream the context is enqueuing on."""
        shape = (self.n_dists, self.ny, self.nx)
        check(self.ctx.lib.adm_register_targets(self.handle, self._checked(data, shape, 'data'),
                                                self._checked(affine, (self.n_dists, 2, 3), 'affine'), self._target.ptr))
        return self._target

    def grad(self, data, affine, pred, grad_affine, grad_scale=1.):
        """grad_affine [D, 2, 3] += grad_scale * dL/d affine of L = mean (pred - target)^2 over all D * Py * Px values, with ``pred``
        [D, Py, Px] the predicted magnitudes on the device (MultisliceEngine.pred_device())."""
        shape = (self.n_dists, self.ny, self.nx)
        check(self.ctx.lib.adm_register_grad(self.handle, self._checked(data, shape, 'data'), self._checked(affine, (self.n_dists, 2, 3), 'affine'),
                                             self._checked(pred, shape, 'pred'), float(grad_scale),
                                             self._checked(grad_affine, (self.n_dists, 2, 3), 'grad_affine')))


class HomogeneousObject(object):
    """The single-material constraint of Fresnel multi-distance holography (optimize_ctf_lg_kappa with forward_algorithm='fresnel':
    multislice_propagate_batch(..., kappa=10^ctf_lg_kappa[0]), adorym/propagate.py:223-225): the forward model sees the TIED object
    (delta, kappa delta) in place of the user's (delta, beta), and the gradient w.r.t. the tied object is folded back into the
    gradients w.r.t. delta and ctf_lg_kappa.  Owns the tied object, the tied gradient and the partial sums; ``obj_shape`` is the
    object's, [Y, X, Z, 2] or [Y, X, 2] ('delta_beta' unknowns).  See include/adm.h (adm_kappa_*) and csrc/adm_kappa_tie.hip.
    NOTE the sense: beta = kappa delta here, cos(xi) / kappa in the CTF model (CTFEngine) -- the reference's two meanings."""

    def __init__(self, ctx, obj_shape):
        shape = tuple(int(s) for s in obj_shape)
        if len(shape) < 2 or shape[-1] != 2 or min(shape) < 1:
            raise ValueError('HomogeneousObject: obj_shape must end in the (delta, beta) axis of length 2, got %r' % (list(obj_shape),))
        self.ctx, self.shape = ctx, shape
        self.n_vox = int(np.prod(shape[:-1]))
        self._tied = DeviceArray(ctx, shape, np.float32)
        self._grad = DeviceArray(ctx, shape, np.float32)
        self._scratch = DeviceArray(ctx, (KAPPA_SCRATCH_DOUBLES,), np.float64)

    def _checked(self, a, name, size=None):
        size = 2 * self.n_vox if size is None else size
        if not isinstance(a, DeviceArray):
            raise TypeError('HomogeneousObject: %s must be a DeviceArray' % name)
        if a.dtype != np.float32 or a.size != size:
            raise ValueError('HomogeneousObject: %s must be float32 of %d values, got %s %r' % (name, size, np.dtype(a.dtype).name, list(a.shape)))
        return a.ptr

    def tie(self, obj, lg_kappa):
        """The tied object (delta, fl32(kappa) delta) of ``obj`` under ``lg_kappa`` (DeviceArray [1]): the engine's own DeviceArray,
        overwritten by the next call; queued on the stream the context is enqueuing on.  obj's beta channel is not read."""
        check(self.ctx.lib.adm_kappa_tie(self.ctx.handle, self._checked(obj, 'obj'), self._checked(lg_kappa, 'lg_kappa', 1), self.n_vox,
                                         self._tied.ptr))
        return self._tied

    def tied_grad(self):
        """The buffer for dL/d(tied object), the engine's own and NOT initialised: the forward model overwrites it, or the caller
        zero-fills it where the model accumulates."""
        return self._grad

    def fold(self, obj, lg_kappa, grad_obj, grad_lg_kappa, overwrite=False):
        """tied_grad() folded into the gradients of the free unknowns: grad_obj.delta (+)= g_delta + fl32(kappa) g_beta and, if
        given, grad_lg_kappa[0] (+)= ln10 kappa sum(delta g_beta).  ``overwrite``: both are set ('=') and grad_obj.beta is zeroed --
        for buffers that hold garbage; otherwise both are added to and grad_obj.beta is left as it is."""
        gk = None if grad_lg_kappa is None else self._checked(grad_lg_kappa, 'grad_lg_kappa', 1)
        check(self.ctx.lib.adm_kappa_fold(self.ctx.handle, self._checked(obj, 'obj'), self._checked(lg_kappa, 'lg_kappa', 1), self._grad.ptr,
                                          self.n_vox, 2 if overwrite else 1, self._checked(grad_obj, 'grad_obj'), gk, self._scratch.ptr))
