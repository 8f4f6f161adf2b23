"""NumPy restatement of the reference's projection approximation (test infrastructure only: the checker, never the product).

  multislice_propagate_batch(..., pure_projection=True), unknown_type 'delta_beta'      adorym/propagate.py:158-193

built on the pinned oracle (oracle/adorym_oracle.py).  The reference sums the tile along the beam, p = sum_z tile, multiplies the
probe once by exp(-k1 p_beta) (cos, sin)(-sigma k1 p_delta) and goes to the detector: that is the oracle's multislice of an object
with ONE slice (one modulation, no propagation inside the sample; ``binning`` plays no part), the slice being the sum.  The
gradient of a sum w.r.t. each of its terms is the gradient w.r.t. the sum: the one-slice tile gradient, the same for every z.
"""
import numpy as np

from oracle import adorym_oracle as O


def project(a, dtype='float64'):
    """[..., S, 2] -> [..., 1, 2]: the sum along the beam, in ``dtype`` like the reference's tensors."""
    return np.asarray(a).astype(np.dtype(dtype), copy=False).sum(axis=-2, keepdims=True)


def forward_adjoint_tiles(tiles, probes, meas, phys, dtype='float64', **loss_kw):
    """Loss, prediction [B,Py,Px], grad_tiles [B,Py,Px,S,2], grad_probes complex [M,Py,Px] of the projection model on tiles
    [B,Py,Px,S,2] (and dL/dshifts [B,2] with ``shifts=``); ``phys`` and ``loss_kw`` as O.forward_adjoint_tiles takes them
    (phys.binning must be 1)."""
    if phys.binning != 1:
        raise ValueError('the projection model has no binning: build Physics with binning=1')
    dt = np.dtype(dtype)
    out = O.forward_adjoint_tiles(project(tiles, dt), probes, meas, phys, dt, **loss_kw)
    return out[:2] + (np.broadcast_to(out[2], np.shape(tiles)).astype(dt),) + out[3:]


def predict(tiles, probes, phys, dtype='float64'):
    return O.predict(project(tiles, dtype), probes, phys, dtype)[0]


def forward_adjoint_object(obj, coords_fp16, probes, pos_batch, meas, phys, dtype='float64', **loss_kw):
    """O.forward_adjoint_object for the projection model: rotate, cut tiles, sum them along the beam, evaluate the one-slice
    problem, overlap-add, copy to every slice, rotate back.  Returns loss, pred, the object gradient [Y,X,S,2], the probe gradient
    (and dL/dshifts with ``shifts=``)."""
    dt = np.dtype(dtype)
    obj = np.asarray(obj).astype(dt, copy=False)
    rot = O.rotate_fwd(obj, coords_fp16, dt) if coords_fp16 is not None else obj
    probes = np.asarray(probes)
    tiles, _ = O.extract_tiles(rot, pos_batch, probes.shape[-2:], phys.unknown_type)
    out = forward_adjoint_tiles(tiles, probes, meas, phys, dt, **loss_kw)
    g = O.scatter_tiles_adj(out[2], pos_batch, obj.shape)
    if coords_fp16 is not None:
        g = O.rotate_adj(g, coords_fp16, dt)
    return out[:2] + (g,) + out[3:]


# ---------------------------------------------------------------------------------------------- the kernel pair's host reference
def z_sum_and_bar(vol):
    """vol float32 [Z, ...] -> (S, bar): the float64 sum S over z of the float32 values and the bound on |got - S| for a result
    formed by a double accumulator in ANY order plus one rounding to float32:  2^-24 |S| + Z 2^-53 sum_z |v|.
    (Each of the at most Z - 1 double additions errs by at most 2^-53 of a partial sum, itself at most sum|v| (1 + Z 2^-53); the
    rounding to float32 adds half an ulp of the double result, at most 2^-24 of it.  No factor on top.)"""
    v = np.asarray(vol)
    assert v.dtype == np.float32
    S = v.astype(np.float64).sum(axis=0)
    return S, 2. ** -24 * np.abs(S) + v.shape[0] * 2. ** -53 * np.abs(v.astype(np.float64)).sum(axis=0)


def mixed_values(r, shape):
    """float32 values of mixed sign with magnitudes spread over 1e-8 ... 1e-2 (log-uniform)."""
    return (r.choice([-1., 1.], size=shape) * 10. ** r.uniform(-8, -2, size=shape)).astype(np.float32)
