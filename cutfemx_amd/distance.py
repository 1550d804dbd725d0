"""cutfemx.distance of the reference, the part a moving-domain loop needs: reinitialize(phi, max_iter, tol)
(python/cutfemx/distance.py:154-160) -- a P1 level set back to a signed distance function, in HBM (cfx_reinitialize).
"""
from __future__ import annotations

import ctypes as C
from dataclasses import dataclass

import numpy as np

from . import _lib
from .mesh import Function

REINIT_CONVERGED, REINIT_MAX_ITER, REINIT_NO_INTERFACE = (_lib.REINIT_CONVERGED, _lib.REINIT_MAX_ITER,
                                                          _lib.REINIT_NO_INTERFACE)
_REASONS = {REINIT_CONVERGED: "converged", REINIT_MAX_ITER: "max_iter", REINIT_NO_INTERFACE: "no_interface"}


@dataclass
class ReinitInfo:
    """cfx_reinit_info: why reinitialize stopped, the sweeps that had vertices to update, the seed vertices (those with
    a finite near-field distance) and the vertex updates computed."""
    reason: int
    sweeps: int
    seeds: int
    updates: int

    @property
    def converged(self) -> bool:
        return self.reason == REINIT_CONVERGED

    @property
    def reason_name(self) -> str:
        return _REASONS.get(self.reason, "running")


def reinit_default_options() -> _lib.ReinitOptions:
    """The defaults of cfx_reinit_options_default (no GPU needed)."""
    o = _lib.ReinitOptions()
    _lib.check(_lib.load().cfx_reinit_options_default(C.byref(o)))
    return o


def reinit_info_buffer():
    """A device buffer for `reinitialize(..., info_out=)`: 24 bytes that hold a cfx_reinit_info; read with
    read_reinit_info."""
    return _lib.DeviceBuffer(3, np.float64)


def read_reinit_info(info_out) -> ReinitInfo:
    """The ReinitInfo a reinitialize call left in `info_out` (one copy to the host)."""
    raw = (info_out.numpy() if isinstance(info_out, _lib.DeviceBuffer) else info_out.cpu().numpy()).tobytes()
    st = _lib.ReinitInfoStruct.from_buffer_copy(raw[:C.sizeof(_lib.ReinitInfoStruct)])
    return ReinitInfo(int(st.reason), int(st.sweeps), int(st.seeds), int(st.updates))


def reinitialize(phi: Function, max_iter: int = 1000, tol: float = 1e-10, *, max_distance: float | None = None,
                 check_every: int = 8, info_out=None):
    """Turn the P1 level set `phi` into the signed distance to its own zero contour, in place on `phi.values` (a numpy
    array, or a device torch tensor that never leaves HBM); returns a ReinitInfo.

    `phi` lives on a scalar degree-1 space on the geometry dofmap (FunctionSpace(mesh, 1)).  Signs and exact zeros are
    kept.  `max_iter` counts sweeps (about 1.3 x largest distance / h are needed); `tol` is kept for the reference's
    signature: the iteration ends when no vertex is left to update.  `max_distance`: compute the distance only up to that
    value and clamp the rest to it -- a few layers cost a few sweeps.  `check_every`: how often the host looks at the
    state; the result does not depend on it.  `info_out` (reinit_info_buffer()): the info stays in HBM and is returned
    as it stands; with device values and check_every = 0 the call then makes no host round trip: exactly `max_iter`
    sweeps are launched and the ones after convergence return at once.  Without an interface (no sign change, no zero)
    `phi` is left untouched and the reason is REINIT_NO_INTERFACE."""
    V = phi.function_space
    n = V.ndofs * V.bs
    vals = phi.values
    o = reinit_default_options()
    o.max_iter, o.tol, o.check_every = int(max_iter), float(tol), int(check_every)
    o.max_distance = 0.0 if max_distance is None else float(max_distance)
    keep: list = []
    if _lib.is_device(vals):
        if _lib.is_torch(vals):
            import torch
            if vals.dtype != torch.float64 or not vals.is_contiguous():
                raise TypeError("phi.values must be a contiguous float64 tensor (it is overwritten in place)")
        if (vals.numel() if _lib.is_torch(vals) else vals.size) != n:
            raise ValueError(f"phi.values must hold {n} values")
        pp = _lib.as_ptr(vals, np.float64, keep)
    else:
        if not (isinstance(vals, np.ndarray) and vals.dtype == np.float64 and vals.flags.c_contiguous):
            vals = phi.values = np.ascontiguousarray(vals, dtype=np.float64)
        if vals.size != n:
            raise ValueError(f"phi.values must hold {n} values")
        pp = vals.ctypes.data_as(C.c_void_p)
    fn = _lib.lib().cfx_reinitialize
    if info_out is not None:
        if not _lib.is_device(info_out):
            raise TypeError("reinitialize: info_out is a device buffer (reinit_info_buffer())")
        _lib.check(fn(V._h, pp, C.byref(o), _lib.as_ptr(info_out, np.float64, keep)))
        return info_out
    st = _lib.ReinitInfoStruct()
    _lib.check(fn(V._h, pp, C.byref(o), C.byref(st)))
    return ReinitInfo(int(st.reason), int(st.sweeps), int(st.seeds), int(st.updates))
