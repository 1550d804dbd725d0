"""cutfemx.distance of the reference, the part a moving-domain loop needs: reinitialize(phi, max_iter, tol)
(python/cutfemx/distance.py:154-160) -- a P1 level set back to a signed distance function, in HBM (cfx_reinitialize) --
extend_normal_velocity (cfx_extend_normal_velocity), and advect, the demos' characteristic step that moves phi
(cfx_advect_level_set).
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


@dataclass
class ExtendInfo(ReinitInfo):
    """cfx_extend_info: the ReinitInfo of the distance stage, the transport sweeps that changed a payload and the
    vertices that take their payload from sources (the others are near the interface, or were never reached)."""
    transport_sweeps: int = 0
    transported: int = 0


@dataclass
class NormalExtensionResult:
    """What extend_normal_velocity returns (the reference's NormalExtensionResult): `speed` on V, `velocity` = speed x
    unit normal on FunctionSpace(mesh, 1, bs=gdim), `signed_distance` on V, and the ExtendInfo (or the device buffer
    given as info_out)."""
    speed: Function
    velocity: Function
    signed_distance: Function
    info: object = None


def extend_info_buffer():
    """A device buffer for `extend_normal_velocity(..., info_out=)`: 40 bytes that hold a cfx_extend_info; read with
    read_extend_info."""
    return _lib.DeviceBuffer(5, np.float64)


def _extend_info(st) -> ExtendInfo:
    return ExtendInfo(int(st.reason), int(st.sweeps), int(st.seeds), int(st.updates), int(st.transport_sweeps),
                      int(st.transported))


def read_extend_info(info_out) -> ExtendInfo:
    """The ExtendInfo an extend_normal_velocity call left in `info_out` (one copy to the host)."""
    raw = (info_out.numpy() if isinstance(info_out, _lib.DeviceBuffer) else info_out.cpu().numpy()).tobytes()
    return _extend_info(_lib.ExtendInfoStruct.from_buffer_copy(raw[:C.sizeof(_lib.ExtendInfoStruct)]))


def _count(a) -> int:
    return int(a.numel()) if _lib.is_torch(a) else int(a.size)


def extend_normal_velocity(phi: Function, interface_speed, *, normal_sign: float = 1.0, max_iter: int = 1000,
                           tol: float = 1e-10, max_distance: float | None = None, check_every: int = 8, info_out=None):
    """Carry a speed given on the zero contour of the P1 level set `phi` to the whole background mesh along the normals
    (cutfemx.distance.extend_normal_velocity, python/cutfemx/distance.py:176-240), in HBM (cfx_extend_normal_velocity).

    `interface_speed` is a Function on phi's space, or an array of one value per vertex: a P1 function w whose trace on
    the zero contour is the speed (this engine has no interface mesh; a speed computed from a solution lives on the
    background mesh anyway).  `phi` is not changed.  Returns a NormalExtensionResult: speed F (constant along the
    normals of the distance field), velocity F n with n = normal_sign x the unit gradient of phi carried the same way,
    and the signed distance -- bit for bit what `reinitialize` with the same `max_iter`, `tol`, `max_distance` and
    `check_every` writes into a copy of phi.  numpy values give numpy results, device tensors device tensors.  Beyond
    `max_distance` the speed and the velocity are 0.  Without an interface the results are zero-filled arrays that the
    call did not touch, and info.reason is REINIT_NO_INTERFACE.  `info_out` (extend_info_buffer()): the info stays in
    HBM; with device values and check_every = 0 the call makes no host round trip."""
    V = phi.function_space
    if V.degree != 1:
        raise ValueError("extend_normal_velocity: the space of phi must have degree 1")
    if V.bs != 1:
        raise ValueError("extend_normal_velocity: the space of phi must be scalar (block size 1)")
    nv, gdim = V.ndofs, V.mesh.gdim
    w = interface_speed.values if isinstance(interface_speed, Function) else interface_speed
    if isinstance(interface_speed, Function) and interface_speed.function_space is not V:
        raise ValueError("extend_normal_velocity: interface_speed must live on the space of phi")
    vals = phi.values
    if _count(vals) != nv:
        raise ValueError(f"extend_normal_velocity: phi.values must hold {nv} values")
    if _count(w) != nv:
        raise ValueError(f"extend_normal_velocity: interface_speed must hold {nv} values, one per vertex")
    if info_out is not None and not _lib.is_device(info_out):
        raise TypeError("extend_normal_velocity: info_out is a device buffer (extend_info_buffer())")
    on_device = _lib.is_device(vals)
    if on_device != _lib.is_device(w):
        raise TypeError("extend_normal_velocity: phi.values and interface_speed must both be host or both be device arrays")
    o = _lib.ExtendOptions()
    _lib.check(_lib.load().cfx_extend_options_default(C.byref(o)))
    o.max_iter, o.tol, o.check_every, o.normal_sign = int(max_iter), float(tol), int(check_every), float(normal_sign)
    o.max_distance = 0.0 if max_distance is None else float(max_distance)
    keep: list = []
    if on_device and _lib.is_torch(vals):
        import torch
        make = lambda n: torch.zeros(n, dtype=torch.float64, device=vals.device)
    elif on_device:
        def make(n):
            buf = _lib.DeviceBuffer(n, np.float64)
            _lib.check(_lib.lib().cfx_device_memset(C.c_void_p(buf.ptr), 0, C.c_size_t(8 * n)))
            return buf
    else:
        make = lambda n: np.zeros(n, dtype=np.float64)
    speed, velocity, dist = make(nv), make(nv * gdim), make(nv)
    ptr = lambda a: _lib.as_ptr(a, np.float64, keep)
    fn = _lib.lib().cfx_extend_normal_velocity
    st = None if info_out is not None else _lib.ExtendInfoStruct()
    info_ptr = ptr(info_out) if info_out is not None else C.byref(st)
    _lib.check(fn(V._h, ptr(vals), ptr(w), ptr(speed), ptr(velocity), ptr(dist), C.byref(o), info_ptr))
    from .mesh import FunctionSpace
    if getattr(V, "_vector_space", None) is None:
        V._vector_space = FunctionSpace(V.mesh, 1, bs=gdim)
    return NormalExtensionResult(Function(V, values=speed, name="speed"), Function(V._vector_space, values=velocity, name="velocity"),
                                 Function(V, values=dist, name="signed_distance"),
                                 info_out if info_out is not None else _extend_info(st))


@dataclass
class AdvectInfo:
    """cfx_advect_info: the vertices whose departure point was found in a cell (fixed dofs included), those whose walk
    left the mesh, those that hit the step limit or had a non-finite target (unchanged), those beyond the band
    (unchanged); the facet crossings of all walks and the most crossings of one vertex."""
    located: int
    outside: int
    capped: int
    skipped: int
    steps: int
    max_walk: int


def advect_info_buffer():
    """A device buffer for `advect(..., info_out=)`: 48 bytes that hold a cfx_advect_info; read with read_advect_info."""
    return _lib.DeviceBuffer(6, np.float64)


def _advect_info(st) -> AdvectInfo:
    return AdvectInfo(int(st.located), int(st.outside), int(st.capped), int(st.skipped), int(st.steps), int(st.max_walk))


def read_advect_info(info_out) -> AdvectInfo:
    """The AdvectInfo an advect call left in `info_out` (one copy to the host)."""
    raw = (info_out.numpy() if isinstance(info_out, _lib.DeviceBuffer) else info_out.cpu().numpy()).tobytes()
    return _advect_info(_lib.AdvectInfoStruct.from_buffer_copy(raw[:C.sizeof(_lib.AdvectInfoStruct)]))


def advect(phi: Function, velocity, dt: float, *, order: int = 2, max_distance: float | None = None, max_steps: int = 4096,
           cells_out=None, info_out=None):
    """Move the P1 level set `phi` along `velocity` over the time `dt` by semi-Lagrangian characteristics, in place on
    `phi.values`, in HBM (cfx_advect_level_set; _advect_level_set_characteristics of the reference's
    demo_compliance_optimization.py).  Returns an AdvectInfo.

    `phi` lives on a scalar degree-1 space on the geometry dofmap.  `velocity` is a Function on a degree-1 space with
    bs = gdim on the same mesh -- the `velocity` of a NormalExtensionResult goes in as it stands -- or an array of
    nv * gdim values, the gdim components of a vertex in a row.  Every vertex takes the old phi at its departure point
    x - dt v_mid (`order` 2: v_mid the velocity at x - dt/2 v; `order` 1: its own velocity), found by a walk through the
    cells; a point outside the mesh takes the P1 extension of the boundary cell the walk left through.  `max_distance`
    = B: vertices with |phi| > B keep their value -- the caller owes dt max|velocity| < B (reinitialize clamps to
    exactly its band: a B a hair below that one skips the clamped vertices).  `max_steps`: a walk of more
    crossings leaves its vertex unchanged and counts it as capped.  `cells_out`: an int32 array of nv entries that
    receives the final cell of every vertex (-1: skipped or capped).  numpy values stay numpy, device tensors stay in
    HBM; mixing the two raises TypeError.  `info_out` (advect_info_buffer()): the info stays in HBM and is returned as it
    stands; with device arrays the call then makes no host round trip."""
    V = phi.function_space
    if V.degree != 1:
        raise ValueError("advect: the space of phi must have degree 1")
    if V.bs != 1:
        raise ValueError("advect: the space of phi must be scalar (block size 1)")
    nv, gdim = V.ndofs, V.mesh.gdim
    if isinstance(velocity, Function):
        W = velocity.function_space
        if W.mesh is not V.mesh or W.degree != 1 or W.bs != gdim:
            raise ValueError("advect: velocity must live on a degree-1 space with bs = gdim on the mesh of phi")
        vel = velocity.values
    else:
        vel = velocity
    vals = phi.values
    on_device = _lib.is_device(vals)
    if on_device != _lib.is_device(vel) or (cells_out is not None and on_device != _lib.is_device(cells_out)):
        raise TypeError("advect: phi.values, velocity and cells_out must all be host or all be device arrays")
    if info_out is not None and not _lib.is_device(info_out):
        raise TypeError("advect: info_out is a device buffer (advect_info_buffer())")
    keep: list = []
    if on_device:
        if _lib.is_torch(vals):
            import torch
            if vals.dtype != torch.float64 or not vals.is_contiguous():
                raise TypeError("phi.values must be a contiguous float64 tensor (it is overwritten in place)")
        pp = _lib.as_ptr(vals, np.float64, keep)
    else:
        if not (isinstance(vals, np.ndarray) and vals.dtype == np.float64 and vals.flags.c_contiguous):
            vals = phi.values = np.ascontiguousarray(vals, dtype=np.float64)
        pp = vals.ctypes.data_as(C.c_void_p)
    if _count(vals) != nv:
        raise ValueError(f"advect: phi.values must hold {nv} values")
    if _count(vel) != nv * gdim:
        raise ValueError(f"advect: velocity must hold {nv * gdim} values, {gdim} per vertex")
    cp = None
    if cells_out is not None:
        if _count(cells_out) != nv:
            raise ValueError(f"advect: cells_out must hold {nv} entries")
        if _lib.is_torch(cells_out):
            import torch
            ok = cells_out.dtype == torch.int32 and cells_out.is_contiguous()
        elif isinstance(cells_out, _lib.DeviceBuffer):
            ok = cells_out.dtype == np.dtype(np.int32)
        else:
            ok = isinstance(cells_out, np.ndarray) and cells_out.dtype == np.int32 and cells_out.flags.c_contiguous
        if not ok:
            raise TypeError("advect: cells_out must be a contiguous int32 array (it is written in place)")
        cp = _lib.as_ptr(cells_out, np.int32, keep)
    o = _lib.AdvectOptions()
    _lib.check(_lib.load().cfx_advect_options_default(C.byref(o)))
    o.dt, o.order, o.max_steps = float(dt), int(order), int(max_steps)
    o.max_distance = 0.0 if max_distance is None else float(max_distance)
    fn = _lib.lib().cfx_advect_level_set
    vp = _lib.as_ptr(vel, np.float64, keep)
    if info_out is not None:
        _lib.check(fn(V._h, pp, vp, pp, cp, C.byref(o), _lib.as_ptr(info_out, np.float64, keep)))
        return info_out
    st = _lib.AdvectInfoStruct()
    _lib.check(fn(V._h, pp, vp, pp, cp, C.byref(o), C.byref(st)))
    return _advect_info(st)


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
