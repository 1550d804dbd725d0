"""form / create_matrix / assemble_matrix / assemble_vector / active_domain /
deactivate_outside: the Python surface of python/cutfemx/fem.py backed by the
HIP engine.

The reference compiles UFL forms to JIT kernels (runintgen/FFCx); a GPU engine
cannot call a CPU function pointer per entity, so a form here is a list of
`Integral` descriptors -- an integrand id + parameters + the same integration
domain data the reference puts in `ufl.Measure(subdomain_data=...)`:

    dx(subdomain_data=[inside_cells, rules]) -> Integral(..., cells=inside_cells, rules=rules)
    dx(subdomain_data=interface_rules)       -> Integral(..., rules=interface_rules, point_data=normals)
    dS(subdomain_data=ghost_facets)          -> Integral(..., facets=ghost_facets)
    dS(subdomain_data=[facets, facet_rules]) -> Integral(..., facets=facets, rules=facet_rules)   (rules hosted by interior facets)
    ds(subdomain_data=[facets, facet_rules]) -> Integral(..., rules=full_facet_rules(...).to_cells()), Integral(..., rules=facet_rules.to_cells())
"""
from __future__ import annotations

import ctypes as C
from dataclasses import dataclass, field

import numpy as np

from . import _lib

_C128, _C64 = np.dtype(np.complex128), np.dtype(np.complex64)


def _is_complex(dt) -> bool:
    return dt is not None and np.dtype(dt) in (_C128, _C64)


def _cfn(name: str, dt):
    """the complex entry point of `name` for the scalar type dt: cfx_<name>_c128 or cfx_<name>_c64"""
    return getattr(_lib.lib(), f"cfx_{name}_{'c64' if np.dtype(dt) == _C64 else 'c128'}")

from .cut import FacetRows, RuntimeQuadratureRules
from .mesh import FunctionSpace

MASS, STIFFNESS, NITSCHE, GHOST_GRADJUMP, ELASTICITY = (_lib.K_MASS, _lib.K_STIFFNESS, _lib.K_NITSCHE,
                                                        _lib.K_GHOST_GRADJUMP, _lib.K_ELASTICITY)
EXTENSION_L2 = _lib.K_EXTENSION_L2
JUMP = _lib.K_JUMP
SIP = _lib.K_SIP
SOURCE, NITSCHE_RHS = _lib.L_SOURCE, _lib.L_NITSCHE_RHS
M_FIELD, M_L2_DIFF, M_H1_SEMI = _lib.M_FIELD, _lib.M_L2_DIFF, _lib.M_H1_SEMI   # functionals (rank 0, assemble_scalar)
DIV_TEST, DIV_TRIAL = _lib.K_DIV_TEST, _lib.K_DIV_TRIAL   # rectangular blocks: scale div(v) p / scale q div(u)
F_ONE, F_SINPROD, F_POISSON_RHS, F_COEFFICIENT = _lib.F_ONE, _lib.F_SINPROD, _lib.F_POISSON_RHS, _lib.F_COEFFICIENT


@dataclass
class Integral:
    """One integral of a form (the per-integral tuple of python/cutfemx/fem.py:346-351)."""
    kernel: int
    cells: object = None                      # standard (uncut) cells: ids, numpy/torch/(ptr, n)
    rules: RuntimeQuadratureRules | None = None  # runtime quadrature on the cut cells
    facets: FacetRows | np.ndarray | None = None  # interior facets (c0,lf0,c1,lf1)
    point_data: object = None                 # per-point coefficients aligned with `rules`
    params: tuple = ()
    qdegree: int = 2                          # quadrature degree on the standard entities
    coefficient: object = None                # Function / dof values of the form's space (field id F_COEFFICIENT)
    coefficients: tuple = ()                  # registered integrands: Functions packed into `w` in this order, each on its
                                              # own space (Form::coefficients(), pack_form.h:69-158); not with `coefficient`
    scale: complex = 1.0                      # constant that multiplies the integrand (fem.Constant kappa in `kappa * ... * dx`,
                                              # test_complex_assembly.py:55-91): a complex value makes the form complex128
    _keep: list = field(default_factory=list, repr=False)

    def __post_init__(self):
        self.coefficients = tuple(self.coefficients)
        if self.coefficient is not None and len(self.coefficients) > 0:
            raise ValueError("Integral: give either `coefficient` (one Function of the form's space) or `coefficients` "
                             "(a list, each Function on its own space), not both")

    def _coefficient_values(self):
        c = self.coefficient
        if c is None or _lib.is_torch(c):   # (a torch tensor has a `values` METHOD: dof values in HBM are taken as they are)
            return c
        return getattr(c, "values", c)

    def _complex_coefficient(self) -> bool:
        v = self._coefficient_values()
        if v is None or _lib.is_torch(v) or isinstance(v, _lib.DeviceBuffer):   # (dof values in HBM are real)
            return False
        return np.iscomplexobj(v)

    def _cstruct(self, part: str = "re") -> _lib.Integral:
        keep = []
        if part == "re":
            self._keep = keep          # what the form of the real parts aliases lives as long as this descriptor ...
        else:
            self._keep_im = keep       # ... and so does what the form of the imaginary parts aliases
        itype = _lib.CELL
        ent_ptr, n_ent = None, 0
        if self.facets is None and self.rules is not None and self.rules.host_width == 4 and (
                self.kernel in (_lib.K_GHOST_GRADJUMP, _lib.K_JUMP, _lib.K_SIP) or self.kernel in _user_integrand_facet):
            itype = _lib.INTERIOR_FACET       # dS over runtime rules only
        if self.facets is not None:
            itype = _lib.INTERIOR_FACET
            if isinstance(self.facets, FacetRows):
                ent_ptr, n_ent = C.c_void_p(self.facets.ptr), self.facets.size
                keep.append(self.facets)
            elif _lib.is_torch(self.facets):  # (nf, 4) int32 tensor, host or device
                ent_ptr, n_ent = _lib.as_ptr(self.facets, np.int32, keep), int(self.facets.numel() // 4)
            else:
                rows = np.ascontiguousarray(self.facets, dtype=np.int32).reshape(-1, 4)
                ent_ptr, n_ent = _lib.as_ptr(rows, np.int32, keep), rows.shape[0]
        elif self.cells is not None:
            if isinstance(self.cells, tuple):  # (device pointer, count)
                ent_ptr, n_ent = C.c_void_p(self.cells[0]), int(self.cells[1])
                keep.append(self.cells)       # a DeviceEntities tuple pins the CutData that owns the list
            else:
                ent_ptr = _lib.as_ptr(self.cells, np.int32, keep)
                n_ent = int(keep[-1].numel() if _lib.is_torch(keep[-1]) else keep[-1].size)
        pd, stride = None, 0
        if self.point_data is not None:
            pdata = self.point_data
            stride = 1 if pdata.ndim == 1 else int(pdata.shape[1])
            pd = _f64_ptr(pdata, keep)
        params = (C.c_double * 8)(*([float(v) for v in self.params] + [0.0] * (8 - len(self.params))))
        coeff = None
        if self.coefficient is not None:
            values = self._coefficient_values()   # a Function or its dof array
            if self._complex_coefficient():       # complex Function: its real / imaginary parts feed two real forms
                values = np.ascontiguousarray(np.real(values) if part == "re" else np.imag(values), dtype=np.float64)
            coeff = _f64_ptr(values, keep)
        return _lib.Integral(itype, self.kernel, int(self.qdegree), stride, ent_ptr, n_ent,
                             self.rules._h if self.rules is not None else None, pd, params, coeff)


class _Widened:
    """fp64 HBM copy of a float32 device array (cfx_widen_f32), released with the integral that holds it."""

    def __init__(self, ptr, n):
        p = C.c_void_p()
        _lib.check(_lib.lib().cfx_widen_f32(C.c_void_p(ptr), C.c_int64(n), C.byref(p)))
        self.ptr = p.value

    def __del__(self):
        try:
            if self.ptr:
                _lib.load().cfx_device_free(C.c_void_p(self.ptr))
                self.ptr = None
        except Exception:
            pass


def _f64_ptr(a, keep: list):
    """Per-point data / coefficient values for a cfx_integral: float32 device arrays are widened in HBM."""
    if _lib.scalar_dtype(a) == np.float32 and _lib.is_device(a):
        n = a.size if isinstance(a, _lib.DeviceBuffer) else int(a.numel())
        w = _Widened(a.ptr if isinstance(a, _lib.DeviceBuffer) else a.contiguous().data_ptr(), n)
        keep.append(w)
        return C.c_void_p(w.ptr)
    return _lib.as_ptr(a, np.float64, keep)


def _coefficient_list(functions, keep: list):
    """(n, cfx_coefficient array) of an ordered list of Functions; what the array points to is appended to `keep`."""
    functions = tuple(functions)
    for f in functions:
        if not hasattr(f, "function_space") or not hasattr(f, "values"):
            raise TypeError("coefficients: a list of Functions (each with its function_space and values)")
        v = f.values
        if v.is_complex() if _lib.is_torch(v) else _is_complex(v.dtype) if isinstance(v, _lib.DeviceBuffer) else np.iscomplexobj(v):
            raise ValueError("coefficients: complex Functions in a coefficient list are not supported (the Functions of a "
                             "list are real; a complex constant goes into Integral.scale)")
    arr = (_lib.Coefficient * max(len(functions), 1))()
    for k, f in enumerate(functions):
        W = f.function_space
        v = f.values
        n = v.size if isinstance(v, _lib.DeviceBuffer) else int(v.numel()) if _lib.is_torch(v) else np.asarray(v).size
        if n != W.ndofs * W.bs:
            raise ValueError(f"coefficients[{k}]: {n} values for a space of {W.ndofs} dofs x block size {W.bs}")
        arr[k].space = W._h.value
        arr[k].values = _f64_ptr(f.values, keep).value
        keep.append(W)
    return len(functions), arr


class CutForm:
    """Compiled form handle (python/cutfemx/fem.py CutForm)."""

    def __init__(self, V: FunctionSpace, integrals, rank: int, trial_space: FunctionSpace | None = None, dtype=None):
        self.function_space, self.rank = V, rank
        # Form::function_spaces() = [test, trial] (Form.h:119-178): the same space twice unless `trial_space` is given
        self.trial_space = V if trial_space is None else trial_space
        self.integrals = list(integrals)
        # scalar type T of the form (cutfemx.fem.form(..., dtype=), wrappers/fem.cpp:490-500): complex128 when asked for,
        # or when a constant / coefficient of an integral is complex; real forms with unit constants stay on the
        # float64 entry points
        cplx = any(isinstance(i.scale, complex) and i.scale.imag != 0.0 for i in self.integrals) \
            or any(i._complex_coefficient() for i in self.integrals)
        if dtype is not None and np.dtype(dtype) not in (np.dtype(np.float64), np.dtype(np.float32), _C128, _C64):
            raise TypeError("forms are float64 (float32 containers), complex128 or complex64")
        if cplx and dtype is not None and not _is_complex(dtype):
            raise TypeError("a complex constant or coefficient needs dtype=complex128 (or complex64)")
        # (complex64: the containers the form assembles into are interleaved float32; the form itself is the same)
        self.dtype = np.dtype(dtype) if _is_complex(dtype) else (_C128 if cplx else np.dtype(np.float64))
        self._scaled = any(complex(i.scale) != 1.0 for i in self.integrals)
        if self._scaled and not _is_complex(self.dtype):
            raise TypeError("Integral.scale belongs to complex forms (fold a real constant into `params`)")
        self._h_im = None

        if self.trial_space is not V:
            # a registered two-space integrand packs its coefficient with the TEST space's dofmap
            for i in self.integrals:
                cs = getattr(i.coefficient, "function_space", None)
                if i.kernel in _user_integrand_two and cs is not None and cs is not V:
                    raise ValueError("cfx_form_create2: the coefficient of a registered two-space integrand must be a "
                                     "Function of the test space (it is packed with the test space's dofmap)")

        def create(part):
            # (the arrays an Integral hands over live until its next _cstruct call: each form is created -- and its host
            # arrays uploaded -- before the next one is described)
            arr = (_lib.Integral * len(self.integrals))(*[i._cstruct(part) for i in self.integrals])
            h = C.c_void_p()
            if self.trial_space is not V:
                if rank != 2:
                    raise ValueError("a trial space goes with a bilinear form")
                _lib.check(_lib.lib().cfx_form_create2(V._h, self.trial_space._h, len(self.integrals), arr, C.byref(h)))
            else:
                _lib.check(_lib.lib().cfx_form_create(V._h, rank, len(self.integrals), arr, C.byref(h)))
            return h
        self._h = None
        self._h = create("re")
        if any(i._complex_coefficient() for i in self.integrals):
            # the imaginary parts of the complex coefficients: a second real form, assembled with the constants i s_k
            # for the integrals that carry one and 0 for the others
            self._h_im = create("im")
        self._coefficient_keep: dict = {}
        for k, i in enumerate(self.integrals):
            if len(tuple(i.coefficients)) > 0:
                self.set_coefficients(k, i.coefficients)

    def set_coefficients(self, integral_index: int, functions) -> None:
        """Attach the ordered list of Functions `functions` to integral `integral_index` of this live form
        (cfx_form_set_coefficients): new values or a new list, without a new form or row plan and without a host
        read-back.  Host values are copied now, device values are aliased until they are replaced; an empty list returns
        the integral to what it was created with.  The integrand reads Function k at `w + CFX_W_OFF<k>`."""
        keep: list = []
        n, arr = _coefficient_list(functions, keep)
        handles = [self._h] + ([self._h_im] if self._h_im is not None else [])
        for h in handles:   # (the form of the imaginary parts of a complex `coefficient` shares the real list)
            _lib.check(_lib.lib().cfx_form_set_coefficients(h, int(integral_index), n, arr))
        self._coefficient_keep[int(integral_index)] = keep   # (the previous list's arrays are released after the swap)

    def _parts(self):
        """(form handle, interleaved complex constants) of the real forms that make up this complex128 form."""
        n = len(self.integrals)
        s = np.array([complex(i.scale) for i in self.integrals])
        out = [(self._h, (C.c_double * (2 * n))(*np.column_stack([s.real, s.imag]).ravel()))]
        if self._h_im is not None:
            t = np.array([1j * complex(i.scale) if i._complex_coefficient() else 0.0 for i in self.integrals])
            out.append((self._h_im, (C.c_double * (2 * n))(*np.column_stack([t.real, t.imag]).ravel())))
        return out

    def prepare(self):
        """Build the form's derived tables now (cfx_form_prepare) instead of inside the first assembly call."""
        _lib.check(_lib.lib().cfx_form_prepare(self._h))
        return self

    def lattice_tile_lists(self):
        """Diagnostics (cfx_form_lattice_tile_lists): None, or the plan's plain rows, their template flags and the
        filtered tile list as a dict of numpy arrays (plain_rows, templ, tile_first, tile_id)."""
        n, t = C.c_int64(0), C.c_int64(-1)
        f = _lib.lib().cfx_form_lattice_tile_lists
        _lib.check(f(self._h, C.byref(n), C.byref(t), None, None, None, None))
        if t.value < 0:
            return None
        rows, templ = np.zeros(max(n.value, 1), dtype=np.int32), np.zeros(max(n.value, 1), dtype=np.uint8)
        first, ids = np.zeros(max(t.value, 1), dtype=np.int32), np.zeros(max(t.value, 1), dtype=np.int32)
        ptr = lambda a: a.ctypes.data_as(C.c_void_p)
        _lib.check(f(self._h, C.byref(n), C.byref(t), ptr(rows), ptr(templ), ptr(first), ptr(ids)))
        return dict(plain_rows=rows[:n.value], templ=templ[:n.value], tile_first=first[:t.value], tile_id=ids[:t.value])

    def __del__(self):
        try:
            if self._h:
                _lib.load().cfx_form_destroy(self._h)
                self._h = None
            if getattr(self, "_h_im", None):
                _lib.load().cfx_form_destroy(self._h_im)
                self._h_im = None
        except Exception:
            pass


class overlap:
    """Two independent pieces of a step on two HIP streams (cfx_overlap_begin / _side / _end):

        L.prepare(); a.prepare()                 # shared tables are built before the lanes part
        with fem.overlap() as lanes:
            lanes.side(lambda: fem.assemble_vector(L, b))          # queued on the second stream
            A = fem.create_matrix(a); fem.assemble_matrix(a, A=A)  # meanwhile on the main stream
        # joined here

    The reference assembles a and L one after the other (python/demo/demo_poisson.py:40-60); they share inputs only."""

    def __enter__(self):
        _lib.check(_lib.lib().cfx_overlap_begin())
        return self

    def side(self, fn):
        _lib.check(_lib.lib().cfx_overlap_side(1))
        try:
            return fn()
        finally:
            _lib.check(_lib.lib().cfx_overlap_side(0))

    def __exit__(self, *exc):
        _lib.check(_lib.lib().cfx_overlap_end())
        return False


_user_integrand_rank: dict[int, int] = {}
_user_integrand_two: set[int] = set()   # ids of cfx_integrand_register2
_user_integrand_facet: set[int] = set()  # ids of rank-0 interior-facet integrands (dS over facet-hosted rules alone)


def _coefficient_signature(coefficients):
    sig = [(int(c[0]), int(c[1]) if len(c) > 1 else 1) for c in coefficients]
    nd = (C.c_int * max(len(sig), 1))(*[c[0] for c in sig])
    bs = (C.c_int * max(len(sig), 1))(*[c[1] for c in sig])
    return sig, nd, bs


def _coefficient_defaults(sig) -> str:
    """The CFX_W_* macros of the signature as defaults: the text a source is validated with where no list is compiled in."""
    lines, off = ["#ifndef CFX_NCOEF", f"#define CFX_NCOEF {len(sig)}",
                  f"#define CFX_CSTRIDE {sum(n * b for n, b in sig)}"], 0
    for k, (n, b) in enumerate(sig):
        lines += [f"#define CFX_W_ND{k} {n}", f"#define CFX_W_BS{k} {b}", f"#define CFX_W_OFF{k} {off}"]
        off += n * b
    return "\n".join(lines + ["#endif", ""])


def register_integrand(name: str, source: str, rank: int = 2, facet: bool = False, variant=None, trial=None,
                       coefficients=None) -> int:
    """Register the HIP C++ source of an integrand; returns the id to put into `Integral.kernel`.

    The reference generates a tabulate_tensor kernel per form at run time (runintgen / FFCx,
    python/cutfemx/_runintgen_adapter.py:181-217) and calls it per entity on the CPU; here the SOURCE of a device function

        __device__ void name(double* A, const double* w, const double* c, const double* coordinate_dofs,
                             int nq, const double* points, const double* weights, const double* point_data)

    (local tensor, packed coefficient, constants = Integral.params, vertex coordinates [(tdim+1)][3], the entity's
    rule: reference points, physical-measure weights, per-point data) is compiled for gfx950 with hipRTC -- see
    include/cutfemx_amd.h (cfx_integrand_register) for the contract and the helpers in scope (cfx_tabulate, ...).
    Cell integrals of Lagrange spaces of degree 1 or 2 (scalar or vector-valued: CFX_BS, CFX_NDB), over standard entities
    and / or runtime rules.  `facet=True`: an interior-facet integrand

        __device__ void name(double* A, const double* w, const double* c, const double* coordinate_dofs,
                             const int* entity_local_index, int nq, const double* points0, const double* points1,
                             const double* weights)

    over (c0, lf0, c1, lf1) rows -- macro tensor [[00, 01], [10, 11]], both cells' coordinate_dofs, {lf0, lf1}
    (assemble_matrix_impl.h:528-542).  `rank=0`: the integrand of a functional (assemble_scalar) -- the same argument
    lists, `A` is `double A[1]`, zero on entry, and the integrand adds its entity's value; with `facet=True` a rank-0
    interior-facet integrand.  `variant=(tdim, dofs per cell[, bs])`: the variant the source is validated
    against at registration (default (3, 4, 1)).

    A bilinear integrand between two spaces (the off-diagonal blocks of `MixedSpace`, forms with a `trial_space`):
    `variant=(tdim, nd0, bs0, nd1, bs1)`, or `variant=(tdim, nd0[, bs0])` with `trial=(nd1[, bs1])`
    (cfx_integrand_register2).  Its tensor is [NDB0][NDB1] (cells) or [2 NDB0][2 NDB1] (interior facets), with
    CFX_ND0 / CFX_BS0 / CFX_NDB0, CFX_ND1 / CFX_BS1 / CFX_NDB1 and cfx_tabulate0 / cfx_tabulate1 in scope.

    `coefficients=[(nd_0, bs_0), (nd_1, bs_1), ...]`: the integrand reads a coefficient LIST (`Integral.coefficients`:
    Functions on their own spaces, Function k with nd_k dofs per cell and bs_k components packed at `w + CFX_W_OFF<k>`;
    interior facets: cell 0 at `w + 2 * CFX_W_OFF<k>`, cell 1 directly after it).  The variant with this list is compiled
    at registration -- CFX_NCOEF, CFX_CSTRIDE, CFX_W_ND<k>, CFX_W_BS<k>, CFX_W_OFF<k> defined -- so the source is validated
    against the signature without a GPU; a list of other shapes is then refused until `compile_integrand(...,
    coefficients=...)` compiles its variant.  `w` holds at most 64 doubles."""
    if coefficients is not None and len(coefficients) > 0:
        sig, _, _ = _coefficient_signature(coefficients)
        if variant is None:
            variant = (3, 4, 1)
        # the list's macros as defaults, so that the source also compiles where no list is attached
        kid = register_integrand(name, _coefficient_defaults(sig) + source, rank, facet, variant, trial)
        if kid in _user_integrand_two:
            v = list(variant) + ([1] if len(variant) < 3 else [])
            t = v[3:5] if len(v) >= 5 else (list(trial) + [1])[:2]
            compile_integrand2(kid, v[0], v[1], v[2], t[0], t[1], coefficients=sig)
        else:
            tdim, nd, bs = (list(variant) + [1])[:3]
            compile_integrand(kid, tdim, nd, bs, coefficients=sig)
        return kid
    kid = C.c_int()
    two = trial is not None or (variant is not None and len(variant) == 5)
    if two:
        if rank != 2:
            raise ValueError("register_integrand: an integrand between two spaces is bilinear")
        if variant is None:
            raise ValueError("register_integrand: `trial` goes with `variant=(tdim, nd0[, bs0])`")
        if trial is not None:
            if len(variant) > 3:
                raise ValueError("register_integrand: give the trial space either in `variant` or in `trial`")
            tdim, nd0, bs0 = (list(variant) + [1])[:3]
            nd1, bs1 = (list(trial) + [1])[:2]
        else:
            tdim, nd0, bs0, nd1, bs1 = variant
        _lib.check(_lib.load().cfx_integrand_register2(name.encode(), source.encode(), int(bool(facet)), int(tdim), int(nd0),
                                                       int(bs0), int(nd1), int(bs1), C.byref(kid)))
        _user_integrand_rank[kid.value] = 2
        _user_integrand_two.add(kid.value)
        return kid.value
    if rank not in (0, 1, 2):
        raise ValueError("register_integrand: rank must be 0, 1 or 2")
    if variant is None and facet and rank == 0:
        variant = (3, 4, 1)   # (cfx_integrand_register_facet itself stays bilinear)
    if variant is None and not facet:
        _lib.check(_lib.load().cfx_integrand_register(name.encode(), source.encode(), int(rank), C.byref(kid)))
    elif variant is None:
        _lib.check(_lib.load().cfx_integrand_register_facet(name.encode(), source.encode(), C.byref(kid)))
    else:
        tdim, nd, bs = (list(variant) + [1])[:3]
        _lib.check(_lib.load().cfx_integrand_register_variant(name.encode(), source.encode(), int(rank), int(bool(facet)),
                                                              int(tdim), int(nd), int(bs), C.byref(kid)))
    _user_integrand_rank[kid.value] = int(rank)
    if facet and rank == 0:
        _user_integrand_facet.add(kid.value)
    return kid.value


def compile_integrand(kernel_id: int, tdim: int, ndofs_cell: int, bs: int = 1, coefficients=None) -> None:
    """Compile the (tdim, dofs per cell, block size) variant of a registered integrand now instead of at its first use;
    `coefficients=[(nd, bs), ...]`: the variant with that coefficient list (cfx_integrand_compile_coefficients)."""
    if coefficients is not None and len(coefficients) > 0:
        sig, nd, cbs = _coefficient_signature(coefficients)
        _lib.check(_lib.load().cfx_integrand_compile_coefficients(int(kernel_id), int(tdim), int(ndofs_cell), int(bs), 0, 0,
                                                                  len(sig), nd, cbs))
        return
    _lib.check(_lib.load().cfx_integrand_compile_bs(int(kernel_id), int(tdim), int(ndofs_cell), int(bs)))


def compile_integrand2(kernel_id: int, tdim: int, nd0: int, bs0: int, nd1: int, bs1: int, coefficients=None) -> None:
    """Compile the (tdim, test nd0 / bs0, trial nd1 / bs1) variant of a two-space integrand now instead of at its first
    use (cfx_integrand_compile2); `coefficients=[(nd, bs), ...]`: the variant with that coefficient list."""
    if coefficients is not None and len(coefficients) > 0:
        sig, nd, cbs = _coefficient_signature(coefficients)
        _lib.check(_lib.load().cfx_integrand_compile_coefficients(int(kernel_id), int(tdim), int(nd0), int(bs0), int(nd1),
                                                                  int(bs1), len(sig), nd, cbs))
        return
    _lib.check(_lib.load().cfx_integrand_compile2(int(kernel_id), int(tdim), int(nd0), int(bs0), int(nd1), int(bs1)))


def form(integrals, V: FunctionSpace, rank: int | None = None, trial_space: FunctionSpace | None = None, dtype=None) -> CutForm:
    """Create a form from integral descriptors (stands in for cutfemx.fem.form).  `V` is the test space; a bilinear
    form whose trial space differs (the off-diagonal blocks of a Stokes system, test_assembly_stokes.py:34-95) names it
    with `trial_space`."""
    integrals = list(integrals)
    if rank is None:
        # built-in ids: below 100 bilinear, 100..199 linear, 200..299 functionals
        ranks = {_user_integrand_rank[i.kernel] if i.kernel in _user_integrand_rank
                 else (2 if i.kernel < 100 else 1 if i.kernel < 200 else 0) for i in integrals}
        if len(ranks) != 1:
            raise ValueError("all integrals of a form must have the same rank")
        rank = ranks.pop()
    return CutForm(V, integrals, rank, trial_space, dtype)


class MatrixCSR:
    """dolfinx.la.MatrixCSR stand-in: indptr (int64), indices (int32), data in HBM."""

    def __init__(self, pattern_handle, V: FunctionSpace, values=None, dtype=None):
        self._p = pattern_handle
        self.function_space = V
        # scalar type T of la::MatrixCSR<T> (wrappers/fem.cpp:490-500): float64, or float32 through the *_f32 entry points
        self.dtype = np.dtype(_lib.scalar_dtype(values) if dtype is None else dtype)
        if self.dtype not in (np.dtype(np.float32), np.dtype(np.float64), _C128, _C64):
            raise TypeError("MatrixCSR holds float64, float32, complex128 or complex64 values")
        v = _lib.PatternView()
        _lib.check(_lib.lib().cfx_pattern_view_get(self._p, C.byref(v)))
        self._view = v
        self.nrows, self.ncols = int(v.nrows), int(v.ncols)
        self._nnz_pending = _lib._step_open   # made inside a cutfemx_amd.step: nnz may still be in HBM
        self._nnz = int(v.nnz)
        self._owns_values = values is None
        self._zero_pending = False
        if values is None:
            p = C.c_void_p()
            _lib.check(_lib.lib().cfx_device_alloc(C.byref(p), C.c_size_t(self.dtype.itemsize * max(self.nnz, 1))))
            self._vptr = p.value
            self.set_value(0.0)
        else:  # caller-owned HBM buffer: set_value / cfx_assemble_matrix write 8*nnz bytes through the raw pointer
            if isinstance(values, _lib.DeviceBuffer):
                ok_type, count, ptr = values.dtype == self.dtype, values.size, values.ptr
            elif _lib.is_torch(values):
                import torch
                want = torch.float32 if self.dtype == np.dtype(np.float32) else torch.float64
                ok_type = values.dtype == want and values.is_cuda and values.is_contiguous()
                count, ptr = int(values.numel()), values.data_ptr()
            else:
                raise TypeError("values must be a device torch tensor or a DeviceBuffer")
            if not ok_type:
                raise TypeError(f"values must be a contiguous {self.dtype} buffer in HBM")
            if count < self.nnz:
                _lib.lib().cfx_pattern_destroy(self._p)
                self._p = None
                raise ValueError(f"values holds {count} entries but the sparsity pattern needs nnz = {self.nnz}")
            self._values_keep = values
            self._vptr = ptr

    @property
    def nnz(self) -> int:
        """Stored entries.  While the cutfemx_amd.step that made the matrix is open this is the capacity of the
        index / value arrays (the exact count is still in HBM); afterwards it is exact."""
        if self._nnz_pending:
            v = _lib.PatternView()
            _lib.check(_lib.lib().cfx_pattern_view_get(self._p, C.byref(v)))
            self._nnz = int(v.nnz)
            self._nnz_pending = _lib._step_open
        return self._nnz

    @property
    def reuse_stats(self) -> tuple[int, int]:
        """(rows of the pattern that needed a hash set, those of them copied from the space's previous pattern)."""
        h, r = C.c_int64(), C.c_int64()
        _lib.check(_lib.lib().cfx_pattern_reuse_stats(self._p, C.byref(h), C.byref(r)))
        return h.value, r.value

    @property
    def values_ptr(self):
        """HBM address of the value array; a pending set_value(0) is carried out first."""
        if self._zero_pending:
            self._zero_pending = False
            _lib.check(_lib.lib().cfx_device_memset(C.c_void_p(self._vptr), 0, C.c_size_t(self.dtype.itemsize * self.nnz)))
        return self._vptr

    @values_ptr.setter
    def values_ptr(self, p):
        self._vptr = p

    def set_value(self, v: float):
        """la::MatrixCSR::set_value.  Zeroing is deferred to the next use of the values: assemble_matrix then
        clears and assembles in one library call (cfx_assemble_matrix_zeroed)."""
        if complex(v) == 0.0:
            self._zero_pending = True
            return
        self._zero_pending = False
        z = np.full(self.nnz, v if _is_complex(self.dtype) else float(v), dtype=self.dtype)
        _lib.check(_lib.lib().cfx_copy(C.c_void_p(self._vptr), z.ctypes.data_as(C.c_void_p),
                                       C.c_size_t(z.nbytes)))

    def row_block(self, lo: int, hi: int):
        """(indptr - indptr[lo], indices, data) of rows lo..hi-1, downloading only those rows."""
        ip = _lib.download(self._view.indptr + 8 * lo, hi - lo + 1, np.int64)
        e0, e1 = int(ip[0]), int(ip[-1])
        ix = _lib.download(self._view.indices + 4 * e0, e1 - e0, np.int32)
        va = _lib.download(self.values_ptr + self.dtype.itemsize * e0, e1 - e0, self.dtype)
        return ip - e0, ix, va

    def torch_views(self, device):
        """Zero-copy torch tensors (indptr int64, indices int32, values f64) over the HBM arrays."""
        from .dist import as_torch
        return (as_torch(self._view.indptr, self.nrows + 1, "int64", device),
                as_torch(self._view.indices, self.nnz, "int32", device),
                as_torch(self.values_ptr, self.nnz, self.dtype.name, device))

    @property
    def indptr(self):
        return _lib.download(self._view.indptr, self.nrows + 1, np.int64)

    @property
    def indices(self):
        _lib.resolve_counts()
        return _lib.download(self._view.indices, self.nnz, np.int32)

    @property
    def data(self):
        _lib.resolve_counts()
        return _lib.download(self.values_ptr, self.nnz, self.dtype)

    def scatter_reverse(self):
        """Serial: nothing to reduce (multi-GPU reduction lives in cutfemx_amd.dist)."""

    def to_scipy(self):
        import scipy.sparse as sp
        return sp.csr_matrix((self.data, self.indices, self.indptr), shape=(self.nrows, self.ncols))

    def to_dense(self):
        return self.to_scipy().toarray()

    def __del__(self):
        try:
            l = _lib.load()
            if getattr(self, "_owns_values", False) and getattr(self, "_vptr", None):
                l.cfx_device_free(C.c_void_p(self._vptr))
                self._vptr = None
            if self._p:
                l.cfx_pattern_destroy(self._p)
                self._p = None
        except Exception:
            pass


def create_matrix(a: CutForm, values=None, dtype=None) -> MatrixCSR:
    """Sparsity of a bilinear form incl. the all-rows diagonal
    (python/cutfemx/fem.py:810-848 -> assembler.h:567-592).  dtype (or a float32 `values` buffer) selects the
    scalar type of the matrix: float64 (default) or float32."""
    p = C.c_void_p()
    _lib.check(_lib.lib().cfx_create_sparsity(a._h, C.byref(p)))
    if dtype is None and values is None and _is_complex(a.dtype):
        dtype = a.dtype
    return MatrixCSR(p, a.function_space, values, dtype)


def assemble_matrix(a: CutForm, bcs=None, A: MatrixCSR | None = None) -> MatrixCSR:
    """Assemble a bilinear form into CSR (python/cutfemx/fem.py:886-942).
    `bcs` is an int8 dof marker applied to rows and columns, or (bc0, bc1)."""
    if A is None:
        A = create_matrix(a)
    keep: list = []
    bc0 = bc1 = None
    if bcs is not None:
        b0, b1 = bcs if isinstance(bcs, tuple) else (bcs, bcs)
        bc0, bc1 = _lib.as_ptr(b0, np.int8, keep), _lib.as_ptr(b1, np.int8, keep)
    l = _lib.lib()
    if _is_complex(A.dtype):
        zero = 1 if A._zero_pending else 0
        A._zero_pending = False
        for h, scales in a._parts():
            _lib.check(_cfn("assemble_matrix", A.dtype)(h, A._p, bc0, bc1, scales, zero, C.c_void_p(A._vptr)))
            zero = 0
        return A
    if _is_complex(a.dtype):
        raise TypeError("a complex form assembles into a complex matrix (create_matrix(a) makes one)")
    f32 = A.dtype == np.dtype(np.float32)
    if A._zero_pending:     # A.set_value(0) + assemble_matrix(A, a, bcs) as one call
        A._zero_pending = False
        fn = l.cfx_assemble_matrix_zeroed_f32 if f32 else l.cfx_assemble_matrix_zeroed
    else:
        fn = l.cfx_assemble_matrix_f32 if f32 else l.cfx_assemble_matrix
    _lib.check(fn(a._h, A._p, bc0, bc1, C.c_void_p(A._vptr)))
    return A


def assemble_vector(L: CutForm, b=None, dtype=np.float64):
    """Assemble a linear form (python/cutfemx/fem.py:851-883).  Returns a numpy
    vector, or accumulates into `b` (numpy array or device torch tensor; float64 or float32)."""
    V = L.function_space
    if b is None:
        b = np.zeros(V.ndofs * V.bs, dtype=L.dtype if _is_complex(L.dtype) else dtype)
    if _is_complex(_lib.scalar_dtype(b)):
        for h, scales in L._parts():
            _lib.check(_cfn("assemble_vector", _lib.scalar_dtype(b))(h, scales, _vec_ptr(b)))
        return b
    if _is_complex(L.dtype):
        raise TypeError("a complex form assembles into a complex vector")
    fn = _lib.lib().cfx_assemble_vector_f32 if _lib.scalar_dtype(b) == np.float32 else _lib.lib().cfx_assemble_vector
    _lib.check(fn(L._h, _vec_ptr(b)))
    return b


def _vec_ptr(b):
    return C.c_void_p(b.data_ptr()) if _lib.is_torch(b) else b.ctypes.data_as(C.c_void_p)


def apply_lifting(b, a: CutForm, bc_markers, bc_values, x0=None, alpha: float = 1.0):
    """b <- b - alpha A (g - x0) over the Dirichlet columns, entity by entity
    (python/cutfemx/fem.py:604-632 -> lift_bc_impl, assemble_vector_impl.h:383-436).
    `bc_markers` (int8) / `bc_values` / `x0` hold one entry per dof; one bilinear form,
    i.e. one block of the reference's list-of-forms signature."""
    keep: list = []
    if _is_complex(a.dtype) and not _is_complex(_lib.scalar_dtype(b)):
        # (as assemble_matrix / assemble_vector: the real entry points would drop the constants and the imaginary part)
        raise TypeError("a complex form lifts into a complex vector")
    if _is_complex(_lib.scalar_dtype(b)):
        cdt = np.dtype(_lib.scalar_dtype(b))
        g = np.ascontiguousarray(bc_values, dtype=cdt)
        x = None if x0 is None else np.ascontiguousarray(x0, dtype=cdt)
        al = complex(alpha)
        for h, scales in a._parts():
            _lib.check(_cfn("apply_lifting", cdt)(
                h, _lib.as_ptr(bc_markers, np.int8, keep), g.ctypes.data_as(C.c_void_p),
                None if x is None else x.ctypes.data_as(C.c_void_p), C.c_double(al.real), C.c_double(al.imag), scales, _vec_ptr(b)))
        return b
    if _lib.scalar_dtype(b) == np.float32:
        _lib.check(_lib.lib().cfx_apply_lifting_f32(
            a._h, _lib.as_ptr(bc_markers, np.int8, keep), _lib.as_ptr(bc_values, np.float32, keep),
            _lib.as_ptr(x0, np.float32, keep), C.c_float(alpha), _vec_ptr(b)))
        return b
    _lib.check(_lib.lib().cfx_apply_lifting(
        a._h, _lib.as_ptr(bc_markers, np.int8, keep), _lib.as_ptr(bc_values, np.float64, keep),
        _lib.as_ptr(x0, np.float64, keep), C.c_double(alpha), _vec_ptr(b)))
    return b


def set_bc(b, bc_markers, bc_values, x0=None, alpha: float = 1.0):
    """b[dofs] = alpha (g - x0) on the marked dofs (dolfinx.fem.set_bc / DirichletBC.set)."""
    keep: list = []
    n = b.numel() if _lib.is_torch(b) else b.size
    if _is_complex(_lib.scalar_dtype(b)):
        cdt = np.dtype(_lib.scalar_dtype(b))
        g = np.ascontiguousarray(bc_values, dtype=cdt)
        x = None if x0 is None else np.ascontiguousarray(x0, dtype=cdt)
        al = complex(alpha)
        _lib.check(_cfn("set_bc", cdt)(C.c_int64(n), _lib.as_ptr(bc_markers, np.int8, keep), g.ctypes.data_as(C.c_void_p),
                                             None if x is None else x.ctypes.data_as(C.c_void_p), C.c_double(al.real),
                                             C.c_double(al.imag), _vec_ptr(b)))
        return b
    if _lib.scalar_dtype(b) == np.float32:
        _lib.check(_lib.lib().cfx_set_bc_f32(
            C.c_int64(n), _lib.as_ptr(bc_markers, np.int8, keep), _lib.as_ptr(bc_values, np.float32, keep),
            _lib.as_ptr(x0, np.float32, keep), C.c_float(alpha), _vec_ptr(b)))
        return b
    _lib.check(_lib.lib().cfx_set_bc(
        C.c_int64(n), _lib.as_ptr(bc_markers, np.int8, keep), _lib.as_ptr(bc_values, np.float64, keep),
        _lib.as_ptr(x0, np.float64, keep), C.c_double(alpha), _vec_ptr(b)))
    return b


def assemble_scalar(M: CutForm, out=None):
    """The functional of a form (python/cutfemx/fem.py:522-528 -> assemble_scalar_impl.h:26-275).

    A rank-0 form (M_FIELD / M_L2_DIFF / M_H1_SEMI or registered rank-0 integrands) is assembled in HBM
    (cfx_assemble_scalar) and returned as a float.  `out`: a one-element float64 device torch tensor that is overwritten
    with the value and returned instead -- no host read-back, also inside a cutfemx_amd.step.

    A linear form of SOURCE integrals keeps its older route: the Lagrange basis is a partition of unity, so the
    functional int f is the sum of the assembled vector (python/tests/test_cut_api.py:796-811 checks the reference the
    same way)."""
    if M.rank == 0 and not _is_complex(M.dtype):
        if out is not None:
            import torch
            if not (_lib.is_torch(out) and out.is_cuda and out.dtype == torch.float64 and out.numel() == 1
                    and out.is_contiguous()):
                raise TypeError("assemble_scalar: `out` is a one-element float64 device torch tensor")
            _lib.check(_lib.lib().cfx_assemble_scalar(M._h, C.c_void_p(out.data_ptr())))
            return out
        v = C.c_double()
        _lib.check(_lib.lib().cfx_assemble_scalar(M._h, C.byref(v)))
        return float(v.value)
    if M.rank != 1 or any(i.kernel != SOURCE for i in M.integrals):
        raise ValueError("assemble_scalar takes a rank-0 form (a functional: M_* or registered rank-0 integrands) or a "
                         "linear form made of SOURCE integrals (f dx)")
    if out is not None:
        raise ValueError("assemble_scalar: `out` goes with a rank-0 form")
    b = assemble_vector(M)
    return complex(b.sum()) if _is_complex(M.dtype) else float(b.sum())


# ---- the solve in HBM: y = A x, Jacobi-preconditioned CG and MINRES (cfx_csr_spmv / cfx_cg_solve / cfx_minres_solve) ----
PC_NONE, PC_JACOBI = _lib.PC_NONE, _lib.PC_JACOBI
PC_ABS_JACOBI, PC_ABS_ROWSUM = _lib.PC_ABS_JACOBI, _lib.PC_ABS_ROWSUM   # minres_solve alone
CG_CONVERGED, CG_MAX_ITER, CG_BREAKDOWN, CG_BAD_DIAGONAL = (_lib.CG_CONVERGED, _lib.CG_MAX_ITER, _lib.CG_BREAKDOWN,
                                                           _lib.CG_BAD_DIAGONAL)
_CG_REASONS = {CG_CONVERGED: "converged", CG_MAX_ITER: "max_iter", CG_BREAKDOWN: "breakdown",
               CG_BAD_DIAGONAL: "bad_diagonal"}


@dataclass
class CGInfo:
    """cfx_cg_info: why cg_solve stopped, after how many updates of x, |r|_2 of the recurrence and |b|_2 (both over
    the iterated rows).  minres_solve returns the same record with the two norms taken in the M^-1 norm of its rule."""
    reason: int
    iterations: int
    residual_norm: float
    rhs_norm: float

    @property
    def converged(self) -> bool:
        return self.reason == CG_CONVERGED

    @property
    def reason_name(self) -> str:
        return _CG_REASONS.get(self.reason, "running")


def cg_default_options() -> _lib.CGOptions:
    """The defaults of cfx_cg_options_default (no GPU needed)."""
    o = _lib.CGOptions()
    _lib.check(_lib.load().cfx_cg_options_default(C.byref(o)))
    return o


def cg_info_buffer():
    """A device buffer for `cg_solve(..., info_out=)`: 24 bytes that hold a cfx_cg_info; read with read_cg_info."""
    return _lib.DeviceBuffer(3, np.float64)


def read_cg_info(info_out) -> CGInfo:
    """The CGInfo a cg_solve call left in `info_out` (one copy to the host)."""
    raw = (info_out.numpy() if isinstance(info_out, _lib.DeviceBuffer) else info_out.cpu().numpy()).tobytes()
    st = _lib.CGInfoStruct.from_buffer_copy(raw[:C.sizeof(_lib.CGInfoStruct)])
    return CGInfo(int(st.reason), int(st.iterations), float(st.residual_norm), float(st.rhs_norm))


def _csr_arrays(A):
    """(nrows, indptr, indices, values) of a float64 MatrixCSR or MergedCSR: HBM addresses."""
    if np.dtype(A.dtype) != np.dtype(np.float64):
        raise TypeError("the solve takes float64 matrices (f32 and complex containers are out of scope)")
    if isinstance(A, MergedCSR):
        return A.nrows, A._indptr, A._indices, A._values
    return A.nrows, A._view.indptr, A._view.indices, A.values_ptr   # (addresses alone: no count is needed)


def _device_f64(a, n: int, what: str, keep: list):
    """HBM address of n float64 values: a device torch tensor / DeviceBuffer as it stands, a host array uploaded."""
    if _lib.is_device(a):
        if (a.numel() if _lib.is_torch(a) else a.size) < n:
            raise ValueError(f"{what} holds fewer than {n} values")
        if _lib.is_torch(a):
            import torch
            if a.dtype != torch.float64 or not a.is_contiguous():
                raise TypeError(f"{what} must be a contiguous float64 tensor")
            keep.append(a)
            return C.c_void_p(a.data_ptr())
        return _lib.as_ptr(a, np.float64, keep)
    h = np.ascontiguousarray(a, dtype=np.float64).ravel()
    if h.size < n:
        raise ValueError(f"{what} holds fewer than {n} values")
    d = _lib.DeviceBuffer(h.size, np.float64)
    d.fill_from(h)
    keep.append(d)
    return C.c_void_p(d.ptr)


def _row_list(rows, keep: list):
    """(device pointer, count) of an int32 row list: device torch tensor / DeviceBuffer, or a host array uploaded."""
    if rows is None:
        return None, 0
    if _lib.is_device(rows):
        n = int(rows.numel()) if _lib.is_torch(rows) else rows.size
        if _lib.is_torch(rows):
            import torch
            if rows.dtype != torch.int32 or not rows.is_contiguous():
                rows = rows.to(torch.int32).contiguous()
            keep.append(rows)
            return C.c_void_p(rows.data_ptr()), n
        return _lib.as_ptr(rows, np.int32, keep), n
    h = np.ascontiguousarray(rows, dtype=np.int32).ravel()
    d = _lib.DeviceBuffer(h.size, np.int32)
    d.fill_from(h)
    keep.append(d)
    return C.c_void_p(d.ptr), h.size


def csr_from_arrays(indptr, indices, values, ncols: int | None = None) -> "MergedCSR":
    """A caller's CSR matrix (host arrays: indptr, indices, float64 values) copied into HBM as a MergedCSR, for spmv and
    cg_solve.  ncols defaults to the number of rows."""
    ip = np.ascontiguousarray(indptr, dtype=np.int64)
    ix = np.ascontiguousarray(indices, dtype=np.int32)
    va = np.ascontiguousarray(values, dtype=np.float64)
    nrows, nnz = ip.size - 1, int(ip[-1]) if ip.size else 0
    if nrows < 0 or ix.size < nnz or va.size < nnz:
        raise ValueError("csr_from_arrays: indptr needs nrows + 1 entries, indices and values indptr[-1] entries")
    ncols = nrows if ncols is None else int(ncols)
    if nnz and (ix[:nnz].min() < 0 or ix[:nnz].max() >= ncols):
        raise ValueError("csr_from_arrays: a column index lies outside [0, ncols)")
    l, ptrs = _lib.lib(), []
    for h in (ip, ix, va):
        p = C.c_void_p()
        _lib.check(l.cfx_device_alloc(C.byref(p), C.c_size_t(max(h.nbytes, 8))))
        if h.nbytes:
            _lib.check(l.cfx_copy(p, h.ctypes.data_as(C.c_void_p), C.c_size_t(h.nbytes)))
        ptrs.append(p.value)
    return MergedCSR(ptrs[0], ptrs[1], ptrs[2], nnz, nrows, ncols, np.zeros(1, dtype=np.int64), np.zeros(1, dtype=np.int64))


def active_rows(domain: "ActiveDomain"):
    """The rows of the active dofs of `domain` as an int32 device torch tensor, ascending: the complement of the
    domain's inactive-dof list, formed on the device."""
    import torch
    from .dist import as_torch
    V = domain.function_space
    _lib.resolve_counts()
    _, _, idf, ni = domain._view()
    dev = torch.device("cuda", torch.cuda.current_device())
    mask = torch.ones(V.ndofs * V.bs, dtype=torch.bool, device=dev)
    if ni > 0:
        mask[as_torch(idf, ni, "int32", dev).long()] = False
    return torch.nonzero(mask).reshape(-1).to(torch.int32)


def spmv(A, x, out=None, rows=None, lanes_per_row: int = 0):
    """y = A x in HBM (cfx_csr_spmv); `A` a float64 MatrixCSR or MergedCSR.  `x`: ncols values, `out`: nrows values
    (allocated when None); device torch tensors / DeviceBuffers are used in place, a numpy `x` is uploaded and the product
    comes back as numpy.  `rows`: only y[rows] is written.  lanes_per_row: 0 (chosen from the matrix) or 1, 4, 8, 16, 64."""
    nrows, ip, ix, va = _csr_arrays(A)
    keep: list = []
    host = not _lib.is_device(x)
    xp = _device_f64(x, A.ncols, "x", keep)
    rp, nr = _row_list(rows, keep)
    if out is None:
        if _lib.is_torch(x) and not host:
            import torch
            out = torch.zeros(nrows, dtype=torch.float64, device=x.device)
        else:
            out = np.zeros(nrows) if host else _lib.DeviceBuffer(nrows, np.float64)
            if not host:
                _lib.check(_lib.lib().cfx_device_memset(C.c_void_p(out.ptr), 0, C.c_size_t(8 * nrows)))
    yp = _device_f64(out, nrows, "out", keep)
    _lib.check(_lib.lib().cfx_csr_spmv(C.c_int64(nrows), C.c_void_p(ip), C.c_void_p(ix), C.c_void_p(va), rp, C.c_int64(nr),
                                       int(lanes_per_row), xp, yp))
    if not _lib.is_device(out):      # a host `out`: the staged copy comes back (unlisted entries as they went in)
        out[...] = keep[-1].numpy().reshape(out.shape)
    return out


def _krylov_solve(who: str, entry: str, o, A, b, x0, rows, domain, info_out):
    """The call both solvers make (cfx_cg_solve / cfx_minres_solve have one argument list): vectors, row list and info
    of `who`, then `entry` with the options `o`; returns (x, info)."""
    nrows, ip, ix, va = _csr_arrays(A)
    keep: list = []
    if domain is not None:
        rows = active_rows(domain)
    rp, nr = _row_list(rows, keep)
    if _lib.is_torch(b) and b.is_cuda:
        import torch
        if b.dtype != torch.float64 or not b.is_contiguous() or b.numel() != nrows:
            raise TypeError(f"b must be a contiguous float64 tensor of {nrows} values")
        x = torch.zeros_like(b) if x0 is None else torch.as_tensor(x0, dtype=torch.float64, device=b.device).clone().contiguous()
        bp, xp = C.c_void_p(b.data_ptr()), C.c_void_p(x.data_ptr())
    else:
        if _lib.is_device(b) or _lib.is_device(x0):
            raise TypeError(f"{who}: b (and x0) are numpy arrays or device torch tensors")
        b = np.ascontiguousarray(b, dtype=np.float64)
        x = np.zeros(nrows) if x0 is None else np.array(x0, dtype=np.float64).ravel()
        bp, xp = b.ctypes.data_as(C.c_void_p), x.ctypes.data_as(C.c_void_p)
        if b.size != nrows:
            raise ValueError(f"b must hold {nrows} values")
    if (x.numel() if _lib.is_torch(x) else x.size) != nrows:
        raise ValueError(f"x0 must hold {nrows} values")
    fn = getattr(_lib.lib(), entry)
    if info_out is not None:
        if not _lib.is_device(info_out):
            raise TypeError(f"{who}: info_out is a device buffer (cg_info_buffer())")
        ipn = _device_f64(info_out, 3, "info_out", keep)
        _lib.check(fn(C.c_int64(nrows), C.c_void_p(ip), C.c_void_p(ix), C.c_void_p(va), rp, C.c_int64(nr), bp, xp, C.byref(o), ipn))
        return x, info_out
    st = _lib.CGInfoStruct()
    _lib.check(fn(C.c_int64(nrows), C.c_void_p(ip), C.c_void_p(ix), C.c_void_p(va), rp, C.c_int64(nr), bp, xp, C.byref(o),
                  C.byref(st)))
    return x, CGInfo(int(st.reason), int(st.iterations), float(st.residual_norm), float(st.rhs_norm))


def _krylov_options(who: str, o, A, rows, domain, names: dict, precond, rtol, atol, max_iter, check_every, lanes_per_row):
    """The checks that run before the library is entered, and the options struct filled from the keywords."""
    if A.ncols != A.nrows:
        raise ValueError(f"{who} takes a square matrix")
    if rows is not None and domain is not None:
        raise ValueError(f"{who}: give `rows` or `domain`, not both")
    pc = names.get(precond.lower() if isinstance(precond, str) else precond)
    if pc is None:
        raise ValueError(f"{who}: precond is " + " or ".join(repr(k) for k in names if isinstance(k, str)))
    o.rtol, o.atol, o.precond, o.lanes_per_row = float(rtol), float(atol), pc, int(lanes_per_row)
    if max_iter is not None:
        o.max_iter = int(max_iter)
    if check_every is not None:
        o.check_every = int(check_every)
    return o


def cg_solve(A, b, x0=None, *, rtol: float = 1e-10, atol: float = 0.0, max_iter: int | None = None,
             precond: str = "jacobi", rows=None, domain=None, check_every: int | None = None, info_out=None,
             lanes_per_row: int = 0):
    """Solve A x = b by (Jacobi-)preconditioned conjugate gradients in HBM (cfx_cg_solve); returns (x, info).

    `A`: a float64 MatrixCSR or MergedCSR, symmetric positive definite on the iterated rows.  `b`: numpy array or
    device torch tensor; `x` comes back as the same kind (a new array; `x0` is not modified).  `rows` (int32 list, host or
    device) or `domain` (an ActiveDomain: its active rows, listed on the device) restrict the solve: entries of x
    outside the list keep the value of x0 (0 by default) and act as data.  Stops at |r| <= max(rtol |b|, atol).
    `check_every`: how often the host looks at the state (None: the library's default); the result does not depend on it.
    `info_out` (cg_info_buffer()): the cfx_cg_info stays in HBM, `info` is then info_out itself and -- with device
    vectors and check_every = 0 -- the call makes no host round trip: exactly `max_iter` iterations are launched and the
    ones after convergence return at once."""
    _csr_arrays(A)
    o = _krylov_options("cg_solve", cg_default_options(), A, rows, domain, {"jacobi": PC_JACOBI, "none": PC_NONE, None: PC_NONE},
                        precond, rtol, atol, max_iter, check_every, lanes_per_row)
    return _krylov_solve("cg_solve", "cfx_cg_solve", o, A, b, x0, rows, domain, info_out)


def minres_default_options() -> _lib.CGOptions:
    """The defaults of cfx_minres_options_default (no GPU needed)."""
    o = _lib.CGOptions()
    _lib.check(_lib.load().cfx_minres_options_default(C.byref(o)))
    return o


def minres_solve(A, b, x0=None, *, rtol: float = 1e-10, atol: float = 0.0, max_iter: int | None = None,
                 check_every: int | None = None, precond: str | None = "abs_jacobi", rows=None, domain=None,
                 lanes_per_row: int = 0, info_out=None):
    """Solve A x = b for a SYMMETRIC, possibly indefinite A by diagonally preconditioned MINRES in HBM
    (cfx_minres_solve); returns (x, info) -- what python/demo/demo_stokes.py:39-60 leaves to spsolve.

    Arguments, row-list semantics and return value are those of cg_solve (`A`: MatrixCSR, MergedCSR or csr_from_arrays).
    Symmetry on the iterated rows is required and NOT checked.  precond: "abs_jacobi" (m_i = |a_ii|; a listed row
    without a nonzero stored diagonal gives reason CG_BAD_DIAGONAL), "abs_rowsum" (m_i = sum_j |a_ij|: works where the
    diagonal is absent) or None / "none".  Stops at |r|_{M^-1} <= max(rtol |b|_{M^-1}, atol), |y|_{M^-1} = sqrt(y . M^-1 y)
    over the iterated rows; info.residual_norm / rhs_norm are these norms (the 2-norms when there is no preconditioner)."""
    _csr_arrays(A)
    names = {"abs_jacobi": PC_ABS_JACOBI, "abs_rowsum": PC_ABS_ROWSUM, "none": PC_NONE, None: PC_NONE}
    o = _krylov_options("minres_solve", minres_default_options(), A, rows, domain, names, precond, rtol, atol, max_iter,
                        check_every, lanes_per_row)
    return _krylov_solve("minres_solve", "cfx_minres_solve", o, A, b, x0, rows, domain, info_out)


def bicgstab_default_options() -> _lib.CGOptions:
    """The defaults of cfx_bicgstab_options_default (no GPU needed)."""
    o = _lib.CGOptions()
    _lib.check(_lib.load().cfx_bicgstab_options_default(C.byref(o)))
    return o


def bicgstab_solve(A, b, x0=None, *, rtol: float = 1e-10, atol: float = 0.0, max_iter: int | None = None,
                   precond: str | None = "jacobi", rows=None, domain=None, check_every: int | None = None, info_out=None,
                   lanes_per_row: int = 0):
    """Solve A x = b for a NONSYMMETRIC A by right-preconditioned BiCGStab in HBM (cfx_bicgstab_solve); returns
    (x, info) -- what python/demo/demo_compliance_optimization.py:1302-1350 leaves to spsolve.

    Arguments, row-list semantics and return value are those of cg_solve (`A`: MatrixCSR, MergedCSR or csr_from_arrays);
    the matrix need be neither symmetric nor definite.  precond: "jacobi" (d_i = a_ii with its sign; a listed row without
    a nonzero stored diagonal gives reason CG_BAD_DIAGONAL) or None / "none".  The preconditioner acts from the right, so
    the rule is cg_solve's: |r|_2 <= max(rtol |b|_2, atol) with r the residual of the system itself; info.residual_norm /
    rhs_norm are these 2-norms.  CG_BREAKDOWN: a scalar of the recurrence vanished or is not finite (the header lists
    which iterate x then holds)."""
    _csr_arrays(A)
    o = _krylov_options("bicgstab_solve", bicgstab_default_options(), A, rows, domain,
                        {"jacobi": PC_JACOBI, "none": PC_NONE, None: PC_NONE}, precond, rtol, atol, max_iter, check_every,
                        lanes_per_row)
    return _krylov_solve("bicgstab_solve", "cfx_bicgstab_solve", o, A, b, x0, rows, domain, info_out)


def zero_rows(A: MatrixCSR, *, tol: float = 0.0) -> np.ndarray:
    """Rows whose assembled entries are all <= tol in magnitude (python/cutfemx/fem.py:777-782)."""
    p, n = C.c_void_p(), C.c_int64()
    if A.dtype == np.dtype(np.float32):
        _lib.check(_lib.lib().cfx_zero_rows_f32(A._p, C.c_void_p(A.values_ptr), C.c_float(tol), C.byref(p), C.byref(n)))
    else:
        _lib.check(_lib.lib().cfx_zero_rows(A._p, C.c_void_p(A.values_ptr), C.c_double(tol), C.byref(p), C.byref(n)))
    out = _lib.download(p.value, n.value, np.int32)
    _lib.check(_lib.lib().cfx_device_free(p))
    return out


def zero_block_rows(A_blocks, *, tol: float = 0.0) -> list[np.ndarray]:
    """Zero rows of each block row of a MatrixCSR block system (python/cutfemx/fem.py:784-800,
    cpp/cutfemx/fem/deactivate.h:279-320): row r of block row i is listed when it is zero in EVERY block A[i][j]
    (None blocks count as zero).  Same checks and messages as the reference."""
    rows = [list(r) for r in A_blocks]
    if not rows:
        raise RuntimeError("Zero-row scan requires at least one block row")
    nb = len(rows)
    out = []
    for i, row in enumerate(rows):
        if len(row) != nb:
            raise RuntimeError("Zero-row scan requires a square block matrix")
        if row[i] is None:
            raise RuntimeError("Zero-row scan requires every diagonal matrix block")
        nrows = row[i].nrows
        if any(A is not None and A.nrows != nrows for A in row):
            raise RuntimeError("Zero-row scan found incompatible row maps in a block row")
        zero = None
        for A in row:
            if A is None:
                continue
            z = zero_rows(A, tol=tol)
            zero = z if zero is None else np.intersect1d(zero, z, assume_unique=True)
        out.append(np.asarray(zero, dtype=np.int32))
    return out


class MergedCSR:
    """The monolithic CSR matrix of a block system (merge_blocks): indptr (int64), indices (int32), float64 data in HBM."""

    def __init__(self, indptr, indices, values, nnz, nrows, ncols, row_offsets, col_offsets):
        self._indptr, self._indices, self._values = indptr, indices, values
        self.nnz, self.nrows, self.ncols = int(nnz), int(nrows), int(ncols)
        self.row_offsets, self.col_offsets = row_offsets, col_offsets   # first row / column of every block
        self.dtype = np.dtype(np.float64)

    @property
    def indptr(self):
        return _lib.download(self._indptr, self.nrows + 1, np.int64)

    @property
    def indices(self):
        return _lib.download(self._indices, self.nnz, np.int32)

    @property
    def data(self):
        return _lib.download(self._values, self.nnz, np.float64)

    def torch_views(self, device):
        """Zero-copy torch tensors (indptr int64, indices int32, values f64) over the HBM arrays."""
        from .dist import as_torch
        return (as_torch(self._indptr, self.nrows + 1, "int64", device), as_torch(self._indices, self.nnz, "int32", device),
                as_torch(self._values, self.nnz, "float64", device))

    def to_scipy(self):
        import scipy.sparse as sp
        return sp.csr_matrix((self.data, self.indices, self.indptr), shape=(self.nrows, self.ncols))

    def to_dense(self):
        return self.to_scipy().toarray()

    def __del__(self):
        try:
            l = _lib.load()
            for name in ("_indptr", "_indices", "_values"):
                if getattr(self, name, None):
                    l.cfx_device_free(C.c_void_p(getattr(self, name)))
                    setattr(self, name, None)
        except Exception:
            pass


def merge_blocks(A_blocks) -> MergedCSR:
    """One CSR matrix from a block system of float64 MatrixCSR blocks (None: an empty block): the monolithic matrix the
    reference assembles on a mixed element (python/tests/test_assembly_stokes.py:34-95), with block-ordered dofs -- all
    rows of block row 0, then of block row 1 ...; columns likewise.  Every block row / column needs one block that fixes
    its size; sizes must agree along rows and columns.  Runs on the GPU (cfx_csr_block_merge); the blocks are not changed."""
    rows = [list(r) for r in A_blocks]
    if not rows or not rows[0]:
        raise RuntimeError("merge_blocks requires at least one block")
    nbr, nbc = len(rows), len(rows[0])
    if any(len(r) != nbc for r in rows):
        raise RuntimeError("merge_blocks requires the same number of blocks in every block row")
    nrows, ncols = [None] * nbr, [None] * nbc
    for i, r in enumerate(rows):
        for j, A in enumerate(r):
            if A is None:
                continue
            if A.dtype != np.dtype(np.float64):
                raise TypeError("merge_blocks takes float64 blocks")
            if nrows[i] not in (None, A.nrows) or ncols[j] not in (None, A.ncols):
                raise RuntimeError("merge_blocks found incompatible block sizes")
            nrows[i], ncols[j] = A.nrows, A.ncols
    if any(n is None for n in nrows) or any(n is None for n in ncols):
        raise RuntimeError("merge_blocks requires a block in every block row and every block column")
    _lib.resolve_counts()
    n = nbr * nbc
    ip, ix, va = (C.c_void_p * n)(), (C.c_void_p * n)(), (C.c_void_p * n)()
    for i, r in enumerate(rows):
        for j, A in enumerate(r):
            if A is not None:
                k = i * nbc + j
                ip[k], ix[k], va[k] = A._view.indptr, A._view.indices, A.values_ptr
    nr, nc = (C.c_int64 * nbr)(*nrows), (C.c_int64 * nbc)(*ncols)
    o_ip, o_ix, o_va, o_nnz = C.c_void_p(), C.c_void_p(), C.c_void_p(), C.c_int64()
    _lib.check(_lib.lib().cfx_csr_block_merge(nbr, nbc, ip, ix, va, nr, nc, C.byref(o_ip), C.byref(o_ix), C.byref(o_va),
                                              C.byref(o_nnz)))
    return MergedCSR(o_ip.value, o_ix.value, o_va.value, o_nnz.value, sum(nrows), sum(ncols),
                     np.concatenate([[0], np.cumsum(nrows)[:-1]]).astype(np.int64),
                     np.concatenate([[0], np.cumsum(ncols)[:-1]]).astype(np.int64))


def permute_csr(A, row_perm, col_perm=None) -> MergedCSR:
    """The matrix `A` (a MergedCSR or MatrixCSR of float64 values) with row r moved to row_perm[r] and column c to
    col_perm[c] (default: the same map), columns of every row ascending again -- on the GPU (cfx_csr_permute)."""
    col_perm = row_perm if col_perm is None else col_perm
    rp = np.ascontiguousarray(row_perm, dtype=np.int32)
    cp = np.ascontiguousarray(col_perm, dtype=np.int32)
    if rp.size != A.nrows or cp.size != A.ncols:
        raise ValueError("permute_csr: one target per row and per column")
    if isinstance(A, MergedCSR):
        ip, ix, va, nnz = A._indptr, A._indices, A._values, A.nnz
    else:
        _lib.resolve_counts()
        ip, ix, va, nnz = A._view.indptr, A._view.indices, A.values_ptr, A.nnz
    o_ip, o_ix, o_va = C.c_void_p(), C.c_void_p(), C.c_void_p()
    _lib.check(_lib.lib().cfx_csr_permute(C.c_int64(A.nrows), C.c_int64(A.ncols), C.c_void_p(ip), C.c_void_p(ix), C.c_void_p(va),
                                          rp.ctypes.data_as(C.c_void_p), cp.ctypes.data_as(C.c_void_p), C.byref(o_ip),
                                          C.byref(o_ix), C.byref(o_va)))
    return MergedCSR(o_ip.value, o_ix.value, o_va.value, nnz, A.nrows, A.ncols, np.zeros(1, np.int64), np.zeros(1, np.int64))


class MixedSpace:
    """A space on a mixed element -- `mixed_element([P2 vector, P1])` of python/tests/test_assembly_stokes.py:34-95 -- as ONE
    object: the caller's mixed dofmap (DOLFINx's: the dofs of all sub-elements numbered together, cell by cell) and the
    sub-elements' (degree, block size).

        W = fem.MixedSpace(mesh, mixed_dofmap, ndofs, [(2, gdim), (1, 1)])
        a = {(0, 0): [Integral(...)], (0, 1): [...], (1, 0): [...], (1, 1): [...]}   # integrals by (test, trial) sub-element
        A = W.assemble_matrix(a)          # ONE CSR matrix in the numbering of `mixed_dofmap`

    Row `mixed_dofmap[c]` lists the cell's dofs sub-element by sub-element; sub-element s takes ndofs_cell(degree_s) x
    bs_s entries, (node i, component k) at i * bs_s + k (the layout of DOLFINx's flattened mixed dofmaps).  The engine
    assembles per (test, trial) pair on block spaces it derives from the columns of the mixed dofmap -- sub.space(s): nodes
    numbered in the order of their first component's mixed dof --, merges the blocks (merge_blocks: block-ordered dofs)
    and moves rows and columns to the mixed numbering (permute_csr with block_to_mixed)."""

    def __init__(self, mesh, mixed_dofmap, ndofs: int, subs):
        from .mesh import FunctionSpace
        M = np.ascontiguousarray(mixed_dofmap, dtype=np.int32)
        if M.ndim != 2 or M.shape[0] != mesh.num_cells:
            raise ValueError("MixedSpace: mixed_dofmap holds one row per cell")
        tdim = mesh.tdim
        self.mesh, self.ndofs, self.subs = mesh, int(ndofs), [(int(d), int(b)) for d, b in subs]
        self.spaces, self.block_to_mixed, self.offsets = [], [], []
        o = 0
        for degree, bs in self.subs:
            if degree not in (1, 2):
                raise ValueError("MixedSpace: sub-elements of degree 1 or 2")
            nd = tdim + 1 if degree == 1 else (tdim + 1) * (tdim + 2) // 2
            if o + nd * bs > M.shape[1]:
                raise ValueError("MixedSpace: the mixed dofmap has fewer entries per cell than its sub-elements need")
            cols = o + bs * np.arange(nd)
            comp0 = M[:, cols]
            nodes = np.unique(comp0)                       # ascending: node k of the block space <-> nodes[k]
            sub_map = np.searchsorted(nodes, comp0).astype(np.int32)
            perm = np.full(nodes.size * bs, -1, dtype=np.int64)
            for k in range(bs):
                perm[sub_map.ravel().astype(np.int64) * bs + k] = M[:, cols + k].ravel()
            if degree == 1 and nodes.size == mesh.num_nodes and np.array_equal(sub_map, mesh.conn):
                V = FunctionSpace(mesh, 1, bs=bs)           # the geometry dofmap itself: the stencil paths apply
            else:
                V = FunctionSpace(mesh, degree, dofmap=sub_map, ndofs=int(nodes.size), bs=bs)
            self.spaces.append(V)
            self.block_to_mixed.append(perm)
            self.offsets.append(o)
            o += nd * bs
        if o != M.shape[1]:
            raise ValueError("MixedSpace: the sub-elements do not account for every entry of a mixed dofmap row")
        P = np.concatenate(self.block_to_mixed)
        if P.size != self.ndofs or P.min() < 0 or np.unique(P).size != P.size or P.max() != self.ndofs - 1:
            raise ValueError("MixedSpace: the sub-elements' dofs do not number 0 .. ndofs - 1 exactly once")
        self.permutation = P.astype(np.int32)              # block-ordered dof -> mixed dof
        self.block_offsets = np.concatenate([[0], np.cumsum([p.size for p in self.block_to_mixed])]).astype(np.int64)

    def sub(self, s: int):
        """The block space of sub-element s (W.sub(s).collapse() of the reference)."""
        return self.spaces[s]

    def form(self, integrals, test: int, trial: int) -> CutForm:
        """The bilinear form of the integrals between sub-elements `test` and `trial`."""
        V0, V1 = self.spaces[test], self.spaces[trial]
        return form(list(integrals), V0, rank=2, trial_space=None if trial == test else V1)

    def assemble_matrix(self, blocks: dict, deactivate: dict | None = None) -> MergedCSR:
        """ONE matrix in the mixed numbering from integrals given by (test, trial) sub-element pair.  `deactivate`
        (optional): {s: ActiveDomain or True} -- the inactive rows of diagonal block (s, s) get a unit diagonal
        (deactivate_outside_blocks) before the merge; True takes the block's own active domain."""
        ns = len(self.spaces)
        forms = {k: (v if isinstance(v, CutForm) else self.form(v, *k)) for k, v in blocks.items()}
        A = [[assemble_matrix(forms[(i, j)]) if (i, j) in forms else None for j in range(ns)] for i in range(ns)]
        if deactivate:
            doms = []
            for s in range(ns):
                d = deactivate.get(s)
                doms.append(active_domain(forms[(s, s)]) if d is True else d)
            if all(d is not None for d in doms):
                deactivate_outside_blocks(A, doms)
            else:
                for s, d in enumerate(doms):
                    if d is not None:
                        deactivate_outside(A[s][s], None, d)
        # (a sub-element without any block still needs its rows: an empty pattern of the right size is not built here)
        merged = merge_blocks(A)
        return permute_csr(merged, self.permutation)

    def vector_to_mixed(self, b_blocks) -> np.ndarray:
        """Block vectors (one per sub-element, block numbering) -> one vector in the mixed numbering."""
        out = np.zeros(self.ndofs, dtype=np.float64)
        for perm, b in zip(self.block_to_mixed, b_blocks):
            out[perm] = np.asarray(b.cpu() if hasattr(b, "cpu") else b, dtype=np.float64)
        return out


def deactivate_outside_blocks(A_blocks, active_domains, b_blocks=None, *, diagonal: float = 1.0,
                              rhs_value: float = 0.0) -> list:
    """Deactivate block rows from per-row active-domain support (python/cutfemx/fem.py:739-775,
    cpp/cutfemx/fem/deactivate.h:420-457): the inactive rows of block row i come from active_domains[i]; only the
    diagonal block A_blocks[i][i] and the optional right-hand side b_blocks[i] are modified -- off-diagonal blocks are
    left alone on purpose (an inactive coupling entry is a form / domain consistency bug, not something to clean)."""
    rows = [list(r) for r in A_blocks]
    domains = list(active_domains)
    if not rows:
        raise RuntimeError("Block deactivation requires at least one block row")
    if len(rows) != len(domains):
        raise RuntimeError("Block deactivation requires one ActiveDomain per block row")
    nb = len(rows)
    for i, row in enumerate(rows):
        if len(row) != nb:
            raise RuntimeError("Block deactivation requires a square block matrix")
        if domains[i] is None:
            raise RuntimeError("Block deactivation received a null ActiveDomain")
        if row[i] is None:
            raise RuntimeError("Block deactivation requires every diagonal matrix block")
    if b_blocks is not None:
        b_blocks = list(b_blocks)
        if len(b_blocks) != nb:
            raise RuntimeError("Block deactivation requires one RHS vector per block row")
        if any(b is None for b in b_blocks):
            raise RuntimeError("Block deactivation received a null RHS vector")
    for i in range(nb):
        deactivate_outside(rows[i][i], None if b_blocks is None else b_blocks[i], domains[i], diagonal=diagonal,
                           rhs_value=rhs_value)
    return domains


def tabulate_entity(a: CutForm, integral: int, index: int, use_rule: bool) -> np.ndarray:
    """Local tensor of one entity (for local-entry parity checks)."""
    V = a.function_space
    I = a.integrals[integral]
    facet_type = I.facets is not None or (I.rules is not None and I.rules.host_width == 4)
    nloc = V.ndofs_cell * V.bs * (2 if facet_type else 1)
    V1 = getattr(a, "trial_space", V)
    nloc1 = nloc if V1 is V else V1.ndofs_cell * V1.bs * (2 if facet_type else 1)   # [(nd0 bs0) x (nd1 bs1)] row-major for rectangular forms (facets: both cells)
    Ae = np.zeros((nloc, nloc1) if a.rank == 2 else (nloc,) if a.rank == 1 else (1,))   # a functional: the entity's value
    _lib.check(_lib.lib().cfx_tabulate_entity(a._h, integral, C.c_int64(index), int(use_rule),
                                              Ae.ctypes.data_as(C.c_void_p)))
    return Ae


class ActiveDomain:
    """cutfemx.fem.ActiveDomain (cpp/cutfemx/fem/deactivate.h:387-400)."""

    def __init__(self, handle, V, form=None):
        # (the lists of the domain are compacted on first request from the plan of `form`, whose facet rows alias the
        # form's own entity arrays: the form -- and with it the lists its integrals pin -- lives as long as this object)
        self._h, self.function_space, self._form = handle, V, form

    def _view(self):
        """(active cells, count, inactive dofs, count): the counts are capacities while the cutfemx_amd.step that made
        the domain is open, exact afterwards."""
        ac, na, idf, ni = C.c_void_p(), C.c_int64(), C.c_void_p(), C.c_int64()
        _lib.check(_lib.lib().cfx_active_view(self._h, C.byref(ac), C.byref(na), C.byref(idf), C.byref(ni)))
        return ac.value, na.value, idf.value, ni.value

    @property
    def active_cells(self):
        _lib.resolve_counts()
        ac, na, _, _ = self._view()
        return _lib.download(ac, na, np.int32)

    @property
    def inactive_dofs(self):
        _lib.resolve_counts()
        _, _, idf, ni = self._view()
        return _lib.download(idf, ni, np.int32)

    @property
    def num_active_dofs(self):
        """Dofs touched by an entity of the form (no list is built for this: the row marks of the form's plan)."""
        V = self.function_space
        ni = C.c_int64()
        _lib.check(_lib.lib().cfx_active_view(self._h, None, None, None, C.byref(ni)))
        return V.ndofs * V.bs - ni.value

    def __del__(self):
        try:
            if self._h:
                _lib.load().cfx_active_destroy(self._h)
                self._h = None
        except Exception:
            pass


def active_domain(a: CutForm) -> ActiveDomain:
    h = C.c_void_p()
    _lib.check(_lib.lib().cfx_active_domain(a._h, C.byref(h)))
    return ActiveDomain(h, a.function_space, a)


def deactivate_outside(A: MatrixCSR | None, b, domain: ActiveDomain, diagonal: float = 1.0,
                       rhs_value: float = 0.0) -> ActiveDomain:
    """diag=1 / rhs=0 on dofs outside the active domain (deactivate.h:402-418)."""
    bp = None
    if b is not None:
        bp = C.c_void_p(b.data_ptr()) if _lib.is_torch(b) else b.ctypes.data_as(C.c_void_p)
    dts = {np.dtype(A.dtype)} if A is not None else set()
    if b is not None:
        dts.add(np.dtype(_lib.scalar_dtype(b)))
    if len(dts) > 1:
        raise TypeError("deactivate_outside: matrix and vector must have one scalar type")
    if dts in ({_C128}, {_C64}):
        d, r = complex(diagonal), complex(rhs_value)
        _lib.check(_cfn("deactivate_outside", next(iter(dts)))(domain._h, A._p if A is not None else None,
                                                          C.c_void_p(A.values_ptr) if A is not None else None, bp,
                                                          C.c_double(d.real), C.c_double(d.imag), C.c_double(r.real), C.c_double(r.imag)))
        return domain
    if dts == {np.dtype(np.float32)}:
        _lib.check(_lib.lib().cfx_deactivate_outside_f32(domain._h, A._p if A is not None else None,
                                                         C.c_void_p(A.values_ptr) if A is not None else None, bp,
                                                         C.c_float(diagonal), C.c_float(rhs_value)))
        return domain
    _lib.check(_lib.lib().cfx_deactivate_outside(domain._h, A._p if A is not None else None,
                                                 C.c_void_p(A.values_ptr) if A is not None else None, bp,
                                                 C.c_double(diagonal), C.c_double(rhs_value)))
    return domain
