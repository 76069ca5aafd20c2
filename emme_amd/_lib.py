"""ctypes binding of include/emme_hip.h.  Names mirror the reference's objects:
Params <- Parameters (include/Parameters.h), Context <- EigenSolver (include/solver.h:44-516).
"""
from __future__ import annotations

import ctypes as C
import os

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
_LIB = None


class EmmeError(RuntimeError):
    def __init__(self, code, msg):
        super().__init__(f"[emme {code}] {msg}")
        self.code = code
        self.reason = msg


def lib_path() -> str:
    # EMME_LIB lets a developer A/B a differently-built library; the default is the in-tree one
    return os.environ.get("EMME_LIB") or os.path.join(HERE, "libemme_hip.so")


class Params(C.Structure):
    """emme_params_t (include/emme_params.h)."""

    _fields_ = [
        ("conf", C.c_int), ("iteration_method", C.c_int),
        ("q", C.c_double), ("shat", C.c_double), ("tau", C.c_double),
        ("epsilon_n", C.c_double), ("epsilon_r", C.c_double),
        ("eta_i", C.c_double), ("eta_e", C.c_double), ("k_rho", C.c_double),
        ("beta_e", C.c_double), ("R", C.c_double), ("vt", C.c_double),
        ("omega_d_coeff", C.c_double), ("length", C.c_double), ("theta", C.c_double),
        ("npoints", C.c_int), ("iteration_step_limit", C.c_int),
        ("integration_precision", C.c_double), ("integration_accuracy", C.c_double),
        ("integration_iteration_limit", C.c_int), ("integration_start_points", C.c_int),
        ("arc_coeff", C.c_double),
        ("water_bag_weight_vpara", C.c_double), ("water_bag_weight_vperp", C.c_double),
        ("drift_center_transformation_switch", C.c_int),
        ("iteration_precision", C.c_double),
        ("initial_guess", C.c_double * 2),
        ("eta_k", C.c_double), ("lh", C.c_int), ("mh", C.c_int),
        ("epsilon_h_t", C.c_double), ("alpha_0", C.c_double), ("r_over_R", C.c_double),
        ("b_theta", C.c_double), ("alpha", C.c_double), ("omega_s_i", C.c_double),
        ("omega_s_e", C.c_double), ("omega_d_bar", C.c_double),
        ("deltap", C.c_double), ("beta_e_p", C.c_double), ("rdeltapp", C.c_double),
        ("curvature_aver", C.c_double), ("shat_coeff", C.c_double),
    ]

    @property
    def dim(self) -> int:
        return self.npoints if self.beta_e == 0.0 else 2 * self.npoints


class Profile(C.Structure):
    """emme_profile_t."""

    _fields_ = [
        ("assemble_ms", C.c_double), ("assemble_launches", C.c_long),
        ("deferred_ms", C.c_double), ("deferred_launches", C.c_long),
        ("linstep_ms", C.c_double), ("linstep_launches", C.c_long),
        ("other_ms", C.c_double), ("other_launches", C.c_long),
        ("gk_intervals", C.c_longlong), ("integrand_evals", C.c_longlong),
        ("matrices", C.c_longlong), ("union_rounds", C.c_longlong),
        ("cache_build_ms", C.c_double), ("cache_build_launches", C.c_long),
        ("cache_alloc_ms", C.c_double),
        ("dense_rounds", C.c_longlong), ("sparse_rounds", C.c_longlong),
        ("sparse_columns", C.c_longlong), ("tile_tasks", C.c_longlong),
        ("nullspace_ms", C.c_double), ("nullspace_launches", C.c_long),
    ]


FILL_AUTO, FILL_UNION, FILL_LANES = 0, 1, 2


class Contour(C.Structure):
    """emme_contour_t: the ellipse and the quadrature / probe settings of a region search."""

    _fields_ = [
        ("size", C.c_int), ("center", C.c_double * 2), ("semi_axes", C.c_double * 2),
        ("points", C.c_int), ("max_points", C.c_int), ("probes", C.c_int), ("rank_tol", C.c_double),
    ]


class Options(C.Structure):
    """emme_options_t: per-context options (cache budget, fill routing, LU split ...)."""

    _fields_ = [
        ("size", C.c_int),
        ("node_cache_gb", C.c_double), ("cache_min_batch", C.c_int), ("cache_min_depth", C.c_int),
        ("fill", C.c_int), ("phase_table", C.c_int), ("em_shared", C.c_int), ("wl_min", C.c_int),
        ("union_sel", C.c_int), ("union_ipg_few", C.c_int), ("union_few_chunks", C.c_int),
        ("coop_wide_min", C.c_int), ("defer_one_group", C.c_int),
        ("dense_min_cols", C.c_int), ("dense_min_tasks", C.c_int),
        ("tile_uncached", C.c_int),  # (in what was alignment padding: no other field moved)
        ("dense_cost_ratio", C.c_double),
        ("dense_wide", C.c_int),
        ("skip_lost", C.c_int),
        ("lu_split", C.c_int), ("lu_group_min_n", C.c_int), ("lu_spin_limit", C.c_int),
        ("lu_unblocked", C.c_int),
        ("deriv_cached", C.c_int),
    ]
    # emme_options_t::dense_stage sits in the four bytes behind deriv_cached that pad the struct to its alignment
    # (the size is what it was): mirrored as a property on those bytes, so that the declared fields stay as they were
    _DENSE_STAGE_OFFSET = 108

    @property
    def dense_stage(self) -> int:
        return C.c_int.from_buffer(self, self._DENSE_STAGE_OFFSET).value

    @dense_stage.setter
    def dense_stage(self, v) -> None:
        C.c_int.from_buffer(self, self._DENSE_STAGE_OFFSET).value = int(v)



# options every new Context starts from (the tests build their node cache for a handful of omegas)
_DEFAULT_OPTIONS: dict = {}


def set_default_options(**kw) -> None:
    """Python-side defaults merged into every Context created afterwards (explicit arguments win)."""
    _DEFAULT_OPTIONS.clear()
    _DEFAULT_OPTIONS.update(kw)


def default_options(**kw) -> Options:
    o = Options()
    load().emme_options_default(C.byref(o))
    for k, v in {**_DEFAULT_OPTIONS, **kw}.items():
        if not hasattr(o, k):
            raise TypeError(f"unknown option {k!r}")
        setattr(o, k, v)
    return o


def load():
    """Load libemme_hip.so or raise: the product path never falls back to a CPU path."""
    global _LIB
    if _LIB is not None:
        return _LIB
    path = lib_path()
    if not os.path.exists(path):
        raise EmmeError(-3, f"{path} is missing: build it with __graft_entry__.build() "
                            "(make -C emme_amd/csrc); there is no CPU fallback")
    lib = C.CDLL(path)
    P = C.c_void_p
    PP = C.POINTER(Params)
    lib.emme_last_error.restype = C.c_char_p
    lib.emme_params_from_json.argtypes = [C.c_char_p, PP]
    lib.emme_params_derive.argtypes = [PP]
    lib.emme_tables.argtypes = [PP, P, P, P, P]
    lib.emme_weight.argtypes = [C.c_int, C.c_int, C.c_int]
    lib.emme_weight.restype = C.c_double
    lib.emme_bessel_batch.argtypes = [P, C.c_int, P]
    lib.emme_elementary_batch.argtypes = [C.c_int, P, C.c_int, P]
    lib.emme_integrand_batch.argtypes = [PP, C.c_int, C.c_int, P, P, P, P, P, P]
    lib.emme_ctx_create.argtypes = [PP, C.c_int, C.POINTER(P)]
    lib.emme_options_default.argtypes = [C.POINTER(Options)]
    lib.emme_options_default.restype = None
    lib.emme_ctx_create_ex.argtypes = [PP, C.c_int, C.POINTER(Options), C.POINTER(P)]
    lib.emme_ctx_set_options.argtypes = [P, C.POINTER(Options)]
    lib.emme_ctx_get_options.argtypes = [P, C.POINTER(Options)]
    lib.emme_null_vectors_batch.argtypes = [P, C.c_int, C.c_int, P, P, P]
    lib.emme_ctx_destroy.argtypes = [P]
    lib.emme_ctx_destroy.restype = None
    lib.emme_release_pooled_memory.argtypes = []
    lib.emme_release_pooled_memory.restype = None
    lib.emme_ctx_set_stream.argtypes = [P, P]
    lib.emme_ctx_set_tile_shapes.argtypes = [P, C.c_int]
    lib.emme_ctx_get_tile_shapes.argtypes = [P]
    lib.emme_ctx_set_deriv_cache_shapes.argtypes = [P, C.c_int]
    lib.emme_ctx_get_deriv_cache_shapes.argtypes = [P]
    if hasattr(lib, "emme_ctx_set_mirror_pairs"):  # (an older library loaded through EMME_LIB for an A/B has neither)
        lib.emme_ctx_set_mirror_pairs.argtypes = [P, C.c_int]
        lib.emme_ctx_get_mirror_pairs.argtypes = [P]
    if hasattr(lib, "emme_ctx_set_mirror_shapes"):  # (an older library loaded through EMME_LIB for an A/B has neither)
        lib.emme_ctx_set_mirror_shapes.argtypes = [P, C.c_int]
        lib.emme_ctx_get_mirror_shapes.argtypes = [P]
    if hasattr(lib, "emme_ctx_set_lu_fold"):  # (an older library loaded through EMME_LIB for an A/B has none)
        lib.emme_ctx_set_lu_fold.argtypes = [P, C.c_int]
        lib.emme_ctx_get_lu_fold.argtypes = [P]
        lib.emme_ctx_last_folded_steps.argtypes = [P]
        lib.emme_trace_secant_folded_batch.argtypes = [P, C.c_int, C.c_int, P, P, P, P, P]
    if hasattr(lib, "emme_ctx_set_eigpair_fold"):  # (an older library loaded through EMME_LIB for an A/B has none)
        lib.emme_ctx_set_eigpair_fold.argtypes = [P, C.c_int]
        lib.emme_ctx_get_eigpair_fold.argtypes = [P]
        lib.emme_ctx_last_folded_eigpair_steps.argtypes = [P]
        lib.emme_eigenpair_secant_folded_step_batch.argtypes = [P, C.c_int, C.c_int, P, P, P, P, P, P, P]
        lib.emme_vector_parity.argtypes = [C.c_int, C.c_int, P, P]
    if hasattr(lib, "emme_ctx_linstep_kernel_symbol"):  # (an older library loaded through EMME_LIB for an A/B has none)
        lib.emme_ctx_linstep_kernel_symbol.argtypes = [P]
        lib.emme_ctx_linstep_kernel_symbol.restype = C.c_char_p
        lib.emme_ctx_last_lu_workgroups.argtypes = [P]
        lib.emme_ctx_last_lu_slices.argtypes = [P]
        lib.emme_ctx_compute_units.argtypes = [P]
    lib.emme_ctx_dim.argtypes = [P]
    lib.emme_ctx_fill_mode.argtypes = [P]
    lib.emme_ctx_last_deferred.argtypes = [P]
    lib.emme_ctx_last_deferred.restype = C.c_longlong
    lib.emme_ctx_node_cache_gib.argtypes = [P]
    lib.emme_ctx_node_cache_gib.restype = C.c_double
    lib.emme_ctx_cache_settle.argtypes = [P, P, C.c_int, P]
    lib.emme_ctx_cache_state.argtypes = [P, P, P, P]
    lib.emme_ctx_profile_enable.argtypes = [P, C.c_int]
    lib.emme_ctx_profile_read.argtypes = [P, C.POINTER(Profile), C.c_int]
    lib.emme_assemble_batch.argtypes = [P, P, C.c_int, P, P]
    lib.emme_trace_solve_batch.argtypes = [P, C.c_int, C.c_int, P, P, P, P]
    lib.emme_qr_secant_batch.argtypes = [P, C.c_int, C.c_int, P, P, P, P]
    lib.emme_newton_step_batch.argtypes = [P, P, P, C.c_int, P, P, C.c_int, P]
    lib.emme_solve_roots.argtypes = [P, P, C.c_int, C.c_double, C.c_int, P, P, P, P]
    lib.emme_assemble_derivative_batch.argtypes = [P, P, C.c_int, P, P, P]
    lib.emme_solve_roots_newton.argtypes = [P, P, C.c_int, C.c_double, C.c_int, P, P, P, P]
    lib.emme_ctx_get_matrix.argtypes = [P, C.c_int, P]
    lib.emme_params_same_shape.argtypes = [PP, PP]
    lib.emme_ctx_bind_param_sets.argtypes = [P, P, C.c_int]
    lib.emme_ctx_param_sets.argtypes = [P]
    lib.emme_assemble_sets_batch.argtypes = [P, P, P, C.c_int, P, P, P]
    lib.emme_solve_roots_sets.argtypes = [P, P, P, C.c_int, C.c_int, C.c_double, C.c_int, P, P, P, P]
    lib.emme_solve_eigenpairs.argtypes = [P, P, P, C.c_int, P, C.c_double, C.c_int, P, P, P, P, P, P]
    lib.emme_eigenpair_step_batch.argtypes = [P, C.c_int, C.c_int, P, P, P, C.c_int, P, P, P]
    if hasattr(lib, "emme_solve_eigenpairs_secant"):  # (an older library loaded through EMME_LIB for an A/B has none)
        lib.emme_solve_eigenpairs_secant.argtypes = lib.emme_solve_eigenpairs.argtypes
        lib.emme_eigenpair_secant_step_batch.argtypes = [P, C.c_int, C.c_int, P, P, P, P, C.c_int, P, P, P]
        lib.emme_contour_eigpairs.argtypes = [C.c_int, C.c_int, P, P, C.c_double, C.c_int, P, P, P, P]
        lib.emme_find_eigenpairs_in_contour.argtypes = [P, C.POINTER(Contour), C.c_int, C.c_double, C.c_int, C.c_int,
                                                        P, P, P, P, P, P, P, P]
        lib.emme_find_eigenpairs_in_contours_sets.argtypes = [P, C.c_int, P, P, C.c_int, C.c_double, C.c_int, C.c_int,
                                                              P, P, P, P, P, P, P, P, P]
    if hasattr(lib, "emme_root_sensitivities_sets"):  # (an older library loaded through EMME_LIB for an A/B has none)
        lib.emme_sym_forms_batch.argtypes = [P, C.c_int, C.c_int, P, P, C.c_int, P, C.c_int, P, P, P, P, P, P]
        lib.emme_root_sensitivities_sets.argtypes = [P, C.c_int, P, P, P, C.c_int, P, P, P, C.c_int, P, P, P, P, P]
    lib.emme_run_json_lockstep.argtypes = [C.c_char_p, C.c_char_p, C.POINTER(C.c_void_p)]
    lib.emme_scan_plan.argtypes = [C.c_char_p, C.c_int, P, P, P, P, C.c_int, P, P, P]
    lib.emme_null_vector.argtypes = [P, C.c_int, P]
    lib.emme_run_json.argtypes = [C.c_char_p, C.c_char_p, C.POINTER(C.c_void_p)]
    lib.emme_free.argtypes = [C.c_void_p]
    lib.emme_free.restype = None
    lib.emme_scan_values.argtypes = [C.c_double, C.c_double, C.c_double, C.c_double, P, P, C.c_int]
    lib.emme_comm_unique_id.argtypes = [P]
    lib.emme_comm_create.argtypes = [P, C.c_int, C.c_int, C.c_int, C.POINTER(P)]
    lib.emme_comm_destroy.argtypes = [P]
    lib.emme_comm_destroy.restype = None
    lib.emme_gather_roots.argtypes = [P, P, P, P, P, C.c_int, C.c_int, P, P, P]
    lib.emme_comm_available.argtypes = []
    lib.emme_gather_slots.argtypes = [C.c_int, C.c_int]
    lib.emme_gather_share.argtypes = [C.c_int, C.c_int, C.c_int]
    lib.emme_gather_pack.argtypes = [C.c_int, C.c_int, P, P, P, C.c_int, C.c_int, P]
    lib.emme_gather_unpack.argtypes = [C.c_int, C.c_int, P, P, P, P]
    lib.emme_version.argtypes = []
    lib.emme_contour_default.argtypes = [C.POINTER(Contour)]
    lib.emme_contour_default.restype = None
    lib.emme_find_roots_in_contour.argtypes = [P, C.POINTER(Contour), C.c_double, C.c_int, C.c_int, P, P, P, P, P, P]
    lib.emme_contour_moments_batch.argtypes = [P, C.c_int, C.c_int, P, P, P, C.c_int, P, P, P, P, P]
    lib.emme_contour_eigs.argtypes = [C.c_int, C.c_int, P, P, C.c_double, C.c_int, P, P, P]
    lib.emme_contour_moments_groups.argtypes = [P, C.c_int, C.c_int, P, P, C.c_int, P, P, C.c_int, P, P, P, P, P]
    lib.emme_find_roots_in_contours_sets.argtypes = [P, C.c_int, P, P, C.c_int, C.c_double, C.c_int, C.c_int,
                                                     P, P, P, P, P, P, P]
    _LIB = lib
    return lib


def _check(rc):
    if rc != 0:
        raise EmmeError(rc, load().emme_last_error().decode(errors="replace"))


def _fnum(x) -> str:
    if isinstance(x, bool):
        return "true" if x else "false"
    if isinstance(x, int):
        return str(x)
    s = repr(float(x))
    if "e" in s:
        m, e = s.split("e")
        if "." not in m:
            m += ".0"
        return m + "e" + e
    return s


def json_text(d: dict) -> str:
    """Serialise a dict so that the reference grammar (a number is a float only if it
    contains '.') reads back the intended values."""
    items = []
    for k, v in d.items():
        if isinstance(v, str):
            items.append(f'"{k}": "{v}"')
        elif isinstance(v, (list, tuple)):
            items.append(f'"{k}": [' + ", ".join(_fnum(x) for x in v) + "]")
        elif isinstance(v, dict):
            items.append(f'"{k}": ' + json_text(v))
        else:
            items.append(f'"{k}": {_fnum(v)}')
    return "{" + ", ".join(items) + "}"


def params_from_json(text: str) -> Params:
    """Parameters::generate on a JSON text (reference src/Parameters.cpp:10-66)."""
    p = Params()
    _check(load().emme_params_from_json(text.encode(), C.byref(p)))
    return p


def params_from_dict(d: dict) -> Params:
    return params_from_json(json_text(d))


def tables(p: Params):
    n = p.npoints
    eta, g, b = np.zeros(n), np.zeros(n), np.zeros(n)
    dx = C.c_double(0)
    _check(load().emme_tables(C.byref(p), eta.ctypes.data, g.ctypes.data, b.ctypes.data,
                              C.addressof(dx)))
    return eta, g, b, dx.value


def weight(n, i, j) -> float:
    return load().emme_weight(n, i, j)


def bessel(z) -> np.ndarray:
    """util::bessel_i_alter_helper (include/functions.h:381-408) on the device: [n, 4] complex."""
    z = np.ascontiguousarray(np.atleast_1d(z), dtype=np.complex128)
    out = np.zeros((len(z), 4), dtype=np.complex128)
    _check(load().emme_bessel_batch(z.ctypes.data, len(z), out.ctypes.data))
    return out


# emme_elementary_batch: name -> (fn, doubles in, doubles out) per item
ELEMENTARY = {"rcp": (0, 1, 1), "rsqrt": (1, 1, 1), "exp": (2, 1, 1), "exp_s": (3, 1, 1), "exp_v": (4, 1, 1),
              "sincos": (5, 1, 2), "sincos_s": (6, 1, 2), "sincos_v": (7, 1, 2), "crcp": (8, 2, 2)}
FORM_F, FORM_F_DF, FORM_SPLIT, FORM_W = 0, 1, 2, 3


def elementary(fn: str, x) -> np.ndarray:
    """One device math primitive of the fill per argument (emme_elementary_batch): [n] for rcp / rsqrt / exp*,
    [n, 2] = (sin, cos) for sincos*, complex [n] in and out for crcp."""
    code, n_in, n_out = ELEMENTARY[fn]
    x = np.ascontiguousarray(np.atleast_1d(x), dtype=np.complex128 if n_in == 2 else np.float64)
    out = np.zeros((len(x), n_out))
    _check(load().emme_elementary_batch(code, x.ctypes.data, len(x), out.ctypes.data))
    if fn == "crcp":
        return out.view(np.complex128)[:, 0]
    return out[:, 0] if n_out == 1 else out


def integrand(p: Params, form: int, i, j, m, x, omega) -> np.ndarray:
    """The device's pointwise integrand per item (emme_integrand_batch), complex [n, k]: form 0: F; 1: F, F';
    2: A0, T, Q1, Q0, F; 3: W."""
    i, j, m = (np.ascontiguousarray(a, dtype=np.int32) for a in (i, j, m))
    x = np.ascontiguousarray(x, dtype=np.float64)
    w = np.ascontiguousarray(omega, dtype=np.complex128)
    n = len(x)
    if not (len(i) == len(j) == len(m) == len(w) == n):
        raise ValueError("i, j, m, x and omega need one entry per item")
    out = np.zeros((n, {0: 1, 1: 2, 2: 5, 3: 1}.get(form, 1)), dtype=np.complex128)
    _check(load().emme_integrand_batch(C.byref(p), form, n, i.ctypes.data, j.ctypes.data, m.ctypes.data, x.ctypes.data,
                                       w.ctypes.data, out.ctypes.data))
    return out


def null_vector(M) -> np.ndarray:
    """nullSpace (reference include/solver.h:58-112) of a complex symmetric matrix."""
    M = np.ascontiguousarray(M, dtype=np.complex128)
    v = np.zeros(M.shape[0], dtype=np.complex128)
    _check(load().emme_null_vector(M.ctypes.data, M.shape[0], v.ctypes.data))
    return v


def vector_parity(vecs) -> np.ndarray:
    """Share of every vector in the subspace that is even under the flip i -> n-1-i (emme_vector_parity, DESIGN.md
    §14.2): |v1 + J v2|^2 / (2 |v|^2), 1 for an even mode, 0 for an odd one; NaN for a zero or non-finite vector.  vecs:
    [nvec, n] or one vector [n], from any eigenpair entry point.  No device."""
    v = _c128(vecs)
    one = v.ndim == 1
    v = np.ascontiguousarray(v[None] if one else v)
    if v.ndim != 2 or v.shape[0] < 1 or v.shape[1] < 1:
        raise ValueError("vecs must be [nvec, n]")
    even = np.zeros(v.shape[0], dtype=np.float64)
    _check(load().emme_vector_parity(v.shape[1], v.shape[0], v.ctypes.data, even.ctypes.data))
    return even[0] if one else even


def contour_default(**kw) -> Contour:
    """emme_contour_default, then the given fields (center / semi_axes as complex or pairs)."""
    c = Contour()
    load().emme_contour_default(C.byref(c))
    for k, v in kw.items():
        if not hasattr(c, k):
            raise TypeError(f"unknown contour field {k!r}")
        if k in ("center", "semi_axes"):
            v = (v.real, v.imag) if isinstance(v, complex) else tuple(v)
            getattr(c, k)[0], getattr(c, k)[1] = float(v[0]), float(v[1])
        else:
            setattr(c, k, v)
    return c


def contour_eigs(A0, A1, rank_tol=None, max_eigs=64):
    """The Beyn step on moments A0, A1 (n x L): (eigenvalues mu of the reduced matrix, numerical rank k, the L
    singular values of A0).  rank_tol None: the emme_contour_t default."""
    A0 = np.ascontiguousarray(A0, dtype=np.complex128)
    A1 = np.ascontiguousarray(A1, dtype=np.complex128)
    if A0.ndim != 2 or A0.shape != A1.shape:
        raise ValueError("A0 and A1 must be n x L matrices of one shape")
    n, L = A0.shape
    if rank_tol is None:
        rank_tol = contour_default().rank_tol
    mu = np.zeros(max(max_eigs, 1), dtype=np.complex128)
    sig = np.zeros(L)
    k = C.c_int(0)
    _check(load().emme_contour_eigs(n, L, A0.ctypes.data, A1.ctypes.data, rank_tol, max_eigs, mu.ctypes.data,
                                    C.byref(k), sig.ctypes.data))
    return mu[:min(k.value, max_eigs)].copy(), k.value, sig


def scan_values(head, step, tail):
    """The values (and turning flags) one {head, step, tail} axis visits (src/main.cpp:139-172)."""
    if isinstance(tail, (list, tuple)):
        t0, t1 = tail
    else:
        t0, t1 = tail, head + 0.5 * np.copysign(step, head - tail)
    vals = np.zeros(100000)
    turn = np.zeros(100000, dtype=np.int32)
    n = load().emme_scan_values(head, step, t0, t1, vals.ctypes.data, turn.ctypes.data, len(vals))
    return vals[:n].copy(), turn[:n].copy()


def run_json(text: str, matrix_dir: str | None = None) -> dict:
    """The reference's main() on an input.json text (src/main.cpp:182-338); returns output.json."""
    import json
    out = C.c_void_p()
    rc = load().emme_run_json(text.encode(), matrix_dir.encode() if matrix_dir else None, C.byref(out))
    _check(rc)
    try:
        return json.loads(C.string_at(out).decode())
    finally:
        load().emme_free(out)


def run_json_lockstep(text: str, matrix_dir: str | None = None) -> dict:
    """run_json with the independent lines of the scan solved side by side (emme_run_json_lockstep):
    same output.json."""
    import json
    out = C.c_void_p()
    rc = load().emme_run_json_lockstep(text.encode(), matrix_dir.encode() if matrix_dir else None, C.byref(out))
    _check(rc)
    try:
        return json.loads(C.string_at(out).decode())
    finally:
        load().emme_free(out)


def scan_plan(text: str) -> dict:
    """The round plan of run_json_lockstep for an input.json text (host only): per point (axis by axis, each in
    scan_values order) its axis, index on the axis, round (-1 on a sequential axis) and pred (index of the point it
    continues from, -1: initial_guess); per axis whether the sequential driver runs it; the number of rounds."""
    lib = load()
    na, nr = C.c_int(0), C.c_int(0)
    n = lib.emme_scan_plan(text.encode(), 0, None, None, None, None, 0, None, C.byref(na), C.byref(nr))
    if n < 0:
        _check(n)
    axis, index, rnd, pred = (np.zeros(max(n, 1), dtype=np.int32) for _ in range(4))
    seq = np.zeros(max(na.value, 1), dtype=np.int32)
    n = lib.emme_scan_plan(text.encode(), n, axis.ctypes.data, index.ctypes.data, rnd.ctypes.data, pred.ctypes.data,
                           na.value, seq.ctypes.data, C.byref(na), C.byref(nr))
    if n < 0:
        _check(n)
    return {"axis": axis[:n].copy(), "index": index[:n].copy(), "round": rnd[:n].copy(), "pred": pred[:n].copy(),
            "sequential": seq[:na.value].astype(bool), "n_rounds": nr.value}


def params_same_shape(a: Params, b: Params) -> bool:
    """Can b be bound to a context made for a (emme_params_same_shape: npoints, beta_e == 0 alike,
    integration_start_points, iteration_method)?  last_error() names the first field that differs."""
    return load().emme_params_same_shape(C.byref(a), C.byref(b)) == 0


def last_error() -> str:
    return load().emme_last_error().decode()


def neighbour_sets(bases, names, rel_step=1e-4):
    """The parameter sets a root_sensitivities call needs (host only).  bases: one parameter dict or a list of them (all
    of one shape); names: the parameters to differentiate by.  Returns (params, set, set_plus, set_minus, dp): params is
    the list of Params to bind -- the bases first, then p (1 + rel_step) and p (1 - rel_step) per base and name (an
    absolute step of rel_step where p = 0; a whole step of at least 1 for an integer) -- set [nbases] the bases' indices,
    set_plus / set_minus [nbases, len(names)] those of the neighbours and dp [nbases, len(names)] = p+ - p- as the sets
    hold it.  A name that changes the shape (npoints, integration_start_points, iteration_method, a beta_e step across
    0: params_same_shape) is refused with a ValueError."""
    bases = [bases] if isinstance(bases, dict) else list(bases)
    names = list(names)
    if not bases:
        raise ValueError("neighbour_sets needs at least one base")
    params = [params_from_dict(d) for d in bases]
    for k, p in enumerate(params[1:]):
        if not params_same_shape(params[0], p):
            raise ValueError(f"base {k + 1} has another shape than base 0: {last_error()}")
    nb, nn = len(bases), len(names)
    set_plus = np.zeros((nb, nn), dtype=np.int32)
    set_minus = np.zeros((nb, nn), dtype=np.int32)
    dp = np.zeros((nb, nn), dtype=np.float64)
    for ib, d in enumerate(bases):
        for k, name in enumerate(names):
            if name not in d or isinstance(d[name], (str, bool, list, tuple, dict)):
                raise ValueError(f"{name!r} is not a numeric parameter of base {ib}")
            p = d[name]
            if isinstance(p, (int, np.integer)):
                h = max(1, int(round(abs(p) * rel_step)))
            else:
                h = abs(p) * rel_step if p != 0 else rel_step
            if name == "beta_e" and p != 0 and not (p - h) * (p + h) > 0:
                raise ValueError(f"a step of 'beta_e' from {p} crosses 0, where the shape changes (base {ib})")
            sides = []
            for sign in (1, -1):
                try:
                    q = params_from_dict({**d, name: p + sign * h})
                except EmmeError as e:
                    raise ValueError(f"a step of {name!r} gives no valid parameter set: {e.reason}") from e
                if not params_same_shape(params[ib], q):
                    raise ValueError(f"a step of {name!r} changes the shape of base {ib}: {last_error()}")
                sides.append(q)
            set_plus[ib, k], set_minus[ib, k] = len(params), len(params) + 1
            params += sides
            dp[ib, k] = float(p + h) - float(p - h)
    return params, np.arange(nb, dtype=np.int32), set_plus, set_minus, dp


def release_pooled_memory() -> None:
    """Give the node-cache buffers kept from destroyed contexts back to the driver."""
    load().emme_release_pooled_memory()


COMM_ID_BYTES = 128

# emme_ctx_set_tile_shapes (include/emme_hip.h)
TILE_SHAPES_ES15 = 0
TILE_SHAPES_ALL = 1
# emme_ctx_set_deriv_cache_shapes (include/emme_hip.h)
DERIV_CACHE_SHAPES_ES15 = 0
DERIV_CACHE_SHAPES_ALL = 1
# emme_ctx_set_mirror_shapes (include/emme_hip.h)
MIRROR_SHAPES_ES15 = 0
MIRROR_SHAPES_ALL = 1


def comm_available() -> bool:
    """Can RCCL be bound in this process?  Not a collective (see emme_comm_available)."""
    return load().emme_comm_available() == 0


def gather_pack(rank: int, world: int, roots, iters, info, n_total: int) -> np.ndarray:
    """emme_gather_pack: this rank's 4 m doubles of the all-gather (host only)."""
    lib = load()
    r = np.ascontiguousarray(roots, dtype=np.complex128)
    it = np.ascontiguousarray(iters, dtype=np.int32)
    inf = np.ascontiguousarray(info, dtype=np.int32)
    m = lib.emme_gather_slots(n_total, world)
    if m < 0:
        _check(m)
    send = np.zeros(4 * m)
    _check(lib.emme_gather_pack(rank, world, r.ctypes.data, it.ctypes.data, inf.ctypes.data, len(r), n_total,
                                send.ctypes.data))
    return send


def gather_unpack(world: int, n_total: int, allbuf):
    """emme_gather_unpack: the all-gather's world * 4 m doubles in item order (host only)."""
    a = np.ascontiguousarray(allbuf, dtype=np.float64)
    ra = np.zeros(n_total, dtype=np.complex128)
    ia = np.zeros(n_total, dtype=np.int32)
    fa = np.zeros(n_total, dtype=np.int32)
    _check(load().emme_gather_unpack(world, n_total, a.ctypes.data, ra.ctypes.data, ia.ctypes.data, fa.ctypes.data))
    return ra, ia, fa


def comm_unique_id() -> bytes:
    """ncclGetUniqueId through the C ABI (rank 0 calls it and hands the bytes to the others)."""
    buf = C.create_string_buffer(COMM_ID_BYTES)
    _check(load().emme_comm_unique_id(buf))
    return buf.raw


class Comm:
    """RCCL communicator of the scan's one collective (emme_comm_* in include/emme_hip.h)."""

    def __init__(self, unique_id: bytes, rank: int, world: int, device: int = -1):
        assert len(unique_id) == COMM_ID_BYTES
        self.lib = load()
        self.rank, self.world = rank, world
        h = C.c_void_p()
        _check(self.lib.emme_comm_create(unique_id, rank, world, device, C.byref(h)))
        self.h = h

    def close(self):
        if getattr(self, "h", None):
            self.lib.emme_comm_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def gather_roots(self, roots, iters, info, n_total: int, stream_handle: int = 0):
        """ONE ncclAllGather of {w_re, w_im, iters, info}; returns all n_total results in item
        order (item k was solved by rank k mod world) on every rank."""
        r = np.ascontiguousarray(roots, dtype=np.complex128)
        it = np.ascontiguousarray(iters, dtype=np.int32)
        inf = np.ascontiguousarray(info, dtype=np.int32)
        ra = np.zeros(n_total, dtype=np.complex128)
        ia = np.zeros(n_total, dtype=np.int32)
        fa = np.zeros(n_total, dtype=np.int32)
        _check(self.lib.emme_gather_roots(self.h, C.c_void_p(stream_handle), r.ctypes.data, it.ctypes.data,
                                          inf.ctypes.data, len(r), n_total, ra.ctypes.data, ia.ctypes.data,
                                          fa.ctypes.data))
        return ra, ia, fa


def _c128(a, shape=None):
    a = np.ascontiguousarray(a, dtype=np.complex128)
    return a if shape is None else a.reshape(shape)


def _operand_pair(A, B, a_device_ptr, b_device_ptr, copy=False):
    """The two matrix operands of a linear-algebra call as (pointer A, pointer B, nbatch, n, keep-alive): host arrays
    [nbatch, n, n] (or one [n, n] matrix each) as they are (copy: private copies, for a call that destroys them), or
    with a_device_ptr / b_device_ptr that operand in device memory -- then A = (nbatch, n) if both are, and the
    argument of the device operand is not looked at otherwise."""
    host = [None if p is not None else _c128(X) for X, p in ((A, a_device_ptr), (B, b_device_ptr))]
    host = [None if h is None else np.ascontiguousarray(h[None] if h.ndim == 2 else h) for h in host]
    if copy:
        host = [None if h is None else h.copy() for h in host]
    first = next((h for h in host if h is not None), None)
    nb, n = (first.shape[0], first.shape[1]) if first is not None else (int(A[0]), int(A[1]))
    for h in host:
        if h is not None and h.shape != (nb, n, n):
            raise ValueError("the operands must be [nbatch, n, n] of one shape")
    ptrs = [h.ctypes.data if h is not None else C.c_void_p(p) for h, p in zip(host, (a_device_ptr, b_device_ptr))]
    return ptrs[0], ptrs[1], nb, n, host


class Context:
    """One (device, parameter set): owns device tables and batch scratch."""

    def __init__(self, params: Params, device: int = -1, **options):
        """options: fields of emme_options_t (node_cache_gb, cache_min_batch, fill, lu_split, ...); lu_fold (0 / 1): the
        folded trace-secant step, which is a setter of the context (set_lu_fold); eigpair_fold (0 / 1): the folded secant
        eigenpair step, likewise (set_eigpair_fold); mirror_shapes (MIRROR_SHAPES_ES15 / MIRROR_SHAPES_ALL): which shapes
        mirror on a symmetric grid, likewise (set_mirror_shapes)."""
        self.lib = load()
        self.params = params
        h = C.c_void_p()
        lu_fold = options.pop("lu_fold", None)
        eigpair_fold = options.pop("eigpair_fold", None)
        mirror_shapes = options.pop("mirror_shapes", None)
        o = default_options(**options)
        _check(self.lib.emme_ctx_create_ex(C.byref(params), device, C.byref(o), C.byref(h)))
        self.h = h
        self.dim = self.lib.emme_ctx_dim(h)
        if lu_fold is not None:
            self.set_lu_fold(lu_fold)
        if eigpair_fold is not None:
            self.set_eigpair_fold(eigpair_fold)
        if mirror_shapes is not None:
            self.set_mirror_shapes(mirror_shapes)

    def options(self) -> Options:
        o = Options()
        _check(self.lib.emme_ctx_get_options(self.h, C.byref(o)))
        return o

    def set_options(self, **kw) -> None:
        o = self.options()
        for k, v in kw.items():
            if not hasattr(o, k):
                raise TypeError(f"unknown option {k!r}")
            setattr(o, k, v)
        _check(self.lib.emme_ctx_set_options(self.h, C.byref(o)))

    def set_tile_shapes(self, shapes: int) -> None:
        """Which shapes the option tile_uncached serves: TILE_SHAPES_ES15 (default: electrostatic GK15 only) or
        TILE_SHAPES_ALL (electromagnetic and GK31 contexts as well: k_assemble_tile_shape, and for calls over bound
        parameter sets k_assemble_tile_shape_sets, fill mode 7).  From the next call on."""
        _check(self.lib.emme_ctx_set_tile_shapes(self.h, int(shapes)))

    def set_deriv_cache_shapes(self, shapes: int) -> None:
        """Which shapes the option deriv_cached sends through the node cache: DERIV_CACHE_SHAPES_ES15 (default:
        electrostatic GK15 only) or DERIV_CACHE_SHAPES_ALL (electromagnetic and GK31 contexts with the tiled cache as
        well: k_assemble_dense_shape_deriv).  No effect while deriv_cached = 0.  From the next call on."""
        _check(self.lib.emme_ctx_set_deriv_cache_shapes(self.h, int(shapes)))

    def deriv_cache_shapes(self) -> int:
        v = self.lib.emme_ctx_get_deriv_cache_shapes(self.h)
        if v < 0:
            _check(v)
        return v

    def tile_shapes(self) -> int:
        v = self.lib.emme_ctx_get_tile_shapes(self.h)
        if v < 0:
            _check(v)
        return v

    def set_mirror_pairs(self, on: bool) -> None:
        """Fill one pair of every mirror-image couple (i, j) / (N-1-j, N-1-i) on symmetric grids (DESIGN.md §5.0c;
        default on; electrostatic GK15 on the tiled cache, other shapes under set_mirror_shapes).  A layout setting: rejected once the node cache exists."""
        _check(self.lib.emme_ctx_set_mirror_pairs(self.h, 1 if on else 0))

    def set_mirror_shapes(self, shapes: int) -> None:
        """Which shapes mirror on a symmetric grid: MIRROR_SHAPES_ES15 (default: electrostatic GK15 only) or
        MIRROR_SHAPES_ALL (electromagnetic and GK31 contexts on the tiled cache as well).  A layout
        setting: rejected once the node cache exists."""
        _check(self.lib.emme_ctx_set_mirror_shapes(self.h, int(shapes)))

    def mirror_shapes(self) -> int:
        v = self.lib.emme_ctx_get_mirror_shapes(self.h)
        if v < 0:
            _check(v)
        return v

    def set_lu_fold(self, on) -> None:
        """The folded trace-secant step (default on): steps of solve_roots whose two fills ran mirrored,
        on an even order, factor the even and the odd block instead of the matrix.  0: the unfolded step bit for bit."""
        _check(self.lib.emme_ctx_set_lu_fold(self.h, int(on)))

    def lu_fold(self) -> int:
        v = self.lib.emme_ctx_get_lu_fold(self.h)
        if v < 0:
            _check(v)
        return v

    def last_folded_steps(self) -> int:
        """Steps of the last root search that ran folded."""
        return self.lib.emme_ctx_last_folded_steps(self.h)

    def trace_secant_folded(self, M, M_old, domega, device_ptrs=None):
        """tr(M_b^-1 (M_b - M_old_b) / domega_b) and info per item by the folded step (emme_trace_secant_folded_batch)
        for symmetric matrices that are centrosymmetric apart from their last row and column.  device_ptrs = (M, M_old,
        domega, tr, info) device addresses: all five operands in device memory, M = (nbatch, n); returns None then."""
        if device_ptrs is not None:
            nb, n = int(M[0]), int(M[1])
            _check(self.lib.emme_trace_secant_folded_batch(self.h, n, nb, *[C.c_void_p(int(p)) for p in device_ptrs]))
            return None
        M = _c128(M)
        M = np.ascontiguousarray(M[None] if M.ndim == 2 else M)
        Mo = _c128(M_old, M.shape)
        nb, n = M.shape[0], M.shape[1]
        dw = _c128(np.broadcast_to(np.asarray(domega, dtype=np.complex128), (nb,)))
        tr = np.zeros(nb, dtype=np.complex128)
        info = np.zeros(nb, dtype=np.int32)
        _check(self.lib.emme_trace_secant_folded_batch(self.h, n, nb, M.ctypes.data, Mo.ctypes.data, dw.ctypes.data,
                                                       tr.ctypes.data, info.ctypes.data))
        return tr, info

    def mirror_pairs(self) -> int:
        """1 if the node cache is (or, before it exists, would be) laid out over the half pair list."""
        v = self.lib.emme_ctx_get_mirror_pairs(self.h)
        if v < 0:
            _check(v)
        return v

    def close(self):
        if getattr(self, "h", None):
            self.lib.emme_ctx_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def __enter__(self):
        return self

    def __exit__(self, *a):
        self.close()

    def set_stream(self, stream_handle: int):
        _check(self.lib.emme_ctx_set_stream(self.h, C.c_void_p(stream_handle)))

    FILL_KERNELS = {0: "k_assemble (lanes=nodes)", 1: "k_assemble_wl (omega-lane)",
                    2: "k_assemble_cached (HBM node cache)",
                    3: "k_assemble_union (HBM node cache + phase table)",
                    4: "k_assemble_dense (tiled HBM node cache + weighted phase tables, FP64 matrix cores)",
                    5: "k_assemble_tile (table-free tile fill, FP64 matrix cores)"}
    # fill mode 6 (emme_assemble_sets_batch / emme_solve_roots_sets): not a kernel family of the plain fills above
    SETS_FILL_KERNEL = "k_assemble_sets (lanes=nodes, a parameter set per item)"
    # fill mode 7: at least one (set, contour class) group of the call went through the tile fill over sets
    TILE_SETS_FILL_KERNEL = "k_assemble_tile_sets (table-free tile fill, a parameter set per chunk)"

    def fill_kernel(self) -> str:
        mode = self.lib.emme_ctx_fill_mode(self.h)
        if mode == 7:
            return self.TILE_SETS_FILL_KERNEL
        return self.SETS_FILL_KERNEL if mode == 6 else self.FILL_KERNELS.get(mode, "none yet")

    def last_deferred(self) -> int:
        """Integrals the last fill handed to its work list (finished from scratch by a second launch)."""
        n = self.lib.emme_ctx_last_deferred(self.h)
        if n < 0:
            _check(int(n))
        return int(n)

    def fill_kernel_symbol(self) -> str:
        """Name of the last fill's main kernel as rocprofv3 prints it (key of profiles/*_pmc_summary.json)."""
        mode = self.lib.emme_ctx_fill_mode(self.h)
        pts = self.params.integration_start_points
        em = self.params.beta_e != 0.0
        o = self.options()
        folded = "true" if o.phase_table else "false"
        if mode == 4:
            if pts == 15 and not em and not o.dense_stage:
                return "k_assemble_dense<-1, 15, 1>"  # (without the LDS operand stage)
            return "k_assemble_dense<1, %d, %d>" % (pts, 3 if em else 1)
        if mode == 5:
            if em or pts != 15:
                return "k_assemble_tile_shape<%d, %d>" % (pts, 3 if em else 1)
            return "k_assemble_tile"
        if mode == 3:
            return "k_assemble_union<15, %d>" % o.union_sel
        if mode == 2:
            return f"k_assemble_cached_em<{pts}, {folded}>" if em else f"k_assemble_cached<{pts}, {folded}>"
        if mode == 1:
            return f"k_assemble_wl<{pts}>"
        if mode == 6:
            return f"k_assemble_sets<{pts}>"
        if mode == 7:
            if em or pts != 15:
                return "k_assemble_tile_shape_sets<%d, %d>" % (pts, 3 if em else 1)
            return "k_assemble_tile_sets"
        return f"k_assemble<{pts}, false>"

    def linstep_kernel_symbol(self) -> str:
        """Name of the kernel of the context's last LU launch as rocprofv3 prints it ("" before the first): after a
        trace step k_trace_solve_blocked<false, false> (one workgroup per matrix), k_trace_solve_blocked<true, false>
        (several), k_trace_solve_grouped, k_trace_solve_blocked<true, true> (chunked panel) or k_trace_solve (unblocked);
        after the factorisation behind null vectors, eigenpair steps and contour moments k_lu_inplace,
        k_trace_solve_blocked<true, true> or k_lu_unblocked_inplace.  What was launched, not what was asked for."""
        s = self.lib.emme_ctx_linstep_kernel_symbol(self.h)
        if s is None:
            _check(-1)
        return s.decode()

    def last_lu_workgroups(self) -> int:
        """Workgroups per matrix of that launch."""
        return self.lib.emme_ctx_last_lu_workgroups(self.h)

    def last_lu_slices(self) -> int:
        """Launches the last batched factorisation was cut into (1 after a trace step)."""
        return self.lib.emme_ctx_last_lu_slices(self.h)

    def compute_units(self) -> int:
        """Compute units of the context's device (its properties' multiProcessorCount)."""
        return self.lib.emme_ctx_compute_units(self.h)

    def node_cache_gib(self) -> float:
        return self.lib.emme_ctx_node_cache_gib(self.h)

    def cache_settle(self, omegas) -> int:
        """Grow the node cache to its final shape for these omegas (the canonical state); returns
        the number of fills it took."""
        w = _c128(np.atleast_1d(omegas))
        n = C.c_int(0)
        _check(self.lib.emme_ctx_cache_settle(self.h, w.ctypes.data, w.shape[0], C.byref(n)))
        return n.value

    def cache_state(self):
        """(depth of the fully cached tree, cached subtrees, GiB held)."""
        d, k, g = C.c_int(0), C.c_int(0), C.c_double(0)
        _check(self.lib.emme_ctx_cache_state(self.h, C.byref(d), C.byref(k), C.byref(g)))
        return d.value, k.value, g.value

    def profile(self, on=True):
        _check(self.lib.emme_ctx_profile_enable(self.h, int(on)))

    def profile_read(self, reset=False) -> Profile:
        pr = Profile()
        _check(self.lib.emme_ctx_profile_read(self.h, C.byref(pr), int(reset)))
        return pr

    # matrixAssembler (include/solver.h:417-515), batched over omega
    def assemble(self, omegas, out_device_ptr: int | None = None, want_intervals=False):
        w = _c128(np.atleast_1d(omegas))
        nb = w.shape[0]
        iv = np.zeros(nb, dtype=np.int64)
        if out_device_ptr is None:
            M = np.zeros((nb, self.dim, self.dim), dtype=np.complex128)
            _check(self.lib.emme_assemble_batch(self.h, w.ctypes.data, nb, M.ctypes.data,
                                                iv.ctypes.data))
            return (M, iv) if want_intervals else M
        _check(self.lib.emme_assemble_batch(self.h, w.ctypes.data, nb,
                                            C.c_void_p(out_device_ptr), iv.ctypes.data))
        return iv

    def assemble_derivative(self, omegas, want_intervals=False, omega_device_ptr: int | None = None,
                            out_device_ptr: int | None = None, mp_device_ptr: int | None = None):
        """M(omega) and the exact M'(omega) of the same quadrature trees, through the uncached kernels
        (option deriv_cached = 1: through the node cache where the context has the tiled one; with tile_uncached = 1
        as well, through the table-free tile fill where there is no cache to read): returns (M, Mp[, intervals]).
        omega_device_ptr: the omegas in device memory (omegas is then the batch size); out_device_ptr / mp_device_ptr:
        M / Mp go to device memory (the header wants both on one side) and come back as None."""
        if omega_device_ptr is not None:
            nb, wp = int(omegas), C.c_void_p(omega_device_ptr)
        else:
            w = _c128(np.atleast_1d(omegas))
            nb, wp = w.shape[0], w.ctypes.data
        iv = np.zeros(nb, dtype=np.int64)
        M = np.zeros((nb, self.dim, self.dim), dtype=np.complex128) if out_device_ptr is None else None
        Mp = np.zeros((nb, self.dim, self.dim), dtype=np.complex128) if mp_device_ptr is None else None
        _check(self.lib.emme_assemble_derivative_batch(self.h, wp, nb,
                                                       M.ctypes.data if M is not None else C.c_void_p(out_device_ptr),
                                                       Mp.ctypes.data if Mp is not None else C.c_void_p(mp_device_ptr),
                                                       iv.ctypes.data))
        return (M, Mp, iv) if want_intervals else (M, Mp)

    def assemble_rc(self, omegas) -> int:
        """emme_assemble_batch's return code alone (0, or EMME_ENUMERIC when a matrix holds a non-finite integral)."""
        w = _c128(np.atleast_1d(omegas))
        M = np.zeros((w.shape[0], self.dim, self.dim), dtype=np.complex128)
        return self.lib.emme_assemble_batch(self.h, w.ctypes.data, w.shape[0], M.ctypes.data, None)

    def assemble_raw(self, omegas, set=None):
        """emme_assemble_batch (set given: emme_assemble_sets_batch on the bound sets set[b]) without raising on its
        return code: (rc, M, intervals).  The library copies every matrix and interval count out before it returns
        EMME_ENUMERIC, so the items beside a lost one are there to be read."""
        w = _c128(np.atleast_1d(omegas))
        nb = w.shape[0]
        M = np.zeros((nb, self.dim, self.dim), dtype=np.complex128)
        iv = np.zeros(nb, dtype=np.int64)
        if set is None:
            rc = self.lib.emme_assemble_batch(self.h, w.ctypes.data, nb, M.ctypes.data, iv.ctypes.data)
        else:
            st = np.ascontiguousarray(np.atleast_1d(set), dtype=np.int32)
            if st.shape[0] != nb:
                raise ValueError("set needs one entry per omega")
            rc = self.lib.emme_assemble_sets_batch(self.h, st.ctypes.data, w.ctypes.data, nb, M.ctypes.data, None,
                                                   iv.ctypes.data)
        return rc, M, iv

    def assemble_derivative_raw(self, omegas, set=None):
        """The derivative twin of assemble_raw (emme_assemble_derivative_batch, or emme_assemble_sets_batch with Mp):
        (rc, M, Mp, intervals)."""
        w = _c128(np.atleast_1d(omegas))
        nb = w.shape[0]
        M = np.zeros((nb, self.dim, self.dim), dtype=np.complex128)
        Mp = np.zeros((nb, self.dim, self.dim), dtype=np.complex128)
        iv = np.zeros(nb, dtype=np.int64)
        if set is None:
            rc = self.lib.emme_assemble_derivative_batch(self.h, w.ctypes.data, nb, M.ctypes.data, Mp.ctypes.data,
                                                         iv.ctypes.data)
        else:
            st = np.ascontiguousarray(np.atleast_1d(set), dtype=np.int32)
            if st.shape[0] != nb:
                raise ValueError("set needs one entry per omega")
            rc = self.lib.emme_assemble_sets_batch(self.h, st.ctypes.data, w.ctypes.data, nb, M.ctypes.data,
                                                   Mp.ctypes.data, iv.ctypes.data)
        return rc, M, Mp, iv

    def trace_solve(self, A, B, a_device_ptr: int | None = None, b_device_ptr: int | None = None):
        """tr(A_b^-1 B_b) and info per item (emme_trace_solve_batch) on private copies of A and B; a_device_ptr /
        b_device_ptr: that operand in device memory, where the call destroys it (both: A = (nbatch, n))."""
        pa, pb, nb, n, _keep = _operand_pair(A, B, a_device_ptr, b_device_ptr, copy=True)
        tr = np.zeros(nb, dtype=np.complex128)
        info = np.zeros(nb, dtype=np.int32)
        _check(self.lib.emme_trace_solve_batch(self.h, n, nb, pa, pb, tr.ctypes.data, info.ctypes.data))
        return tr, info

    # the linear algebra of newtonQRSecantIteration (include/solver.h:244-370): q with
    # domega = -1/q, for arbitrary square A (= M) and B (= M')
    def qr_secant(self, A, B, a_device_ptr: int | None = None, b_device_ptr: int | None = None):
        """(a_device_ptr / b_device_ptr: that operand in device memory; both: A = (nbatch, n))"""
        pa, pb, nb, n, _keep = _operand_pair(A, B, a_device_ptr, b_device_ptr)
        q = np.zeros(nb, dtype=np.complex128)
        info = np.zeros(nb, dtype=np.int32)
        _check(self.lib.emme_qr_secant_batch(self.h, n, nb, pa, pb, q.ctypes.data, info.ctypes.data))
        return q, info

    # newtonTraceSecantIteration / newtonQRSecantIteration (include/solver.h:113-160, 210-383),
    # batched; method: 0 trace-secant, 1 QR-secant
    def newton_step(self, omegas, M, Mp, method=0, omega_device_ptr: int | None = None,
                    domega_device_ptr: int | None = None, m_device_ptr: int | None = None,
                    mp_device_ptr: int | None = None, info_device_ptr: int | None = None):
        """Returns (omega, domega, M, Mp, info) after the step.  *_device_ptr: that array in device memory, updated in
        place (the header wants all five on one side) -- its argument is not looked at and it comes back as None;
        with omega_device_ptr, omegas is the batch size."""
        if omega_device_ptr is not None:
            w, nb = None, int(omegas)
        else:
            w = _c128(np.atleast_1d(omegas)).copy()
            nb = w.shape[0]
        M = None if m_device_ptr is not None else _c128(M, (nb, self.dim, self.dim)).copy()
        Mp = None if mp_device_ptr is not None else _c128(Mp, (nb, self.dim, self.dim)).copy()
        dw = None if domega_device_ptr is not None else np.zeros(nb, dtype=np.complex128)
        info = None if info_device_ptr is not None else np.zeros(nb, dtype=np.int32)
        p = [a.ctypes.data if a is not None else C.c_void_p(d)
             for a, d in ((w, omega_device_ptr), (dw, domega_device_ptr), (M, m_device_ptr), (Mp, mp_device_ptr),
                          (info, info_device_ptr))]
        _check(self.lib.emme_newton_step_batch(self.h, p[0], p[1], nb, p[2], p[3], method, p[4]))
        return w, dw, M, Mp, info

    # solve_once_eigen (src/main.cpp:19-80), batched over initial guesses
    def solve_roots(self, guesses, tol=None, step_limit=None, want_iterates=False):
        g = _c128(np.atleast_1d(guesses))
        n = g.shape[0]
        tol = self.params.iteration_precision if tol is None else tol
        step_limit = self.params.iteration_step_limit if step_limit is None else step_limit
        roots = np.zeros(n, dtype=np.complex128)
        iters = np.zeros(n, dtype=np.int32)
        info = np.zeros(n, dtype=np.int32)
        its = np.zeros((n, step_limit + 1), dtype=np.complex128) if want_iterates else None
        _check(self.lib.emme_solve_roots(self.h, g.ctypes.data, n, tol, step_limit,
                                         roots.ctypes.data, iters.ctypes.data, info.ctypes.data,
                                         its.ctypes.data if want_iterates else None))
        return (roots, iters, info, its) if want_iterates else (roots, iters, info)

    def solve_roots_newton(self, guesses, tol=None, step_limit=None, want_iterates=False):
        """solve_roots with the exact M' (emme_solve_roots_newton): starts at the guesses themselves."""
        g = _c128(np.atleast_1d(guesses))
        n = g.shape[0]
        tol = self.params.iteration_precision if tol is None else tol
        step_limit = self.params.iteration_step_limit if step_limit is None else step_limit
        roots = np.zeros(n, dtype=np.complex128)
        iters = np.zeros(n, dtype=np.int32)
        info = np.zeros(n, dtype=np.int32)
        its = np.zeros((n, step_limit + 1), dtype=np.complex128) if want_iterates else None
        _check(self.lib.emme_solve_roots_newton(self.h, g.ctypes.data, n, tol, step_limit, roots.ctypes.data,
                                                iters.ctypes.data, info.ctypes.data,
                                                its.ctypes.data if want_iterates else None))
        return (roots, iters, info, its) if want_iterates else (roots, iters, info)

    # ---- parameter sets: many sets on one context ----
    def bind_param_sets(self, sets) -> None:
        """Bind parameter sets (a list of Params of this context's shape, params_same_shape) to the context; an empty
        list unbinds.  Items of assemble_sets / solve_roots_sets name them by position."""
        sets = list(sets)
        arr = (Params * max(len(sets), 1))(*sets)
        _check(self.lib.emme_ctx_bind_param_sets(self.h, C.cast(arr, C.c_void_p), len(sets)))

    def param_sets(self) -> int:
        return self.lib.emme_ctx_param_sets(self.h)

    def assemble_sets(self, set, omegas, want_derivative=False, want_intervals=False,
                      omega_device_ptr: int | None = None, out_device_ptr: int | None = None,
                      mp_device_ptr: int | None = None):
        """M(omega_b) of the bound parameter set set[b], one launch for the batch: returns M[, Mp][, intervals]
        (Mp: the exact dM/domega of the same quadrature trees).  omega_device_ptr: the omegas in device memory (omegas is
        not looked at); out_device_ptr / mp_device_ptr: M / Mp go to device memory and come back as None
        (mp_device_ptr asks for the derivative)."""
        st = np.ascontiguousarray(np.atleast_1d(set), dtype=np.int32)
        nb = st.shape[0]
        if omega_device_ptr is not None:
            wp = C.c_void_p(omega_device_ptr)
        else:
            w = _c128(np.atleast_1d(omegas))
            wp = w.ctypes.data
            if w.shape[0] != nb:
                raise ValueError("set needs one entry per omega")
        want_derivative = want_derivative or mp_device_ptr is not None
        iv = np.zeros(nb, dtype=np.int64)
        M = np.zeros((nb, self.dim, self.dim), dtype=np.complex128) if out_device_ptr is None else None
        Mp = np.zeros((nb, self.dim, self.dim), dtype=np.complex128) if want_derivative and mp_device_ptr is None else None
        mpp = C.c_void_p(mp_device_ptr) if mp_device_ptr is not None else (Mp.ctypes.data if want_derivative else None)
        _check(self.lib.emme_assemble_sets_batch(self.h, st.ctypes.data, wp, nb,
                                                 M.ctypes.data if M is not None else C.c_void_p(out_device_ptr), mpp,
                                                 iv.ctypes.data))
        out = (M, Mp) if want_derivative else (M,)
        if want_intervals:
            out = out + (iv,)
        return out[0] if len(out) == 1 else out

    def solve_roots_sets(self, set, guesses, exact=False, tol=None, step_limit=None, want_iterates=False):
        """solve_roots (exact=False) or solve_roots_newton (exact=True) with chain b on the bound parameter set
        set[b]; tol and step_limit (default: this context's own parameters) hold for every chain."""
        g = _c128(np.atleast_1d(guesses))
        n = g.shape[0]
        st = np.ascontiguousarray(np.atleast_1d(set), dtype=np.int32)
        if st.shape[0] != n:
            raise ValueError("set needs one entry per guess")
        tol = self.params.iteration_precision if tol is None else tol
        step_limit = self.params.iteration_step_limit if step_limit is None else step_limit
        roots = np.zeros(n, dtype=np.complex128)
        iters = np.zeros(n, dtype=np.int32)
        info = np.zeros(n, dtype=np.int32)
        its = np.zeros((n, step_limit + 1), dtype=np.complex128) if want_iterates else None
        _check(self.lib.emme_solve_roots_sets(self.h, st.ctypes.data, g.ctypes.data, n, int(bool(exact)), tol, step_limit,
                                              roots.ctypes.data, iters.ctypes.data, info.ctypes.data,
                                              its.ctypes.data if want_iterates else None))
        return (roots, iters, info, its) if want_iterates else (roots, iters, info)

    # ---- Newton on the eigenpair ----
    def solve_eigenpairs(self, guesses, set=None, v0=None, tol=None, step_limit=None, want_iterates=False, secant=False):
        """Newton on (omega, v) from omega_0 = guesses (emme_solve_eigenpairs): one LU without right-hand sides per step,
        and the unit eigenvector and the residual |M v| / |M|_F come with the root.  set: chain b on the bound parameter
        set set[b]; v0 [n, dim]: start vectors (default: from M(omega_0)^-1 s).  secant=True: the secant reading
        (emme_solve_eigenpairs_secant) -- bootstrapped at 0.99 g and g as solve_roots, one plain fill per step, no
        derivative fill.  Returns (roots, vecs, resid, iters, info[, iterates]); info = 0 also for a chain that used
        every step -- resid tells."""
        g = _c128(np.atleast_1d(guesses))
        n = g.shape[0]
        st = None
        if set is not None:
            st = np.ascontiguousarray(np.atleast_1d(set), dtype=np.int32)
            if st.shape[0] != n:
                raise ValueError("set needs one entry per guess")
        if v0 is not None:
            v0 = np.ascontiguousarray(_c128(v0))
            if v0.shape != (n, self.dim):
                raise ValueError("v0 must be [len(guesses), dim]")
        tol = self.params.iteration_precision if tol is None else tol
        step_limit = self.params.iteration_step_limit if step_limit is None else step_limit
        roots = np.zeros(n, dtype=np.complex128)
        vecs = np.zeros((n, self.dim), dtype=np.complex128)
        resid = np.zeros(n, dtype=np.float64)
        iters = np.zeros(n, dtype=np.int32)
        info = np.zeros(n, dtype=np.int32)
        its = np.zeros((n, step_limit + 1), dtype=np.complex128) if want_iterates else None
        search = self.lib.emme_solve_eigenpairs_secant if secant else self.lib.emme_solve_eigenpairs
        _check(search(self.h, st.ctypes.data if st is not None else None, g.ctypes.data, n,
                      v0.ctypes.data if v0 is not None else None, tol, step_limit, roots.ctypes.data, vecs.ctypes.data,
                      resid.ctypes.data, iters.ctypes.data, info.ctypes.data, its.ctypes.data if want_iterates else None))
        return (roots, vecs, resid, iters, info, its) if want_iterates else (roots, vecs, resid, iters, info)

    def eigenpair_secant_step(self, M, M_old, domega, v=None, m_device_ptr: int | None = None,
                              m_old_device_ptr: int | None = None):
        """One secant eigenpair step on caller matrices (emme_eigenpair_secant_step_batch): u = M^-1 (M - M_old) v /
        domega with the difference taken per entry, tau = v^H u (the next domega = -1/tau), resid = |M v| / |M|_F before
        the step.  domega [nbatch]: the step between the two fills.  v None: as eigenpair_step.  Returns (u / |u|, tau,
        resid, info).  m_device_ptr / m_old_device_ptr: that matrix operand in device memory (both: M = (nbatch, n))."""
        pm, pmo, nb, n, _keep = _operand_pair(M, M_old, m_device_ptr, m_old_device_ptr)
        dw = np.ascontiguousarray(_c128(np.atleast_1d(domega)))
        if dw.shape != (nb,):
            raise ValueError("domega needs one entry per matrix")
        if v is None:
            vv = np.zeros((nb, n), dtype=np.complex128)
        else:
            vv = np.array(_c128(v), dtype=np.complex128, order="C", copy=True).reshape(-1, n)
            if vv.shape != (nb, n):
                raise ValueError("v must be [nbatch, n]")
        tau = np.zeros(nb, dtype=np.complex128)
        resid = np.zeros(nb, dtype=np.float64)
        info = np.zeros(nb, dtype=np.int32)
        _check(self.lib.emme_eigenpair_secant_step_batch(self.h, n, nb, pm, pmo, dw.ctypes.data,
                                                         vv.ctypes.data, 0 if v is None else 1, tau.ctypes.data,
                                                         resid.ctypes.data, info.ctypes.data))
        return vv, tau, resid, info

    def set_eigpair_fold(self, on) -> None:
        """The folded secant eigenpair step (default off): steps of solve_eigenpairs(secant=True) and of
        find_eigenpairs_in_contour(exact=False)'s polish whose two fills ran mirrored, on an even order, factor the even
        and the odd block instead of the matrix.  0: every step is the unfolded one, bit for bit."""
        _check(self.lib.emme_ctx_set_eigpair_fold(self.h, int(on)))

    def eigpair_fold(self) -> int:
        v = self.lib.emme_ctx_get_eigpair_fold(self.h)
        if v < 0:
            _check(v)
        return v

    def last_folded_eigpair_steps(self) -> int:
        """Steps of the last eigenpair search that ran folded."""
        return self.lib.emme_ctx_last_folded_eigpair_steps(self.h)

    def eigenpair_secant_folded_step(self, M, M_old, domega, v, device_ptrs=None):
        """One folded secant eigenpair step (emme_eigenpair_secant_folded_step_batch) on symmetric matrices of even order
        that are centrosymmetric apart from their last row and column; v [nbatch, n]: the unit vectors (required).
        Returns (u / |u|, tau, resid, info) as eigenpair_secant_step.  device_ptrs = (M, M_old) device addresses: both
        matrix operands in device memory, M = (nbatch, n)."""
        if device_ptrs is not None:
            nb, n = int(M[0]), int(M[1])
            pm, pmo = (C.c_void_p(int(p)) for p in device_ptrs)
        else:
            pm, pmo, nb, n, _keep = _operand_pair(M, M_old, None, None)
        dw = np.ascontiguousarray(_c128(np.atleast_1d(domega)))
        if dw.shape != (nb,):
            raise ValueError("domega needs one entry per matrix")
        vv = np.array(_c128(v), dtype=np.complex128, order="C", copy=True).reshape(-1, n)
        if vv.shape != (nb, n):
            raise ValueError("v must be [nbatch, n]")
        tau = np.zeros(nb, dtype=np.complex128)
        resid = np.zeros(nb, dtype=np.float64)
        info = np.zeros(nb, dtype=np.int32)
        _check(self.lib.emme_eigenpair_secant_folded_step_batch(self.h, n, nb, pm, pmo, dw.ctypes.data, vv.ctypes.data,
                                                                tau.ctypes.data, resid.ctypes.data, info.ctypes.data))
        return vv, tau, resid, info

    def eigenpair_step(self, M, Mp, v=None, m_device_ptr: int | None = None, mp_device_ptr: int | None = None):
        """One eigenpair step on caller matrices (emme_eigenpair_step_batch): u = M^-1 Mp v, tau = v^H u (domega = -1/tau),
        resid = |M v| / |M|_F before the step.  v None: the step starts from M^-1 s / |M^-1 s| (include/emme_hip.h).
        Returns (u / |u|, tau, resid, info).  m_device_ptr / mp_device_ptr: that matrix operand in device memory (both:
        M = (nbatch, n))."""
        pm, pmp, nb, n, _keep = _operand_pair(M, Mp, m_device_ptr, mp_device_ptr)
        if v is None:
            vv = np.zeros((nb, n), dtype=np.complex128)
        else:
            vv = np.array(_c128(v), dtype=np.complex128, order="C", copy=True).reshape(-1, n)
            if vv.shape != (nb, n):
                raise ValueError("v must be [nbatch, n]")
        tau = np.zeros(nb, dtype=np.complex128)
        resid = np.zeros(nb, dtype=np.float64)
        info = np.zeros(nb, dtype=np.int32)
        _check(self.lib.emme_eigenpair_step_batch(self.h, n, nb, pm, pmp, vv.ctypes.data,
                                                  0 if v is None else 1, tau.ctypes.data, resid.ctypes.data,
                                                  info.ctypes.data))
        return vv, tau, resid, info

    # ---- root sensitivities from eigenpairs ----
    def sym_forms(self, A, B, vecs, a, b=None, x=None, y=None, a_device_ptr: int | None = None,
                  b_device_ptr: int | None = None):
        """Bilinear forms on matrix differences (emme_sym_forms_batch): per item t, form[t] = x^T (A_a - B_b) y (plain
        transpose) and fro2[t] = |A_a - B_b|_F^2, the difference taken per entry before the product.  A, B: [nmat, n, n]
        (B None: no second matrix); vecs [nvec, n]; a, b (None, or -1 per item: none), x (None: item t takes vector t),
        y (None: y = x): index lists.  a_device_ptr / b_device_ptr: the matrices in device memory, A = (nmat, n).
        Returns (form [nitems] complex, fro2 [nitems])."""
        if a_device_ptr is not None:
            nmat, n = int(A[0]), int(A[1])
            pa = C.c_void_p(a_device_ptr)
            pb = C.c_void_p(b_device_ptr) if b_device_ptr is not None else None
            keep = None
        else:
            Ah = _c128(A)
            Ah = np.ascontiguousarray(Ah[None] if Ah.ndim == 2 else Ah)
            nmat, n = Ah.shape[0], Ah.shape[1]
            Bh = None
            if B is not None:
                Bh = _c128(B)
                Bh = np.ascontiguousarray(Bh[None] if Bh.ndim == 2 else Bh)
                if Bh.shape != Ah.shape:
                    raise ValueError("A and B must be [nmat, n, n] of one shape")
            pa, pb, keep = Ah.ctypes.data, (Bh.ctypes.data if Bh is not None else None), (Ah, Bh)
        v = np.ascontiguousarray(_c128(vecs)).reshape(-1, n)
        ia = np.ascontiguousarray(np.atleast_1d(a), dtype=np.int32)
        nitems = ia.shape[0]
        lists = []
        for idx, default in ((b, None), (x, np.arange(nitems)), (y, None)):
            idx = default if idx is None else idx
            if idx is not None:
                idx = np.ascontiguousarray(np.atleast_1d(idx), dtype=np.int32)
                if idx.shape != (nitems,):
                    raise ValueError("a, b, x and y need one entry per item")
            lists.append(idx)
        ib, ix, iy = lists
        form = np.zeros(nitems, dtype=np.complex128)
        fro2 = np.zeros(nitems, dtype=np.float64)
        _check(self.lib.emme_sym_forms_batch(self.h, n, nmat, pa, pb, v.shape[0], v.ctypes.data, nitems, ia.ctypes.data,
                                             ib.ctypes.data if ib is not None else None, ix.ctypes.data,
                                             iy.ctypes.data if iy is not None else None, form.ctypes.data,
                                             fro2.ctypes.data))
        del keep
        return form, fro2

    def root_sensitivities(self, set, roots, vecs, set_plus, set_minus, dp, max_items=0):
        """d omega / d p of eigenpairs over bound parameter sets (emme_root_sensitivities_sets): root r is the eigenpair
        (roots[r], vecs[r]) of bound set set[r], as solve_eigenpairs(set=...) and find_eigenpairs_in_contours_sets return
        it; direction k is the pair of bound sets set_plus[r, k], set_minus[r, k] at parameter distance dp[r, k]
        (neighbour_sets builds all of it).  Returns (dwdp [nroots, ndir], denom, corr, cond, info): denom = v^T M' v,
        corr = -v^T M v / denom (first-order distance to the root), cond = |M|_F |v|^2 / |denom|; info 0, 1 (denom at
        its rounding level) or EMME_ENUMERIC (a NaN eigenpair or a failed base fill) per root."""
        st = np.ascontiguousarray(np.atleast_1d(set), dtype=np.int32)
        nr = st.shape[0]
        w = np.ascontiguousarray(_c128(np.atleast_1d(roots)))
        v = np.ascontiguousarray(_c128(vecs)).reshape(-1, self.dim)
        if w.shape != (nr,) or v.shape != (nr, self.dim):
            raise ValueError("roots must be [len(set)] and vecs [len(set), dim]")
        sp = np.ascontiguousarray(set_plus, dtype=np.int32).reshape(nr, -1)
        sm = np.ascontiguousarray(set_minus, dtype=np.int32).reshape(nr, -1)
        d = np.ascontiguousarray(dp, dtype=np.float64).reshape(nr, -1)
        ndir = sp.shape[1]
        if sm.shape != (nr, ndir) or d.shape != (nr, ndir):
            raise ValueError("set_plus, set_minus and dp must be [len(set), ndir]")
        dwdp = np.zeros((nr, ndir), dtype=np.complex128)
        denom = np.zeros(nr, dtype=np.complex128)
        corr = np.zeros(nr, dtype=np.complex128)
        cond = np.zeros(nr, dtype=np.float64)
        info = np.zeros(nr, dtype=np.int32)
        opt = (lambda arr: arr.ctypes.data) if ndir > 0 else (lambda arr: None)
        _check(self.lib.emme_root_sensitivities_sets(self.h, nr, st.ctypes.data, w.ctypes.data, v.ctypes.data, ndir,
                                                     opt(sp), opt(sm), opt(d), int(max_items), opt(dwdp),
                                                     denom.ctypes.data, corr.ctypes.data, cond.ctypes.data,
                                                     info.ctypes.data))
        return dwdp, denom, corr, cond, info

    def null_vectors(self, M=None, nbatch=None, device_ptr: int | None = None):
        """nullSpace (include/solver.h:58-112) on the device, batched: right singular vector of the smallest
        singular value of every matrix.  M = None: the matrices M(omega_final) of the last solve_roots call;
        device_ptr: the matrices in device memory, M = (nbatch, n).
        Returns (vectors [nbatch, n], info [nbatch])."""
        if device_ptr is not None:
            (nb, n), ptr = M, C.c_void_p(device_ptr)
        elif M is None:
            n, nb, ptr = self.dim, nbatch, None
        else:
            M = _c128(M)
            if M.ndim == 2:
                M = M[None]
            M = np.ascontiguousarray(M)
            nb, n, ptr = M.shape[0], M.shape[1], M.ctypes.data
        v = np.zeros((nb, n), dtype=np.complex128)
        info = np.zeros(nb, dtype=np.int32)
        _check(self.lib.emme_null_vectors_batch(self.h, n, nb, ptr, v.ctypes.data, info.ctypes.data))
        return v, info

    def find_roots_in_contour(self, center, semi_axes, tol=None, step_limit=None, max_roots=64, **contour):
        """Every root inside the ellipse omega(t) = center + a cos t + i b sin t, semi_axes = (a, b) (Beyn's contour
        method + argument-principle count, polished by solve_roots).  contour: points, max_points, probes, rank_tol.
        Returns a dict: roots (sorted by Im descending), iters, info, winding (-1: unresolved), points_used and
        complete (winding >= 0 and as many roots as it counts)."""
        c = contour_default(center=complex(center), semi_axes=tuple(semi_axes), **contour)
        tol = self.params.iteration_precision if tol is None else tol
        step_limit = self.params.iteration_step_limit if step_limit is None else step_limit
        roots = np.zeros(max_roots, dtype=np.complex128)
        iters = np.zeros(max_roots, dtype=np.int32)
        info = np.zeros(max_roots, dtype=np.int32)
        nr, w, pu = C.c_int(0), C.c_int(0), C.c_int(0)
        _check(self.lib.emme_find_roots_in_contour(self.h, C.byref(c), tol, step_limit, max_roots, roots.ctypes.data,
                                                   iters.ctypes.data, info.ctypes.data, C.byref(nr), C.byref(w),
                                                   C.byref(pu)))
        k = min(nr.value, max_roots)
        return {"roots": roots[:k].copy(), "iters": iters[:k].copy(), "info": info[:k].copy(), "n_roots": nr.value,
                "winding": w.value, "points_used": pu.value, "complete": w.value >= 0 and nr.value == w.value}

    def contour_moments(self, M, z, w, L, V=None, device_ptr: int | None = None, v_device_ptr: int | None = None):
        """X_j = M_j^-1 V, A0 = sum w_j X_j, A1 = sum w_j z_j X_j on the device.  M: [nq, n, n] (or device_ptr with
        M = (nq, n)), z, w: nq complex, V: n x L or None (internal probes; v_device_ptr: V in device memory).
        Returns (A0, A1, logdet, info) with logdet[j] = log|det M_j| + i arg det M_j."""
        if device_ptr is None:
            M = np.ascontiguousarray(_c128(M))
            nq, n = M.shape[0], M.shape[1]
            ptr = M.ctypes.data
        else:
            nq, n = M
            ptr = C.c_void_p(device_ptr)
        z = _c128(np.atleast_1d(z))
        w = _c128(np.atleast_1d(w))
        if z.shape[0] != nq or w.shape[0] != nq:
            raise ValueError("z and w need one entry per matrix")
        Vp = None if v_device_ptr is None else C.c_void_p(v_device_ptr)
        if V is not None and v_device_ptr is None:
            V = np.ascontiguousarray(_c128(V))
            if V.shape != (n, L):
                raise ValueError("V must be n x L")
            Vp = V.ctypes.data
        A0 = np.zeros((n, L), dtype=np.complex128)
        A1 = np.zeros((n, L), dtype=np.complex128)
        ld = np.zeros(nq, dtype=np.complex128)
        info = np.zeros(nq, dtype=np.int32)
        _check(self.lib.emme_contour_moments_batch(self.h, n, nq, ptr, z.ctypes.data, w.ctypes.data, L, Vp,
                                                   A0.ctypes.data, A1.ctypes.data, ld.ctypes.data, info.ctypes.data))
        return A0, A1, ld, info

    def contour_moments_groups(self, M, group, ngroups, z, w, L, V=None, device_ptr: int | None = None,
                               v_device_ptr: int | None = None):
        """contour_moments with the matrices dealt into ngroups groups (group[j] in [0, ngroups), any order): returns
        (A0, A1, logdet, info) with A0, A1 of shape [ngroups, n, L], group g summed over its matrices in ascending j
        (info != 0 left out, an empty group zero).  device_ptr / v_device_ptr as in contour_moments."""
        if device_ptr is None:
            M = np.ascontiguousarray(_c128(M))
            nq, n = M.shape[0], M.shape[1]
            ptr = M.ctypes.data
        else:
            nq, n = M
            ptr = C.c_void_p(device_ptr)
        g = np.ascontiguousarray(np.atleast_1d(group), dtype=np.int32)
        z = _c128(np.atleast_1d(z))
        w = _c128(np.atleast_1d(w))
        if g.shape[0] != nq or z.shape[0] != nq or w.shape[0] != nq:
            raise ValueError("group, z and w need one entry per matrix")
        Vp = None if v_device_ptr is None else C.c_void_p(v_device_ptr)
        if V is not None and v_device_ptr is None:
            V = np.ascontiguousarray(_c128(V))
            if V.shape != (n, L):
                raise ValueError("V must be n x L")
            Vp = V.ctypes.data
        A0 = np.zeros((max(ngroups, 0), n, L), dtype=np.complex128)
        A1 = np.zeros((max(ngroups, 0), n, L), dtype=np.complex128)
        ld = np.zeros(nq, dtype=np.complex128)
        info = np.zeros(nq, dtype=np.int32)
        _check(self.lib.emme_contour_moments_groups(self.h, n, nq, ptr, g.ctypes.data, ngroups, z.ctypes.data,
                                                    w.ctypes.data, L, Vp, A0.ctypes.data, A1.ctypes.data, ld.ctypes.data,
                                                    info.ctypes.data))
        return A0, A1, ld, info

    def find_roots_in_contours_sets(self, set, centers, semi_axes, exact=False, tol=None, step_limit=None, max_roots=64,
                                    contours=None):
        """find_roots_in_contour for many (parameter set, contour) items in one lock-step call: item k searches the
        ellipse centers[k], semi_axes[k] = (a, b) on the bound set set[k]; contours: per-item keyword dicts (points,
        max_points, probes, rank_tol) or None.  exact: polish by the Newton search on the exact derivative.  Returns a
        list of dicts shaped like find_roots_in_contour's, plus status (0, or the error that took the item out)."""
        st = np.ascontiguousarray(np.atleast_1d(set), dtype=np.int32)
        n = st.shape[0]
        centers = np.atleast_1d(centers)
        semi_axes = np.asarray(semi_axes, dtype=np.float64).reshape(-1, 2)
        contours = [{}] * n if contours is None else list(contours)
        if len(centers) != n or len(semi_axes) != n or len(contours) != n:
            raise ValueError("centers, semi_axes and contours need one entry per item")
        cts = (Contour * max(n, 1))(*[contour_default(center=complex(centers[k]), semi_axes=tuple(semi_axes[k]),
                                                      **(contours[k] or {})) for k in range(n)])
        tol = self.params.iteration_precision if tol is None else tol
        step_limit = self.params.iteration_step_limit if step_limit is None else step_limit
        roots = np.zeros((max(n, 1), max_roots), dtype=np.complex128)
        iters = np.zeros((max(n, 1), max_roots), dtype=np.int32)
        info = np.zeros((max(n, 1), max_roots), dtype=np.int32)
        nr, w, pu, status = (np.zeros(max(n, 1), dtype=np.int32) for _ in range(4))
        _check(self.lib.emme_find_roots_in_contours_sets(self.h, n, st.ctypes.data, C.cast(cts, C.c_void_p), int(bool(exact)),
                                                         tol, step_limit, max_roots, roots.ctypes.data, iters.ctypes.data,
                                                         info.ctypes.data, nr.ctypes.data, w.ctypes.data, pu.ctypes.data,
                                                         status.ctypes.data))
        out = []
        for k in range(n):
            m = min(int(nr[k]), max_roots)
            out.append({"roots": roots[k, :m].copy(), "iters": iters[k, :m].copy(), "info": info[k, :m].copy(),
                        "n_roots": int(nr[k]), "winding": int(w[k]), "points_used": int(pu[k]),
                        "complete": bool(w[k] >= 0 and nr[k] == w[k]), "status": int(status[k])})
        return out

    # ---- region searches that return eigenpairs ----
    def contour_eigpairs(self, A0, A1, rank_tol=1e-5, max_eigs=64, want_vecs=True):
        """The Beyn step on given moments with its eigenvectors (emme_contour_eigpairs, host only): returns (mu, vecs, k,
        sigma), vecs [min(k, max_eigs), n] with row c = U_k y_c, unit 2-norm (None with want_vecs=False)."""
        A0 = np.ascontiguousarray(_c128(A0))
        A1 = np.ascontiguousarray(_c128(A1))
        n, L = A0.shape
        if A1.shape != (n, L):
            raise ValueError("A0 and A1 must both be n x L")
        mu = np.zeros(max_eigs, dtype=np.complex128)
        vecs = np.zeros((max_eigs, n), dtype=np.complex128) if want_vecs else None
        sigma = np.zeros(L, dtype=np.float64)
        k = C.c_int(0)
        _check(self.lib.emme_contour_eigpairs(n, L, A0.ctypes.data, A1.ctypes.data, rank_tol, max_eigs, mu.ctypes.data,
                                              vecs.ctypes.data if want_vecs else None, C.byref(k), sigma.ctypes.data))
        m = min(k.value, max_eigs)
        return mu[:m].copy(), (vecs[:m].copy() if want_vecs else None), k.value, sigma

    def find_eigenpairs_in_contour(self, center, semi_axes, exact=False, tol=None, step_limit=None, max_roots=64,
                                   **contour):
        """find_roots_in_contour returning every root with its eigenvector (emme_find_eigenpairs_in_contour): the
        candidates carry their Beyn vectors into an eigenpair search -- exact=False: the secant one (plain fills only),
        exact=True: Newton on the exact derivative.  Returns find_roots_in_contour's dict plus vecs [n_roots, dim] (unit
        2-norm) and resid (|M v| / |M|_F per root)."""
        c = contour_default(center=complex(center), semi_axes=tuple(semi_axes), **contour)
        tol = self.params.iteration_precision if tol is None else tol
        step_limit = self.params.iteration_step_limit if step_limit is None else step_limit
        roots = np.zeros(max_roots, dtype=np.complex128)
        vecs = np.zeros((max_roots, self.dim), dtype=np.complex128)
        resid = np.zeros(max_roots, dtype=np.float64)
        iters = np.zeros(max_roots, dtype=np.int32)
        info = np.zeros(max_roots, dtype=np.int32)
        nr, w, pu = C.c_int(0), C.c_int(0), C.c_int(0)
        _check(self.lib.emme_find_eigenpairs_in_contour(self.h, C.byref(c), int(bool(exact)), tol, step_limit, max_roots,
                                                        roots.ctypes.data, vecs.ctypes.data, resid.ctypes.data,
                                                        iters.ctypes.data, info.ctypes.data, C.byref(nr), C.byref(w),
                                                        C.byref(pu)))
        k = min(nr.value, max_roots)
        return {"roots": roots[:k].copy(), "vecs": vecs[:k].copy(), "resid": resid[:k].copy(), "iters": iters[:k].copy(),
                "info": info[:k].copy(), "n_roots": nr.value, "winding": w.value, "points_used": pu.value,
                "complete": w.value >= 0 and nr.value == w.value}

    def find_eigenpairs_in_contours_sets(self, set, centers, semi_axes, exact=False, tol=None, step_limit=None,
                                         max_roots=64, contours=None):
        """find_roots_in_contours_sets returning eigenpairs (emme_find_eigenpairs_in_contours_sets): arguments as there,
        polish as find_eigenpairs_in_contour.  Returns a list of dicts shaped like that call's, plus status."""
        st = np.ascontiguousarray(np.atleast_1d(set), dtype=np.int32)
        n = st.shape[0]
        centers = np.atleast_1d(centers)
        semi_axes = np.asarray(semi_axes, dtype=np.float64).reshape(-1, 2)
        contours = [{}] * n if contours is None else list(contours)
        if len(centers) != n or len(semi_axes) != n or len(contours) != n:
            raise ValueError("centers, semi_axes and contours need one entry per item")
        cts = (Contour * max(n, 1))(*[contour_default(center=complex(centers[k]), semi_axes=tuple(semi_axes[k]),
                                                      **(contours[k] or {})) for k in range(n)])
        tol = self.params.iteration_precision if tol is None else tol
        step_limit = self.params.iteration_step_limit if step_limit is None else step_limit
        m1 = max(n, 1)
        roots = np.zeros((m1, max_roots), dtype=np.complex128)
        vecs = np.zeros((m1, max_roots, self.dim), dtype=np.complex128)
        resid = np.zeros((m1, max_roots), dtype=np.float64)
        iters = np.zeros((m1, max_roots), dtype=np.int32)
        info = np.zeros((m1, max_roots), dtype=np.int32)
        nr, w, pu, status = (np.zeros(m1, dtype=np.int32) for _ in range(4))
        _check(self.lib.emme_find_eigenpairs_in_contours_sets(self.h, n, st.ctypes.data, C.cast(cts, C.c_void_p),
                                                              int(bool(exact)), tol, step_limit, max_roots, roots.ctypes.data,
                                                              vecs.ctypes.data, resid.ctypes.data, iters.ctypes.data,
                                                              info.ctypes.data, nr.ctypes.data, w.ctypes.data,
                                                              pu.ctypes.data, status.ctypes.data))
        out = []
        for k in range(n):
            m = min(int(nr[k]), max_roots)
            out.append({"roots": roots[k, :m].copy(), "vecs": vecs[k, :m].copy(), "resid": resid[k, :m].copy(),
                        "iters": iters[k, :m].copy(), "info": info[k, :m].copy(), "n_roots": int(nr[k]),
                        "winding": int(w[k]), "points_used": int(pu[k]),
                        "complete": bool(w[k] >= 0 and nr[k] == w[k]), "status": int(status[k])})
        return out

    def final_matrix(self, b=0):
        M = np.zeros((self.dim, self.dim), dtype=np.complex128)
        _check(self.lib.emme_ctx_get_matrix(self.h, b, M.ctypes.data))
        return M
