"""ctypes binding of libflashsdf.so (include/flashsdf.h).

This is the product path: every skin / cost evaluation goes through these
entry points into the gfx950 kernels. There is no CPU fallback — if the shared
library is missing or no HIP device is visible, calls raise `FlashNativeError`.
"""
from __future__ import annotations

import ctypes
import os
from ctypes import POINTER, c_char_p, c_double, c_int32, c_int64, c_void_p

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
# FLASHSDF_LIB overrides the library path (A/B builds of the same ABI)
LIB_PATH = os.environ.get("FLASHSDF_LIB") or os.path.join(_HERE, "libflashsdf.so")

FSDF_OK = 0
STATUS_NAMES = {1: "FSDF_ERR_ARG", 2: "FSDF_ERR_HIP", 3: "FSDF_ERR_STATE", 4: "FSDF_ERR_NOMEM",
                5: "FSDF_ERR_DEGENERATE"}


HIP_NULL_STREAM = ctypes.c_void_p(-1).value  # FSDF_HIP_NULL_STREAM ((void*)(intptr_t)-1)


class FlashNativeError(RuntimeError):
    """Raised when the native library fails (or is absent)."""

    def __init__(self, status: int, message: str):
        super().__init__(f"{STATUS_NAMES.get(status, status)}: {message}")
        self.status = status


class FsdfOpts(ctypes.Structure):
    _fields_ = [("device", c_int32), ("precision", c_int32), ("sort_points", c_int32), ("cull", c_int32)]


class FsdfHull(ctypes.Structure):
    _fields_ = [("n_vertices", c_int32), ("n_faces", c_int32), ("vertices", c_void_p), ("faces", c_void_p),
                ("planes", c_void_p)]


SURFACE_HULL, SURFACE_RBF = 0, 1


class FsdfSurface(ctypes.Structure):
    _fields_ = [("kind", c_int32), ("n_centers", c_int32), ("hull", FsdfHull)]


# name -> (restype, argtypes); exactly the functions declared in include/flashsdf.h
_PROTOS = {
    "fsdf_convex_hull": (c_int32, [c_void_p, c_int32, POINTER(c_int32), c_void_p, POINTER(c_int32), c_void_p,
                                   c_void_p]),
    "fsdf_create": (c_int32, [POINTER(c_void_p), POINTER(FsdfOpts)]),
    "fsdf_destroy": (c_int32, [c_void_p]),
    "fsdf_last_error": (c_char_p, [c_void_p]),
    "fsdf_set_stream": (c_int32, [c_void_p, c_void_p]),
    "fsdf_num_hulls": (c_int32, [c_void_p, POINTER(c_int32)]),
    "fsdf_accum_len": (c_int32, [c_void_p, POINTER(c_int32)]),
    "fsdf_set_model": (c_int32, [c_void_p, POINTER(FsdfHull), c_int32]),
    "fsdf_set_surfaces": (c_int32, [c_void_p, POINTER(FsdfSurface), c_int32]),
    "fsdf_set_rbf_params": (c_int32, [c_void_p, c_void_p, c_int64]),
    "fsdf_set_points": (c_int32, [c_void_p, c_void_p, c_int64]),
    "fsdf_set_points_device": (c_int32, [c_void_p, c_void_p, c_int64]),
    "fsdf_prefetch_points": (c_int32, [c_void_p, c_void_p, c_int64]),
    "fsdf_set_points_prefetched": (c_int32, [c_void_p]),
    "fsdf_set_points_range": (c_int32, [c_void_p, c_void_p, c_int64, c_int64, c_int64]),
    "fsdf_set_points_range_device": (c_int32, [c_void_p, c_void_p, c_int64, c_int64, c_int64]),
    "fsdf_regroup_points": (c_int32, [c_void_p]),
    "fsdf_cloud_box_device": (c_int32, [c_void_p, c_void_p, c_int64, c_void_p]),
    "fsdf_curve_keys_device": (c_int32, [c_void_p, c_void_p, c_int64, c_void_p, c_void_p]),
    "fsdf_set_points_keyed_device": (c_int32, [c_void_p, c_void_p, c_void_p, c_void_p, c_int64]),
    "fsdf_regroup_auto": (c_int32, [c_void_p, POINTER(c_int32)]),
    "fsdf_set_regroup": (c_int32, [c_void_p, c_int32]),
    "fsdf_set_solver": (c_int32, [c_void_p, c_int32]),
    "fsdf_num_points": (c_int32, [c_void_p, POINTER(c_int64)]),
    "fsdf_eval": (c_int32, [c_void_p, c_void_p, POINTER(c_double), c_void_p, c_void_p, c_void_p, c_void_p]),
    "fsdf_eval_device": (c_int32, [c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p]),
    "fsdf_skin": (c_int32, [c_void_p, c_void_p, c_void_p, c_int64, c_void_p, c_void_p, c_void_p]),
    "fsdf_set_output_order": (c_int32, [c_void_p, c_int32]),
    "fsdf_get_permutation": (c_int32, [c_void_p, c_void_p]),
    "fsdf_get_permutation_device": (c_int32, [c_void_p, c_void_p]),
    "fsdf_synchronize": (c_int32, [c_void_p]),
    "fsdf_raycast": (c_int32, [c_void_p, c_void_p, c_void_p, c_void_p, c_int64, c_void_p]),
    "fsdf_profile_pass": (c_int32, [c_void_p, c_int32]),
    "fsdf_pass_time": (c_int32, [c_void_p, POINTER(c_double), POINTER(c_int64)]),
    "fsdf_pass_times": (c_int32, [c_void_p, POINTER(c_double), POINTER(c_double), POINTER(c_int64)]),
    "fsdf_kernel_stats": (c_int32, [c_void_p, c_int32, c_void_p]),
    "fsdf_pass_kernel_name": (ctypes.c_char_p, [c_void_p]),
    "fsdf_set_partition": (c_int32, [c_void_p, c_int64, c_int64]),
    "fsdf_set_plan": (c_int32, [c_void_p, c_int32, c_double, c_double, c_int64]),
    "fsdf_chunk_costs": (c_int32, [c_void_p, c_void_p, POINTER(c_int64)]),
    "fsdf_get_partition": (c_int32, [c_void_p, c_int64, POINTER(c_int64), POINTER(c_int64), POINTER(c_int32)]),
    "fsdf_tree_transforms": (c_int32, [c_int32] + [c_void_p] * 13),
    "fsdf_config_gradient": (c_int32, [c_int32] + [c_void_p] * 7 + [c_int32] + [c_void_p] * 5),
    "fsdf_set_mechanism": (c_int32, [c_void_p, c_int32] + [c_void_p] * 8 + [c_int32] + [c_void_p] * 3),
    "fsdf_value_and_gradient": (c_int32, [c_void_p, c_void_p, POINTER(c_double), c_void_p]),
    "fsdf_rbf_solve": (c_int32, [c_int32] + [c_void_p] * 5),
    "fsdf_rbf_adjoint": (c_int32, [c_int32] + [c_void_p] * 7),
    "fsdf_set_rbf_centres": (c_int32, [c_void_p, c_int32, c_int32] + [c_void_p] * 3 + [c_int32] + [c_void_p] * 2),
    "fsdf_set_deformations": (c_int32, [c_void_p, c_int32, c_double]),
    "fsdf_eval_state_device": (c_int32, [c_void_p, c_void_p, c_void_p]),
    "fsdf_state_gradient": (c_int32, [c_void_p] + [c_void_p] * 2 + [POINTER(c_double), c_void_p]),
    "fsdf_descend": (c_int32, [c_void_p, c_void_p, c_int32, c_double, c_double, c_double, c_void_p, c_double,
                               POINTER(c_double), POINTER(c_int32)]),
    "fsdf_gauss_newton_matrix": (c_int32, [c_int32] + [c_void_p] * 7 + [c_int32] + [c_void_p] * 2 + [c_int32] +
                                 [c_void_p] * 2),
    "fsdf_lm_step": (c_int32, [c_int32, c_void_p, c_void_p, c_double, c_double, c_void_p, c_void_p]),
    "fsdf_lm_minimize": (c_int32, [c_void_p, c_void_p, c_int32, c_void_p, c_int32, c_double, c_double, c_double,
                                   c_void_p, POINTER(c_double), POINTER(c_int32), POINTER(c_double)]),
    "fsdf_eval_moments": (c_int32, [c_void_p, c_void_p, POINTER(c_double), c_void_p, c_void_p]),
    "fsdf_value_gradient_hessian": (c_int32, [c_void_p, c_void_p, POINTER(c_double), c_void_p, c_void_p]),
    "fsdf_descend_lm": (c_int32, [c_void_p, c_void_p, c_int32, c_double, c_double, c_double, c_double,
                                  POINTER(c_double), POINTER(c_int32), POINTER(c_double)]),
    "fsdf_set_lm_prior": (c_int32, [c_void_p, c_void_p, c_int32]),
    "fsdf_set_lm_solver": (c_int32, [c_void_p, c_int32]),
    "fsdf_rbf_state_map": (c_int32, [c_int32] + [c_void_p] * 8 + [c_int32, c_int32] + [c_void_p] * 6 + [c_int32] +
                           [c_void_p] * 2),
    "fsdf_gauss_newton_add": (c_int32, [c_int32, c_int32] + [c_void_p] * 4),
    "fsdf_set_lm_skins": (c_int32, [c_void_p, c_int32]),
    "fsdf_skin_moments_time": (c_int32, [c_void_p, POINTER(c_double), POINTER(c_int64)]),
    "fsdf_eval_skin_moments": (c_int32, [c_void_p, c_void_p, POINTER(c_double), c_void_p, c_void_p]),
    "fsdf_set_loss": (c_int32, [c_void_p, c_int32, c_double]),
    "fsdf_set_loss_ref": (c_int32, [c_void_p, c_int32, POINTER(c_double)]),
    "fsdf_get_loss": (c_int32, [c_void_p, POINTER(c_int32), POINTER(c_double)]),
    "fsdf_eval_robust": (c_int32, [c_void_p, c_void_p, POINTER(c_double), c_void_p, c_void_p, c_void_p]),
    "fsdf_set_point_weights": (c_int32, [c_void_p, c_void_p, c_int64]),
    "fsdf_set_point_weights_device": (c_int32, [c_void_p, c_void_p, c_int64]),
    "fsdf_get_point_weights": (c_int32, [c_void_p, c_void_p, POINTER(c_int32)]),
    "fsdf_set_sensor": (c_int32, [c_void_p, c_void_p, c_int32, c_int32, c_int32]),
    "fsdf_get_sensor": (c_int32, [c_void_p, POINTER(c_int32), POINTER(c_int32), POINTER(c_int32)]),
    "fsdf_set_depth_f64": (c_int32, [c_void_p, c_void_p, c_void_p, c_void_p]),
    "fsdf_set_depth_f32": (c_int32, [c_void_p, c_void_p, c_void_p, c_void_p]),
    "fsdf_set_depth_u16": (c_int32, [c_void_p, c_void_p, c_void_p, c_void_p]),
    "fsdf_set_depth_device": (c_int32, [c_void_p, c_void_p, c_int32, c_void_p, c_void_p]),
    "fsdf_get_depth_pixels": (c_int32, [c_void_p, c_void_p, POINTER(c_int64)]),
    "fsdf_set_free_split": (c_int32, [c_void_p, c_int64]),
    "fsdf_get_free_split": (c_int32, [c_void_p, POINTER(c_int64), POINTER(c_int32)]),
    "fsdf_set_free_space": (c_int32, [c_void_p, c_int32, c_int32, c_void_p]),
    "fsdf_get_free_space": (c_int32, [c_void_p, POINTER(c_int32), POINTER(c_int32), c_void_p]),
    "fsdf_set_voxel_grid": (c_int32, [c_void_p, c_double, c_void_p, c_int32]),
    "fsdf_set_voxel_grid_ref": (c_int32, [c_void_p, c_void_p, c_void_p, c_int32]),
    "fsdf_get_voxel_grid": (c_int32, [c_void_p, POINTER(c_double), c_void_p, POINTER(c_int32)]),
    "fsdf_set_points_voxel": (c_int32, [c_void_p, c_void_p, c_int64]),
    "fsdf_set_points_voxel_device": (c_int32, [c_void_p, c_void_p, c_int64]),
    "fsdf_get_voxels": (c_int32, [c_void_p, c_void_p, c_void_p, c_void_p, POINTER(c_int64), POINTER(c_int64),
                                  POINTER(c_int64)]),
    "fsdf_get_voxel_of_point": (c_int32, [c_void_p, c_void_p, POINTER(c_int64)]),
    "fsdf_set_robust_skins": (c_int32, [c_void_p, c_int32]),
    "fsdf_get_robust_skins": (c_int32, [c_void_p, POINTER(c_int32)]),
    "fsdf_eval_robust_skins": (c_int32, [c_void_p, c_void_p, POINTER(c_double), c_void_p, c_void_p, c_void_p,
                                         c_void_p]),
    "fsdf_set_robust_loops": (c_int32, [c_void_p, c_int32]),
    "fsdf_get_robust_loops": (c_int32, [c_void_p, POINTER(c_int32)]),
    "fsdf_eval_robust_device": (c_int32, [c_void_p, c_void_p, c_void_p, c_void_p]),
    "fsdf_score_poses": (c_int32, [c_void_p, c_void_p, c_int32, c_void_p]),
    "fsdf_score_states": (c_int32, [c_void_p, c_void_p, c_int32, c_void_p]),
    "fsdf_score_time": (c_int32, [c_void_p, POINTER(c_double), POINTER(c_int64)]),
    "fsdf_batch_robust_poses": (c_int32, [c_void_p, c_void_p, c_int32, c_void_p, c_void_p, c_void_p]),
    "fsdf_batch_states": (c_int32, [c_void_p, c_void_p, c_int32, c_void_p, c_void_p, c_void_p]),
    "fsdf_descend_lm_batch": (c_int32, [c_void_p, c_void_p, c_int32, c_int32, c_double, c_double, c_double, c_double,
                                        c_void_p, c_void_p, c_void_p]),
    "fsdf_descend_batch": (c_int32, [c_void_p, c_void_p, c_int32, c_int32, c_double, c_double, c_double, c_void_p,
                                     c_double, c_void_p, c_void_p]),
    "fsdf_descend_lm_batch_ref": (c_int32, [c_void_p, c_void_p, c_int32, c_int32, c_void_p, c_void_p, c_void_p,
                                            c_void_p]),
    "fsdf_descend_batch_ref": (c_int32, [c_void_p, c_void_p, c_int32, c_int32, c_void_p, c_void_p, c_void_p,
                                         c_void_p]),
    "fsdf_batch_time": (c_int32, [c_void_p, POINTER(c_double), POINTER(c_int64)]),
}
# fsdf_vgh_fn: int (*)(void* user, const double* x, double* f, double* g, double* H)
VGH_FN = ctypes.CFUNCTYPE(c_int32, c_void_p, POINTER(c_double), POINTER(c_double), POINTER(c_double),
                          POINTER(c_double))
SYMBOLS = tuple(_PROTOS)

_lib = None


def load() -> ctypes.CDLL:
    """Load libflashsdf.so once (raises FlashNativeError if it was never built)."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise FlashNativeError(2, f"{LIB_PATH} not found: build it with `make -C point-cloud-signed-distance_amd/csrc`"
                                  " (or __graft_entry__.build())")
    # ONE HIP runtime per process: PyTorch-ROCm bundles its own libamdhip64
    # (same soname, loaded under another name), and a process that loads ours
    # first ends up with two runtimes, after which torch finds no GPU. With
    # torch imported first, libflashsdf binds to the runtime torch loaded.
    try:
        import torch  # noqa: F401
    except ImportError:
        pass
    lib = ctypes.CDLL(LIB_PATH)
    # an A/B build named by FLASHSDF_LIB may predate an entry point: only the
    # in-tree library must export every one (tests/test_abi.py)
    ab_build = bool(os.environ.get("FLASHSDF_LIB"))
    for name, (res, args) in _PROTOS.items():
        if ab_build and not hasattr(lib, name):
            continue
        fn = getattr(lib, name)
        fn.restype = res
        fn.argtypes = args
    _lib = lib
    return lib


def ptr(a: np.ndarray | None):
    return None if a is None else c_void_p(a.ctypes.data)


def check(status: int, ctx=None, what: str = "") -> None:
    if status != FSDF_OK:
        msg = ""
        if ctx:
            raw = load().fsdf_last_error(ctx)
            msg = raw.decode() if raw else ""
        raise FlashNativeError(status, f"{what}: {msg}" if what else msg)


def convex_hull(points: np.ndarray):
    """conv(points) -> (vertices [m,3], faces [f,3] int32 CCW-outward, planes [f,4])."""
    lib = load()
    pts = np.ascontiguousarray(points, dtype=np.float64).reshape(-1, 3)
    n = pts.shape[0]
    cap_f = max(2 * n - 4, 4)
    verts = np.empty((max(n, 4), 3), np.float64)
    faces = np.empty((cap_f, 3), np.int32)
    planes = np.empty((cap_f, 4), np.float64)
    nv, nf = c_int32(0), c_int32(0)
    st = lib.fsdf_convex_hull(ptr(pts), n, ctypes.byref(nv), ptr(verts), ctypes.byref(nf), ptr(faces), ptr(planes))
    if st != FSDF_OK:
        raise FlashNativeError(st, f"fsdf_convex_hull failed on {n} points")
    return verts[: nv.value].copy(), faces[: nf.value].copy(), planes[: nf.value].copy()


def lm_step(H, g, damping: float, max_step: float):
    """fsdf_lm_step: clamp(−(H + damping·diag(D))⁻¹ g, ±max_step) with D_ii =
    max(H_ii, 1e-12 max_j H_jj), by Cholesky (host only). Returns (status, dx):
    status 5 (FSDF_ERR_DEGENERATE, dx None) for a non-positive or non-finite
    pivot; other failures raise."""
    g = np.ascontiguousarray(g, np.float64).reshape(-1)
    n = g.size
    H = np.ascontiguousarray(H, np.float64).reshape(n, n)
    work = np.empty(n * n + n)
    dx = np.empty(n)
    st = load().fsdf_lm_step(n, ptr(H), ptr(g), float(damping), float(max_step), ptr(work), ptr(dx))
    if st == 5:
        return st, None
    if st != FSDF_OK:
        raise FlashNativeError(st, "fsdf_lm_step: bad arguments")
    return st, dx


def lm_minimize(value_gradient_hessian, x0, iteration_limit: int, damping: float, max_step: float,
                tolerance: float):
    """fsdf_lm_minimize: the Levenberg-Marquardt loop of
    flash.tracking.LevenbergMarquardt.optimize natively (host only), over a
    Python objective x -> (f, g, H). The objective may instead return a nonzero
    int: the loop ends and FlashNativeError carries that status; an exception
    it raises ends the loop too and is raised again here. Returns (x, f,
    evaluations, final damping); f is None when iteration_limit is 0."""
    x = np.array(x0, np.float64, copy=True).reshape(-1)
    n = x.size
    raised = []

    def fn(_user, px, pf, pg, pH):
        try:
            out = value_gradient_hessian(np.ctypeslib.as_array(px, (n,)).copy())
            if isinstance(out, (int, np.integer)):
                return int(out)
            f, g, H = out
            pf[0] = float(f)
            np.ctypeslib.as_array(pg, (n,))[:] = np.asarray(g, np.float64).reshape(n)
            np.ctypeslib.as_array(pH, (n, n))[:] = np.asarray(H, np.float64).reshape(n, n)
            return 0
        except BaseException as e:  # (an exception cannot cross the C frames)
            raised.append(e)
            return 1

    work = np.empty(3 * n * n + 5 * n + 1)
    f, its, lam = c_double(0.0), c_int32(0), c_double(0.0)
    cb = VGH_FN(fn)
    st = load().fsdf_lm_minimize(ctypes.cast(cb, c_void_p), None, n, ptr(x), int(iteration_limit), float(damping),
                                 float(max_step), float(tolerance), ptr(work), ctypes.byref(f), ctypes.byref(its),
                                 ctypes.byref(lam))
    if raised:
        raise raised[0]
    if st != FSDF_OK:
        raise FlashNativeError(st, "fsdf_lm_minimize: the objective's status, or bad arguments")
    return x, (f.value if iteration_limit > 0 else None), its.value, lam.value


class Context:
    """One device context (resident model + cloud). Thin RAII over fsdf_ctx."""

    def __init__(self, device: int = 0, precision: int = 64, cull: bool = True, sort_points: bool = False):
        self._lib = load()
        self._ctx = c_void_p()
        opts = FsdfOpts(device, precision, int(sort_points), int(cull))
        st = self._lib.fsdf_create(ctypes.byref(self._ctx), ctypes.byref(opts))
        if st != FSDF_OK:
            raise FlashNativeError(st, f"fsdf_create(device={device}, precision={precision}) failed:"
                                       " no usable HIP device (the product path has no CPU fallback)")
        self.device = device
        self.precision = precision
        self.K = 0
        self.n = 0
        self._keep = None

    def close(self):
        if self._ctx:
            self._lib.fsdf_destroy(self._ctx)
            self._ctx = c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def set_stream(self, stream_handle: int | None):
        """Launch on this hipStream_t handle; None = the context's own stream.
        Handle 0 is HIP's null stream (torch's default stream reports 0): it is
        passed as FSDF_HIP_NULL_STREAM, since NULL selects the own stream."""
        h = None if stream_handle is None else (HIP_NULL_STREAM if stream_handle == 0 else stream_handle)
        check(self._lib.fsdf_set_stream(self._ctx, c_void_p(h)), self._ctx, "set_stream")

    def set_model(self, hulls):
        """hulls: sequence of (vertices [m,3] f64, faces [f,3] i32, planes [f,4] f64 or None)."""
        self.set_surfaces([("hull", h) for h in hulls])

    def set_surfaces(self, surfaces):
        """surfaces: sequence of ("hull", (vertices, faces, planes)) or ("rbf", n_centres),
        in the scene's surface order (k* indexes it)."""
        arr = (FsdfSurface * len(surfaces))()
        keep = []
        n_rbf = []
        for i, (kind, spec) in enumerate(surfaces):
            if kind == "hull":
                v, f, p = spec
                v = np.ascontiguousarray(v, np.float64)
                f = np.ascontiguousarray(f, np.int32)
                p = None if p is None else np.ascontiguousarray(p, np.float64)
                keep += [v, f, p]
                arr[i] = FsdfSurface(SURFACE_HULL, 0, FsdfHull(v.shape[0], f.shape[0], v.ctypes.data, f.ctypes.data,
                                                               None if p is None else p.ctypes.data))
            elif kind == "rbf":
                arr[i] = FsdfSurface(SURFACE_RBF, int(spec), FsdfHull(0, 0, None, None, None))
                n_rbf.append(int(spec))
            else:
                raise ValueError(kind)
        check(self._lib.fsdf_set_surfaces(self._ctx, arr, len(surfaces)), self._ctx, "set_surfaces")
        self._mechanism_of = None  # the library dropped the mechanism: CostFunctor re-registers
        self.K = len(surfaces)
        self.rbf_centres = n_rbf
        self.accum_len = 1 + 6 * self.K + sum(4 * n + 4 for n in n_rbf)

    def set_rbf_params(self, rows: np.ndarray):
        """Per-pass RBF rows [Σ(n+1), 4] (centres + w, then (a, b)) in surface order."""
        r = np.ascontiguousarray(rows, np.float64)
        check(self._lib.fsdf_set_rbf_params(self._ctx, ptr(r), r.size), self._ctx, "set_rbf_params")

    def set_points(self, xyz: np.ndarray):
        pts = np.ascontiguousarray(xyz, np.float64).reshape(-1, 3)
        check(self._lib.fsdf_set_points(self._ctx, ptr(pts), pts.shape[0]), self._ctx, "set_points")
        self.n = pts.shape[0]

    def set_points_device(self, dev_ptr: int, n: int):
        check(self._lib.fsdf_set_points_device(self._ctx, c_void_p(dev_ptr), n), self._ctx, "set_points_device")
        self.n = n

    def prefetch_points(self, xyz: np.ndarray):
        """Queue the next frame's upload (fsdf_prefetch_points: a copy and sort
        on the context's own stream, issued right after the next pass is
        launched, overlapping the current frame's passes when `xyz` is
        page-locked); set_points_prefetched() makes it resident. The array is
        held until then (the copy reads it)."""
        pts = np.ascontiguousarray(xyz, np.float64).reshape(-1, 3)
        check(self._lib.fsdf_prefetch_points(self._ctx, ptr(pts), pts.shape[0]), self._ctx, "prefetch_points")
        self._prefetched = pts

    def set_points_prefetched(self):
        check(self._lib.fsdf_set_points_prefetched(self._ctx), self._ctx, "set_points_prefetched")
        self.n = self._prefetched.shape[0]
        self._prefetched = None

    def set_points_range(self, xyz: np.ndarray, begin: int, end: int):
        """One shard of a cloud split over devices (fsdf_set_points_range):
        positions [begin, end) of the whole cloud's (Hilbert) order stay
        resident; per-point outputs in resident order, permutation() = their
        indices in the whole cloud."""
        pts = np.ascontiguousarray(xyz, np.float64).reshape(-1, 3)
        check(self._lib.fsdf_set_points_range(self._ctx, ptr(pts), pts.shape[0], int(begin), int(end)), self._ctx,
              "set_points_range")
        self.n = int(end) - int(begin)

    def cloud_box_device(self, d_xyz: int, n: int) -> np.ndarray:
        """fsdf_cloud_box_device: (lo xyz, hi xyz) of a device f64 AoS cloud."""
        box = np.empty(6, np.float64)
        check(self._lib.fsdf_cloud_box_device(self._ctx, c_void_p(d_xyz), int(n), ptr(box)), self._ctx,
              "cloud_box_device")
        return box

    def curve_keys_device(self, d_xyz: int, n: int, box, d_keys: int):
        """fsdf_curve_keys_device: 30-bit Hilbert keys (uint32, device) of the
        points in `box` (6 doubles)."""
        b = np.ascontiguousarray(box, np.float64).reshape(6)
        check(self._lib.fsdf_curve_keys_device(self._ctx, c_void_p(d_xyz), int(n), ptr(b), c_void_p(d_keys)),
              self._ctx, "curve_keys_device")

    def set_points_keyed_device(self, d_xyz: int, d_keys: int, d_index: int, n: int):
        """fsdf_set_points_keyed_device: the exchanged shard becomes resident in
        (key, whole-cloud index) order; permutation = the whole-cloud indices."""
        check(self._lib.fsdf_set_points_keyed_device(self._ctx, c_void_p(d_xyz), c_void_p(d_keys), c_void_p(d_index),
                                                     int(n)), self._ctx, "set_points_keyed_device")
        self.n = int(n)

    def regroup_auto(self) -> bool:
        """fsdf_regroup_auto: regroup only where the library's rule says it pays
        (the last pass ran one wave per chunk); True when it regrouped."""
        applied = c_int32(0)
        check(self._lib.fsdf_regroup_auto(self._ctx, ctypes.byref(applied)), self._ctx, "regroup_auto")
        return bool(applied.value)

    REGROUP_OFF, REGROUP_AUTO = 0, 1

    def set_regroup(self, auto: bool):
        """fsdf_set_regroup: the iteration entry points (value_and_gradient,
        eval_state_device, descend) regroup a new cloud after its first pass by
        the auto rule (default), or never on their own."""
        check(self._lib.fsdf_set_regroup(self._ctx, self.REGROUP_AUTO if auto else self.REGROUP_OFF), self._ctx,
              "set_regroup")

    def set_solver(self, device_loop):
        """fsdf_set_solver: descend's iterations on the device where the scene
        allows (True / 1, the default: rigid scenes), required there
        ("require" / 2: FSDF_ERR_STATE otherwise), or the host loop around
        value_and_gradient (False / 0). "all" / 3: as True, and scenes with
        RBF skins or deformations iterate on the device too where their
        skins' systems fit the step (the host loop otherwise);
        "require-all" / 4: as "require" with those scenes admitted."""
        mode = {"require": 2, "all": 3, "require-all": 4}.get(device_loop) if isinstance(device_loop, str) \
            else int(device_loop)
        if mode is None:
            raise ValueError(f"set_solver: unknown mode {device_loop!r}")
        check(self._lib.fsdf_set_solver(self._ctx, mode), self._ctx, "set_solver")

    def regroup_points(self):
        """Regroup the resident cloud by each point's nearest surface in the
        last pass (fsdf_regroup_points): once per frame, after its first pass.
        Per-point results are unchanged; re-read permutation() for
        resident-order outputs."""
        check(self._lib.fsdf_regroup_points(self._ctx), self._ctx, "regroup_points")

    def set_points_range_device(self, dev_ptr: int, n: int, begin: int, end: int):
        check(self._lib.fsdf_set_points_range_device(self._ctx, c_void_p(dev_ptr), n, int(begin), int(end)),
              self._ctx, "set_points_range_device")
        self.n = int(end) - int(begin)

    def _poses(self, poses):
        p = np.ascontiguousarray(poses, np.float64).reshape(-1, 12)
        if p.shape[0] != self.K:
            raise ValueError(f"expected {self.K} poses, got {p.shape[0]}")
        return p

    def eval(self, poses, per_point: bool = False):
        """One residual pass over the resident cloud -> (cost, accum[1+6K], extras)."""
        p = self._poses(poses)
        accum = np.empty(self.accum_len, np.float64)
        cost = c_double(0.0)
        kstar = d = grad = None
        if per_point:
            kstar = np.empty(self.n, np.int32)
            d = np.empty(self.n, np.float64)
            grad = np.empty((self.n, 3), np.float64)
        check(self._lib.fsdf_eval(self._ctx, ptr(p), ctypes.byref(cost), ptr(accum), ptr(kstar), ptr(d), ptr(grad)),
              self._ctx, "eval")
        return cost.value, accum, (kstar, d, grad)

    def eval_moments(self, poses):
        """fsdf_eval_moments: one pass over the resident cloud and the
        per-surface second moments of its residual, reduced on the device ->
        (cost, accum, moments [K, 21]). Rigid scenes."""
        p = self._poses(poses)
        accum = np.empty(self.accum_len, np.float64)
        mom = np.empty((self.K, 21), np.float64)
        cost = c_double(0.0)
        check(self._lib.fsdf_eval_moments(self._ctx, ptr(p), ctypes.byref(cost), ptr(accum), ptr(mom)), self._ctx,
              "eval_moments")
        return cost.value, accum, mom

    def set_loss(self, loss):
        """fsdf_set_loss: the robust point loss of value_and_gradient,
        value_gradient_hessian, descend, descend_lm and eval_robust — a
        flash.robust.Huber / Tukey (anything with .kind and .scale), or None
        for least squares (the default). A context setting: model and cloud
        swaps keep it."""
        kind, scale = (0, 0.0) if loss is None else (int(loss.kind), float(loss.scale))
        check(self._lib.fsdf_set_loss(self._ctx, kind, scale), self._ctx, "set_loss")
        self._loss = loss

    @property
    def loss(self):
        """The loss last given to set_loss (None: least squares); the library's
        own record is (kind, scale) = loss_setting()."""
        return getattr(self, "_loss", None)

    def loss_setting(self):
        """fsdf_get_loss: (kind, scale) as the library holds them."""
        kind, scale = c_int32(0), c_double(0.0)
        check(self._lib.fsdf_get_loss(self._ctx, ctypes.byref(kind), ctypes.byref(scale)), self._ctx, "get_loss")
        return kind.value, scale.value

    def eval_robust(self, poses, moments: bool = True):
        """fsdf_eval_robust: one pass over the resident cloud and the
        per-surface sums of the context's loss, reduced on the device ->
        (cost = Σρ, accum [1 + 6K] with the robust wrenches, moments [K, 21] =
        Σ w v vᵀ or None, weights [K] = Σ w). Hull-only scenes."""
        p = self._poses(poses)
        accum = np.empty(1 + 6 * self.K, np.float64)
        mom = np.empty((self.K, 21), np.float64) if moments else None
        wts = np.empty(self.K, np.float64)
        cost = c_double(0.0)
        check(self._lib.fsdf_eval_robust(self._ctx, ptr(p), ctypes.byref(cost), ptr(accum), ptr(mom), ptr(wts)),
              self._ctx, "eval_robust")
        return cost.value, accum, mom, wts

    def score_poses(self, poses):
        """fsdf_score_poses: poses [B, K, 12] (or [B, K, 3, 4]) -> costs [B],
        the objective eval_robust returns at each (the context's loss, weights
        and split; a sum, no prior, no regulariser), all candidates in one
        batch of launches. Hull-only scenes; read-only on the context."""
        p = np.ascontiguousarray(poses, np.float64)
        if p.size % (12 * max(self.K, 1)) != 0:
            raise ValueError(f"score_poses: expected [B, {self.K}, 12] poses, got shape {p.shape}")
        B = p.size // (12 * max(self.K, 1))
        cost = np.empty(B, np.float64)
        check(self._lib.fsdf_score_poses(self._ctx, ptr(p), B, ptr(cost)), self._ctx, "score_poses")
        return cost

    def score_states(self, X):
        """fsdf_score_states: states [B, nq] -> costs [B] (set_mechanism first;
        host FK per candidate as value_and_gradient's, then score_poses' path)."""
        x = np.ascontiguousarray(X, np.float64)
        nq = getattr(self, "nq", 0)
        nx = nq + 3 * getattr(self, "n_deform", 0)  # (a deformable scene's rows: the library refuses them itself)
        if x.ndim == 1 and nx:
            x = x.reshape(-1, nx)
        if nq and (x.ndim != 2 or x.shape[1] != nx):
            raise ValueError(f"score_states: X must be [B, {nx}], got shape {x.shape}")
        B = x.shape[0] if x.ndim == 2 else 0
        cost = np.empty(B, np.float64)
        check(self._lib.fsdf_score_states(self._ctx, ptr(x), B, ptr(cost)), self._ctx, "score_states")
        return cost

    def _state_rows(self, X, who):
        """X as contiguous f64 [B, nq] (a single state is a batch of one)."""
        x = np.ascontiguousarray(X, np.float64)
        nq = getattr(self, "nq", 0)
        if not nq:  # no mechanism: the library reports FSDF_ERR_STATE (a single state is one row)
            return x if x.ndim == 2 else x.reshape(1, -1) if x.size else x.reshape(0, 1)
        if x.ndim == 1:
            x = x.reshape(-1, nq) if x.size % nq == 0 else x
        if x.ndim != 2 or x.shape[1] != nq:
            raise ValueError(f"{who}: X must be [B, {nq}], got shape {x.shape}")
        return x

    def batch_robust_poses(self, poses, moments: bool = True):
        """fsdf_batch_robust_poses: poses [B, K, 12] (or [B, K, 3, 4]) ->
        (accum [B, 1 + 6K], moments [B, K, 21] or None, weights [B, K]): per
        candidate what eval_robust returns at its poses, bit for bit, all
        candidates in one batch of launches. Hull-only scenes; read-only on
        the context."""
        p = np.ascontiguousarray(poses, np.float64)
        if p.size % (12 * max(self.K, 1)) != 0:
            raise ValueError(f"batch_robust_poses: expected [B, {self.K}, 12] poses, got shape {p.shape}")
        B = p.size // (12 * max(self.K, 1))
        accum = np.empty((B, 1 + 6 * self.K), np.float64)
        mom = np.empty((B, self.K, 21), np.float64) if moments else None
        wts = np.empty((B, self.K), np.float64)
        check(self._lib.fsdf_batch_robust_poses(self._ctx, ptr(p), B, ptr(accum), ptr(mom), ptr(wts)), self._ctx,
              "batch_robust_poses")
        return accum, mom, wts

    def batch_states(self, X, hessian: bool = True):
        """fsdf_batch_states: states [B, nq] -> (cost [B], grad [B, nq], hess
        [B, nq, nq] or None): value_gradient_hessian's (c, g, H) under a robust
        objective at every row, one batch of launches and one synchronisation
        (set_mechanism first; rigid hull-only scenes)."""
        x = self._state_rows(X, "batch_states")
        B, nq = x.shape
        cost = np.empty(B, np.float64)
        grad = np.empty((B, nq), np.float64)
        hess = np.empty((B, nq, nq), np.float64) if hessian else None
        check(self._lib.fsdf_batch_states(self._ctx, ptr(x), B, ptr(cost), ptr(grad), ptr(hess)), self._ctx,
              "batch_states")
        return cost, grad, hess

    def descend_lm_batch(self, X, iteration_limit, damping, max_step, tolerance=0.0, n_points=1.0):
        """fsdf_descend_lm_batch: descend_lm's host loop for every row of X in
        lockstep, one batch_states per round. Returns (X, f [B], evaluations
        [B], final dampings [B])."""
        x = np.array(self._state_rows(X, "descend_lm_batch"), copy=True)
        B = x.shape[0]
        f, it, lam = np.empty(B, np.float64), np.empty(B, np.int32), np.empty(B, np.float64)
        check(self._lib.fsdf_descend_lm_batch(self._ctx, ptr(x), B, int(iteration_limit), float(damping),
                                              float(max_step), float(tolerance), float(n_points), ptr(f), ptr(it),
                                              ptr(lam)), self._ctx, "descend_lm_batch")
        return x, f, it, lam

    def descend_batch(self, X, iteration_limit, rate, max_step, tolerance=0.0, divisors=None, n_points=1.0):
        """fsdf_descend_batch: descend's host loop (the NaiveSolver rule) for
        every row of X in lockstep. Returns (X, f [B], evaluations [B])."""
        x = np.array(self._state_rows(X, "descend_batch"), copy=True)
        B = x.shape[0]
        div = None if divisors is None else np.ascontiguousarray(divisors, np.float64).reshape(-1)
        if div is not None and div.size != x.shape[1]:
            raise ValueError("descend_batch: divisors must match a state")
        f, it = np.empty(B, np.float64), np.empty(B, np.int32)
        check(self._lib.fsdf_descend_batch(self._ctx, ptr(x), B, int(iteration_limit), float(rate), float(max_step),
                                           float(tolerance), ptr(div), float(n_points), ptr(f), ptr(it)), self._ctx,
              "descend_batch")
        return x, f, it

    def batch_time(self):
        """(summed milliseconds of the batched calls' launches, the slices
        recorded: one per call unless the byte budget split its batch) since the
        last query (profile_pass on)."""
        ms, n = c_double(0.0), c_int64(0)
        check(self._lib.fsdf_batch_time(self._ctx, ctypes.byref(ms), ctypes.byref(n)), self._ctx, "batch_time")
        return ms.value, n.value

    def set_point_weights(self, weights):
        """fsdf_set_point_weights: one confidence weight a_i >= 0 (finite) per
        resident point, in the order of the array the cloud was set from
        (whatever the sort or a regroup did) — a factor of that point's terms
        in every sum of eval_robust, value_and_gradient,
        value_gradient_hessian, descend and descend_lm (hull-only rigid scenes;
        the robust path, also without a loss). None clears them. They belong
        to the resident cloud: every set_points* clears them."""
        if weights is None:
            check(self._lib.fsdf_set_point_weights(self._ctx, None, 0), self._ctx, "set_point_weights")
            return
        w = np.ascontiguousarray(weights, np.float64)
        if w.ndim != 1:
            raise ValueError(f"set_point_weights: one weight per point, got shape {w.shape}")
        check(self._lib.fsdf_set_point_weights(self._ctx, ptr(w), w.shape[0]), self._ctx, "set_point_weights")

    def set_point_weights_device(self, dev_ptr: int, n: int):
        """fsdf_set_point_weights_device: the same from device memory (caller
        order), stream-ordered and NOT validated."""
        check(self._lib.fsdf_set_point_weights_device(self._ctx, c_void_p(dev_ptr), n), self._ctx,
              "set_point_weights_device")

    def point_weights(self):
        """fsdf_get_point_weights: the weights in RESIDENT order (entry i is the
        caller's weight permutation()[i]), or None when none are set."""
        flag = c_int32(0)
        check(self._lib.fsdf_get_point_weights(self._ctx, None, ctypes.byref(flag)), self._ctx, "get_point_weights")
        if not flag.value:
            return None
        out = np.empty(self.n, np.float64)
        check(self._lib.fsdf_get_point_weights(self._ctx, ptr(out), ctypes.byref(flag)), self._ctx,
              "get_point_weights")
        return out

    DEPTH_KINDS = {"range": 0, "z": 1}
    DEPTH_FORMATS = {np.dtype(np.float64): ("fsdf_set_depth_f64", 0), np.dtype(np.float32): ("fsdf_set_depth_f32", 1),
                     np.dtype(np.uint16): ("fsdf_set_depth_u16", 2)}

    def set_sensor(self, rays, kind: str = "range"):
        """fsdf_set_sensor: the depth sensor's rays [rows, cols, 3] (camera
        frame), kept on the device as one direction per pixel — kind "range":
        the depth is the distance along the ray (the reference's DepthSensor);
        "z": the camera-frame z (u = (x/z, y/z, 1)). A context setting: cloud
        and model swaps keep it. None clears it."""
        self._sensor_of = None  # (whose sensor this is: CostFunctor records it after the call)
        if rays is None:
            check(self._lib.fsdf_set_sensor(self._ctx, None, 0, 0, 0), self._ctx, "set_sensor")
            self.sensor_shape = None
            return
        if kind not in self.DEPTH_KINDS:
            raise ValueError(f"set_sensor: kind must be 'range' or 'z', got {kind!r}")
        r = np.ascontiguousarray(rays, np.float64)
        if r.ndim != 3 or r.shape[2] != 3:
            raise ValueError(f"set_sensor: rays must be [rows, cols, 3], got {r.shape}")
        check(self._lib.fsdf_set_sensor(self._ctx, ptr(r), r.shape[0], r.shape[1], self.DEPTH_KINDS[kind]), self._ctx,
              "set_sensor")
        self.sensor_shape = r.shape[:2]

    def sensor(self):
        """fsdf_get_sensor: (rows, cols, kind) as the library holds them, or None."""
        rows, cols, kind = c_int32(0), c_int32(0), c_int32(0)
        check(self._lib.fsdf_get_sensor(self._ctx, ctypes.byref(rows), ctypes.byref(cols), ctypes.byref(kind)),
              self._ctx, "get_sensor")
        return (rows.value, cols.value, ("range", "z")[kind.value]) if rows.value else None

    @staticmethod
    def _depth_args(pose, near, far, scale):
        if pose is not None:
            pose = pose.as_pose12() if hasattr(pose, "as_pose12") else pose
            pose = np.ascontiguousarray(pose, np.float64).reshape(-1)
            if pose.size != 12:
                raise ValueError(f"set_depth: the pose is 12 doubles (R row-major, then t), got {pose.size}")
        return pose, np.array([near, far, scale], np.float64)

    def _num_points(self) -> int:
        n = c_int64(0)
        check(self._lib.fsdf_num_points(self._ctx, ctypes.byref(n)), self._ctx, "num_points")
        return n.value

    def set_depth(self, depth, pose=None, near: float = 0.0, far: float = float("inf"), scale: float = 1.0):
        """fsdf_set_depth_f64 / _f32 / _u16 by the image's dtype: the depth
        image [rows, cols] of the sensor (set_sensor) becomes the resident cloud
        — the points R (s u) + t of the pixels with s = scale · depth finite,
        > 0 and in [near, far], in row-major pixel order (depth_pixels() names
        them); then as set_points. pose: the sensor in the world (a Transform
        or 12 doubles; None: identity). Returns the number of points."""
        d = np.asarray(depth)
        if d.dtype not in self.DEPTH_FORMATS:
            raise TypeError(f"set_depth: the image is float64, float32 or uint16, got {d.dtype}")
        shape = getattr(self, "sensor_shape", None)
        if shape is not None and d.size != shape[0] * shape[1]:
            raise ValueError(f"set_depth: an image of {d.size} pixels for a sensor of {shape[0]} x {shape[1]}")
        d = np.ascontiguousarray(d)
        p, r = self._depth_args(pose, near, far, scale)
        check(getattr(self._lib, self.DEPTH_FORMATS[d.dtype][0])(self._ctx, ptr(d), ptr(p), ptr(r)), self._ctx,
              "set_depth")
        self.n = self._num_points()
        return self.n

    def set_depth_device(self, dev_ptr: int, fmt, pose=None, near: float = 0.0, far: float = float("inf"),
                         scale: float = 1.0):
        """fsdf_set_depth_device: set_depth from an image in device memory
        (rows·cols elements of fmt: a dtype — float64, float32, uint16 — or the
        library's 0 / 1 / 2); only the upload is skipped."""
        if not isinstance(fmt, (int, np.integer)):
            dt = np.dtype(fmt)
            if dt not in self.DEPTH_FORMATS:
                raise TypeError(f"set_depth_device: the image is float64, float32 or uint16, got {dt}")
            fmt = self.DEPTH_FORMATS[dt][1]
        p, r = self._depth_args(pose, near, far, scale)
        check(self._lib.fsdf_set_depth_device(self._ctx, c_void_p(dev_ptr), int(fmt), ptr(p), ptr(r)), self._ctx,
              "set_depth_device")
        self.n = self._num_points()
        return self.n

    def depth_pixels(self) -> np.ndarray:
        """fsdf_get_depth_pixels: pixel (row·cols + col) of every point of the
        resident depth frame, in caller order — the order per-point outputs and
        set_point_weights use: w_img.ravel()[ctx.depth_pixels()] are per-pixel
        confidences as point weights."""
        n = c_int64(0)
        check(self._lib.fsdf_get_depth_pixels(self._ctx, None, ctypes.byref(n)), self._ctx, "get_depth_pixels")
        out = np.empty(n.value, np.int32)
        if n.value:
            check(self._lib.fsdf_get_depth_pixels(self._ctx, ptr(out), ctypes.byref(n)), self._ctx, "get_depth_pixels")
        return out

    def set_free_space(self, free_space):
        """fsdf_set_free_space: the free-space samples every later set_depth
        sends after its observed points — a depthsensors.FreeSpace (anything
        with .samples, .stride, .gap, .spacing, .miss_range), or None for none.
        A context setting like the sensor: frames keep it."""
        if free_space is None:
            check(self._lib.fsdf_set_free_space(self._ctx, 0, 1, None), self._ctx, "set_free_space")
            return
        f = free_space
        lengths = np.array([f.gap, f.spacing, f.miss_range], np.float64)
        check(self._lib.fsdf_set_free_space(self._ctx, int(f.samples), int(f.stride), ptr(lengths)), self._ctx,
              "set_free_space")

    def get_free_space(self):
        """fsdf_get_free_space: (samples, stride, gap, spacing, miss_range) as
        the library holds them, or None when off."""
        samples, stride, lengths = c_int32(0), c_int32(0), np.zeros(3, np.float64)
        check(self._lib.fsdf_get_free_space(self._ctx, ctypes.byref(samples), ctypes.byref(stride), ptr(lengths)),
              self._ctx, "get_free_space")
        return (samples.value, stride.value, *lengths.tolist()) if samples.value else None

    def set_free_split(self, n_surface):
        """fsdf_set_free_split: points [n_surface, n) of the resident cloud, in
        the order of the array it was set from, are free-space samples — they
        count only where the model covers them (d* < 0) in every sum of
        eval_robust, value_and_gradient, value_gradient_hessian, descend and
        descend_lm (hull-only rigid scenes; the robust path, also without a
        loss). None, n or a negative value clears it. It belongs to the
        resident cloud: every set_points* clears it, a set_depth with free
        space on sets its own."""
        check(self._lib.fsdf_set_free_split(self._ctx, -1 if n_surface is None else int(n_surface)), self._ctx,
              "set_free_split")

    def get_free_split(self):
        """fsdf_get_free_split: n_surface of the resident cloud, or None when
        no split is set."""
        n, flag = c_int64(0), c_int32(0)
        check(self._lib.fsdf_get_free_split(self._ctx, ctypes.byref(n), ctypes.byref(flag)), self._ctx,
              "get_free_split")
        return n.value if flag.value else None

    def set_voxel_grid(self, grid):
        """fsdf_set_voxel_grid: the voxel grid that set_points_voxel and every
        later set_depth downsample through — a depthdata.VoxelGrid (anything
        with .size, .origin, .mode), or None for off. A context setting like
        the sensor: frames and model swaps keep it."""
        if grid is None:
            check(self._lib.fsdf_set_voxel_grid(self._ctx, 0.0, None, 1), self._ctx, "set_voxel_grid")
            return
        origin = np.ascontiguousarray(grid.origin, np.float64).reshape(-1)
        if origin.size != 3:
            raise ValueError(f"set_voxel_grid: the origin is 3 numbers, got {origin.size}")
        check(self._lib.fsdf_set_voxel_grid(self._ctx, float(grid.size), ptr(origin), int(grid.mode)), self._ctx,
              "set_voxel_grid")

    def get_voxel_grid(self):
        """fsdf_get_voxel_grid: (size, origin (3 floats), mode) as the library
        holds them, or None when off."""
        size, origin, mode = c_double(0.0), np.zeros(3, np.float64), c_int32(0)
        check(self._lib.fsdf_get_voxel_grid(self._ctx, ctypes.byref(size), ptr(origin), ctypes.byref(mode)), self._ctx,
              "get_voxel_grid")
        return (size.value, tuple(origin.tolist()), mode.value) if size.value else None

    def set_points_voxel(self, xyz: np.ndarray):
        """fsdf_set_points_voxel: the cloud [n, 3] through the context's voxel
        grid (set_voxel_grid) — its m centroids become the resident cloud, in
        ascending cell-key order, then as set_points; under "count" the cells'
        populations become the point weights. Returns m."""
        pts = np.ascontiguousarray(xyz, np.float64).reshape(-1, 3)
        check(self._lib.fsdf_set_points_voxel(self._ctx, ptr(pts), pts.shape[0]), self._ctx, "set_points_voxel")
        self.n = self._num_points()
        return self.n

    def set_points_voxel_device(self, dev_ptr: int, n: int):
        """fsdf_set_points_voxel_device: the same from device memory."""
        check(self._lib.fsdf_set_points_voxel_device(self._ctx, c_void_p(dev_ptr), n), self._ctx,
              "set_points_voxel_device")
        self.n = self._num_points()
        return self.n

    def voxel_sizes(self):
        """fsdf_get_voxels' counters alone: (m voxels, n_in input points, dropped)."""
        m, n_in, dropped = c_int64(0), c_int64(0), c_int64(0)
        check(self._lib.fsdf_get_voxels(self._ctx, None, None, None, ctypes.byref(m), ctypes.byref(n_in),
                                        ctypes.byref(dropped)), self._ctx, "get_voxels")
        return m.value, n_in.value, dropped.value

    def get_voxels(self):
        """fsdf_get_voxels: of the resident voxel cloud (xyz [m, 3], count [m]
        int32, cell [m, 3] int32, n_in, dropped), the voxels in caller order."""
        m, n_in, dropped = self.voxel_sizes()
        xyz, count, cell = np.empty((m, 3), np.float64), np.empty(m, np.int32), np.empty((m, 3), np.int32)
        if m:
            mm = c_int64(0)
            check(self._lib.fsdf_get_voxels(self._ctx, ptr(xyz), ptr(count), ptr(cell), ctypes.byref(mm), None, None),
                  self._ctx, "get_voxels")
        return xyz, count, cell, n_in, dropped

    def get_voxel_of_point(self) -> np.ndarray:
        """fsdf_get_voxel_of_point: for every input point the caller index of
        its voxel, −1 for a dropped (non-finite) point."""
        n = c_int64(0)
        check(self._lib.fsdf_get_voxel_of_point(self._ctx, None, ctypes.byref(n)), self._ctx, "get_voxel_of_point")
        out = np.empty(n.value, np.int32)
        if n.value:
            check(self._lib.fsdf_get_voxel_of_point(self._ctx, ptr(out), ctypes.byref(n)), self._ctx,
                  "get_voxel_of_point")
        return out

    def eval_skin_moments(self, poses):
        """fsdf_eval_skin_moments: one pass over the resident cloud and the
        second moments of its RBF skins at the current rows (set_rbf_params),
        reduced on the device -> (cost, accum, [M_r [4n+4, 4n+4] per skin, in
        surface order])."""
        p = self._poses(poses)
        accum = np.empty(self.accum_len, np.float64)
        ms = [4 * n + 4 for n in self.rbf_centres]
        flat = np.empty(sum(m * m for m in ms), np.float64)
        cost = c_double(0.0)
        check(self._lib.fsdf_eval_skin_moments(self._ctx, ptr(p), ctypes.byref(cost), ptr(accum), ptr(flat)),
              self._ctx, "eval_skin_moments")
        off = np.concatenate([[0], np.cumsum([m * m for m in ms])]).astype(int)
        return cost.value, accum, [flat[off[i]: off[i + 1]].reshape(m, m) for i, m in enumerate(ms)]

    def set_robust_skins(self, enable: bool):
        """fsdf_set_robust_skins: the robust objective (a loss, point weights,
        a free split) also serves scenes with RBF skins and deformations —
        value_and_gradient and descend's host loop, and with set_lm_skins(True)
        value_gradient_hessian and descend_lm's. Off by default: such scenes
        are then refused as before. A context setting."""
        check(self._lib.fsdf_set_robust_skins(self._ctx, int(bool(enable))), self._ctx, "set_robust_skins")
        self.robust_skins = bool(enable)

    def get_robust_skins(self) -> bool:
        """fsdf_get_robust_skins: the switch as the library holds it."""
        v = c_int32(0)
        check(self._lib.fsdf_get_robust_skins(self._ctx, ctypes.byref(v)), self._ctx, "get_robust_skins")
        return bool(v.value)

    def eval_robust_skins(self, poses, moments: bool = True):
        """fsdf_eval_robust_skins (needs set_robust_skins(True)): one pass over
        the resident cloud at the current rows (set_rbf_params) and the sums of
        the context's robust objective -> (cost = Σρ, accum in eval's full
        layout: a hull's robust wrench, a skin's wrench 0, then the skins'
        blocks Σ 2 (aw d*) j; moments [K, 21] with a skin's row zero, or None;
        [Σ aw j jᵀ [4n+4, 4n+4] per skin, in surface order], or None;
        weights [K] = Σ aw)."""
        p = self._poses(poses)
        accum = np.empty(self.accum_len, np.float64)
        mom = np.empty((self.K, 21), np.float64) if moments else None
        ms = [4 * n + 4 for n in self.rbf_centres]
        flat = np.empty(sum(m * m for m in ms), np.float64) if moments else None
        wts = np.empty(self.K, np.float64)
        cost = c_double(0.0)
        check(self._lib.fsdf_eval_robust_skins(self._ctx, ptr(p), ctypes.byref(cost), ptr(accum), ptr(mom), ptr(flat),
                                               ptr(wts)), self._ctx, "eval_robust_skins")
        skin_mom = None
        if moments:
            off = np.concatenate([[0], np.cumsum([m * m for m in ms])]).astype(int)
            skin_mom = [flat[off[i]: off[i + 1]].reshape(m, m) for i, m in enumerate(ms)]
        return cost.value, accum, mom, skin_mom, wts

    def set_robust_loops(self, enable: bool):
        """fsdf_set_robust_loops: a robust objective (a loss, point weights, a
        free split) may run on the device-resident solver loops — descend under
        set_solver(True / "require") and descend_lm under set_lm_solver(True /
        "require") — on hull-only rigid scenes; bit-identical to the host loop.
        Off by default: such objectives then take the host loop and the required
        modes are refused, as before. Scenes with RBF skins or deformations keep
        the host loop either way. A context setting."""
        check(self._lib.fsdf_set_robust_loops(self._ctx, int(bool(enable))), self._ctx, "set_robust_loops")
        self.robust_loops = bool(enable)

    def get_robust_loops(self) -> bool:
        """fsdf_get_robust_loops: the switch as the library holds it."""
        v = c_int32(0)
        check(self._lib.fsdf_get_robust_loops(self._ctx, ctypes.byref(v)), self._ctx, "get_robust_loops")
        return bool(v.value)

    def eval_robust_device(self, poses, d_accum: int, d_moments: int = 0):
        """fsdf_eval_robust_device: eval_robust without the synchronisation and
        the read-back — the pass, the robust launch and the rows' assembly
        enqueued, writing accum [1 + 6K] and (d_moments nonzero) moments
        [K, 21] into device buffers (raw device pointers, fp64): eval_robust's
        accum and moments bit for bit once the stream reaches them."""
        p = self._poses(poses)
        check(self._lib.fsdf_eval_robust_device(self._ctx, ptr(p), c_void_p(d_accum), c_void_p(d_moments or 0)),
              self._ctx, "eval_robust_device")

    def eval_device(self, poses, d_accum: int, d_kstar: int = 0, d_d: int = 0, d_grad: int = 0):
        """Asynchronous pass writing into device buffers (raw device pointers)."""
        p = self._poses(poses)
        check(self._lib.fsdf_eval_device(self._ctx, ptr(p), c_void_p(d_accum), c_void_p(d_kstar or 0),
                                         c_void_p(d_d or 0), c_void_p(d_grad or 0)), self._ctx, "eval_device")

    def skin(self, poses, xyz: np.ndarray):
        """Scene SDF at arbitrary points -> (d [n], kstar [n], grad [n,3])."""
        p = self._poses(poses)
        q = np.ascontiguousarray(xyz, np.float64).reshape(-1, 3)
        n = q.shape[0]
        d = np.empty(n, np.float64)
        k = np.empty(n, np.int32)
        g = np.empty((n, 3), np.float64)
        check(self._lib.fsdf_skin(self._ctx, ptr(p), ptr(q), n, ptr(d), ptr(k), ptr(g)), self._ctx, "skin")
        return d, k, g

    def raycast(self, poses, origin, rays):
        """Secant raycast of unit world rays [n,3] from origin -> depth [n] (NaN = miss)."""
        p = self._poses(poses)
        o = np.ascontiguousarray(origin, np.float64).reshape(3)
        r = np.ascontiguousarray(rays, np.float64).reshape(-1, 3)
        depth = np.empty(len(r), np.float64)
        check(self._lib.fsdf_raycast(self._ctx, ptr(p), ptr(o), ptr(r), len(r), ptr(depth)), self._ctx, "raycast")
        return depth

    ORDER_CALLER, ORDER_RESIDENT = 0, 1

    def set_output_order(self, resident: bool):
        """Per-point outputs of eval / eval_device in resident (device, Hilbert)
        order — coalesced stores — or in caller order (the default)."""
        check(self._lib.fsdf_set_output_order(self._ctx, int(bool(resident))), self._ctx, "set_output_order")

    def permutation(self) -> np.ndarray:
        """perm[i] = caller index of resident point i."""
        out = np.empty(self.n, np.int64)
        check(self._lib.fsdf_get_permutation(self._ctx, ptr(out)), self._ctx, "get_permutation")
        return out

    def permutation_device(self, d_out: int):
        check(self._lib.fsdf_get_permutation_device(self._ctx, c_void_p(d_out)), self._ctx, "get_permutation_device")

    def synchronize(self):
        check(self._lib.fsdf_synchronize(self._ctx), self._ctx, "synchronize")

    def profile_pass(self, enable: bool = True):
        check(self._lib.fsdf_profile_pass(self._ctx, int(enable)), self._ctx, "profile_pass")

    def pass_time(self):
        """(summed whole-pass milliseconds, launches) since the last query."""
        ms, n = c_double(0.0), c_int64(0)
        check(self._lib.fsdf_pass_time(self._ctx, ctypes.byref(ms), ctypes.byref(n)), self._ctx, "pass_time")
        return ms.value, n.value

    def skin_moments_time(self):
        """(summed milliseconds of the skin-moments launches, their count)
        since the last query (profile_pass on)."""
        ms, n = c_double(0.0), c_int64(0)
        check(self._lib.fsdf_skin_moments_time(self._ctx, ctypes.byref(ms), ctypes.byref(n)), self._ctx,
              "skin_moments_time")
        return ms.value, n.value

    def score_time(self):
        """(summed milliseconds of the scoring calls' launches, the calls
        recorded) since the last query (profile_pass on)."""
        ms, n = c_double(0.0), c_int64(0)
        check(self._lib.fsdf_score_time(self._ctx, ctypes.byref(ms), ctypes.byref(n)), self._ctx, "score_time")
        return ms.value, n.value

    def pass_times(self):
        """(summed pass-kernel ms, summed whole-pass ms,
        launches) since the last query."""
        k, p, n = c_double(0.0), c_double(0.0), c_int64(0)
        check(self._lib.fsdf_pass_times(self._ctx, ctypes.byref(k), ctypes.byref(p), ctypes.byref(n)), self._ctx,
              "pass_times")
        return k.value, p.value, n.value

    def pass_kernel_name(self) -> str:
        """The pass-kernel variant of the last residual pass ('' before any)."""
        return self._lib.fsdf_pass_kernel_name(self._ctx).decode()

    def set_partition(self, four_way_max_points: int = -1, two_way_max_points: int = -1):
        """Hull-partitioned pass tiers for this context: -1 = the model's
        default, 0 = off, else the largest cloud the tier runs."""
        check(self._lib.fsdf_set_partition(self._ctx, int(four_way_max_points), int(two_way_max_points)), self._ctx,
              "set_partition")

    def set_plan(self, enable: bool = True, four_way_share: float = -1.0, two_way_share: float = -1.0,
                 max_points: int = -1):
        """Planned pass of resident clouds (fsdf_set_plan): enable, the shares
        of chunks split over 4 / 2 waves (< 0: the default counts), the
        largest cloud it runs (-1: default)."""
        check(self._lib.fsdf_set_plan(self._ctx, int(enable), float(four_way_share), float(two_way_share),
                                      int(max_points)), self._ctx, "set_plan")

    def chunk_costs(self) -> np.ndarray:
        """Per-chunk serial-equivalent durations (100 MHz ticks) of the last planned pass."""
        cnt = c_int64(0)
        check(self._lib.fsdf_chunk_costs(self._ctx, None, ctypes.byref(cnt)), self._ctx, "chunk_costs")
        out = np.empty(cnt.value, np.uint32)
        if cnt.value:
            check(self._lib.fsdf_chunk_costs(self._ctx, out.ctypes.data, ctypes.byref(cnt)), self._ctx, "chunk_costs")
        return out

    def get_partition(self, n: int = 0):
        """(4-way limit, 2-way limit, waves per chunk a pass over n points runs)."""
        a, b, p = c_int64(0), c_int64(0), c_int32(0)
        check(self._lib.fsdf_get_partition(self._ctx, int(n), ctypes.byref(a), ctypes.byref(b), ctypes.byref(p)),
              self._ctx, "get_partition")
        return a.value, b.value, p.value

    def set_mechanism(self, mechanism, surface_body, frame_R, frame_t):
        """Register the mechanism tree and each surface's body / frame for
        value_and_gradient (hull-only scenes)."""
        P = mechanism._kinematic_plan()
        nb = mechanism.num_bodies
        sb = np.ascontiguousarray(surface_body, np.int32)
        fr = np.ascontiguousarray(frame_R, np.float64).reshape(-1, 9)
        ft = np.ascontiguousarray(frame_t, np.float64).reshape(-1, 3)
        check(self._lib.fsdf_set_mechanism(self._ctx, nb, *P["native_ptrs"][:8], mechanism.num_positions, ptr(sb),
                                           ptr(fr), ptr(ft)), self._ctx, "set_mechanism")
        self.nq = mechanism.num_positions

    def set_rbf_centres(self, surface: int, surface_points, skeleton_points, deform_rows=None):
        """Declare RBF surface `surface`'s centres for value_and_gradient:
        lists of (body, body-frame xyz); deform_rows[j] = the deformation row of
        surface point j (-1: rigid)."""
        nsp, nsk = len(surface_points), len(skeleton_points)
        bsp = np.ascontiguousarray([b for b, _ in surface_points], np.int32)
        lsp = np.ascontiguousarray(np.reshape([p for _, p in surface_points], (nsp, 3)), np.float64)
        dr = None if deform_rows is None else np.ascontiguousarray(deform_rows, np.int32)
        bsk = np.ascontiguousarray([b for b, _ in skeleton_points], np.int32)
        lsk = np.ascontiguousarray(np.reshape([p for _, p in skeleton_points], (nsk, 3)), np.float64)
        check(self._lib.fsdf_set_rbf_centres(self._ctx, int(surface), nsp, ptr(bsp), ptr(lsp), ptr(dr), nsk, ptr(bsk),
                                             ptr(lsk)), self._ctx, "set_rbf_centres")

    def set_deformations(self, n_deform: int, weight: float):
        """x = [q; δ] with 3·n_deform deformation entries, regularizer weight."""
        check(self._lib.fsdf_set_deformations(self._ctx, int(n_deform), float(weight)), self._ctx, "set_deformations")
        self.n_deform = int(n_deform)

    def _state_vector(self, x, who):
        """x as contiguous f64 of exactly nq + 3 n_deform entries (the C side
        reads that many)."""
        x = np.ascontiguousarray(x, np.float64).reshape(-1)
        if not hasattr(self, "nq"):
            return x  # no mechanism: the library reports FSDF_ERR_STATE
        n = self.nq + 3 * getattr(self, "n_deform", 0)
        if x.size != n:
            raise ValueError(f"{who}: x must have nq + 3 n_deform = {n} entries, got {x.size}")
        return x

    def value_and_gradient(self, x):
        """(cost, ∂cost/∂x) in one native call (FK, RBF solve, pass, chain rule,
        regularizer)."""
        x = self._state_vector(x, "value_and_gradient")
        g = np.empty(self.nq + 3 * getattr(self, "n_deform", 0))
        c = c_double(0.0)
        check(self._lib.fsdf_value_and_gradient(self._ctx, ptr(x), ctypes.byref(c), ptr(g)), self._ctx,
              "value_and_gradient")
        return c.value, g

    def value_gradient_hessian(self, x):
        """(cost, ∂cost/∂x, the Gauss-Newton Hessian 2 JᵀJ) in one native call
        (fsdf_value_gradient_hessian; rigid scenes, and with set_lm_skins(True)
        scenes with RBF skins and deformations: x, g and H over nq + 3 n_deform)."""
        x = self._state_vector(x, "value_gradient_hessian")
        g = np.empty(x.size)
        H = np.empty((x.size, x.size))
        c = c_double(0.0)
        check(self._lib.fsdf_value_gradient_hessian(self._ctx, ptr(x), ctypes.byref(c), ptr(g), ptr(H)), self._ctx,
              "value_gradient_hessian")
        return c.value, g, H

    def descend_lm(self, x, iteration_limit, damping, max_step, tolerance=0.0, n_points=1.0):
        """fsdf_descend_lm: the Levenberg-Marquardt loop over
        value_gradient_hessian natively. Returns (x, f at x, evaluations made,
        final damping)."""
        x = np.array(self._state_vector(x, "descend_lm"), copy=True)
        f, it, lam = c_double(0.0), c_int32(0), c_double(0.0)
        check(self._lib.fsdf_descend_lm(self._ctx, ptr(x), int(iteration_limit), float(damping), float(max_step),
                                        float(tolerance), float(n_points), ctypes.byref(f), ctypes.byref(it),
                                        ctypes.byref(lam)), self._ctx, "descend_lm")
        return x, f.value, it.value, lam.value

    def set_lm_prior(self, weight):
        """fsdf_set_lm_prior: descend_lm's objective becomes c/N + Σ weight_i
        (x_i − x̄_i)², x̄ the x handed to that call. weight: one value per
        joint coordinate (a scalar is repeated), each >= 0; None clears it."""
        if weight is None:
            check(self._lib.fsdf_set_lm_prior(self._ctx, None, 0), self._ctx, "set_lm_prior")
            return
        w = np.asarray(weight, np.float64)
        if w.ndim == 0:
            if not hasattr(self, "nq"):
                raise ValueError("set_lm_prior: a scalar weight needs the mechanism's coordinate count "
                                 "(call set_mechanism first)")
            n = self.nq + (3 * getattr(self, "n_deform", 0) if getattr(self, "lm_skins", False) else 0)
            w = np.full(n, float(w))
        w = np.ascontiguousarray(w).reshape(-1)
        check(self._lib.fsdf_set_lm_prior(self._ctx, ptr(w), w.size), self._ctx, "set_lm_prior")

    def set_lm_skins(self, enable: bool):
        """fsdf_set_lm_skins: value_gradient_hessian and descend_lm serve scenes
        with RBF skins and deformations (off by default: they are refused)."""
        check(self._lib.fsdf_set_lm_skins(self._ctx, int(bool(enable))), self._ctx, "set_lm_skins")
        self.lm_skins = bool(enable)

    def set_lm_solver(self, device_loop):
        """fsdf_set_lm_solver: descend_lm's loop on the host (False / 0, the
        default), on the device where the scene fits (True / 1), or required
        there ("require" / 2: FSDF_ERR_STATE otherwise). The same bits."""
        mode = {"require": 2}.get(device_loop) if isinstance(device_loop, str) else int(device_loop)
        if mode is None:
            raise ValueError(f"set_lm_solver: unknown mode {device_loop!r}")
        check(self._lib.fsdf_set_lm_solver(self._ctx, mode), self._ctx, "set_lm_solver")
        self.lm_solver_mode = mode  # (the library keeps no getter: callers that switch for one call restore this)

    def descend(self, x, iteration_limit, rate, max_step, tolerance=0.0, divisors=None, n_points=1.0):
        """fsdf_descend: the NaiveSolver loop over value_and_gradient natively.
        Returns (x, f of the last evaluation, evaluations made)."""
        x = np.array(x, np.float64, copy=True)
        if x.size != self.nq + 3 * getattr(self, "n_deform", 0):
            raise ValueError("descend: x must have nq + 3 n_deform entries")
        div = None if divisors is None else np.ascontiguousarray(divisors, np.float64)
        if div is not None and div.shape != x.shape:
            raise ValueError("descend: divisors must match x")
        f = c_double(0.0)
        it = c_int32(0)
        check(self._lib.fsdf_descend(self._ctx, ptr(x), int(iteration_limit), float(rate), float(max_step),
                                     float(tolerance), ptr(div) if div is not None else None, float(n_points),
                                     ctypes.byref(f), ctypes.byref(it)), self._ctx, "descend")
        return x, f.value, it.value

    def eval_state_device(self, x, d_accum: int):
        """FK, RBF solve, poses and the pass at x into the device accumulator
        (asynchronous; value_and_gradient's first half)."""
        x = self._state_vector(x, "eval_state_device")
        check(self._lib.fsdf_eval_state_device(self._ctx, ptr(x), c_void_p(d_accum)), self._ctx, "eval_state_device")

    def state_gradient(self, x, accum):
        """(cost, ∂cost/∂x) from an (all-reduced) host accumulator of the pass at x."""
        x = self._state_vector(x, "state_gradient")
        a = np.ascontiguousarray(accum, np.float64)
        g = np.empty(self.nq + 3 * getattr(self, "n_deform", 0))
        c = c_double(0.0)
        check(self._lib.fsdf_state_gradient(self._ctx, ptr(x), ptr(a), ctypes.byref(c), ptr(g)), self._ctx,
              "state_gradient")
        return c.value, g

    STAT_NAMES = ("wave_iters", "hull_evals", "slow_waves", "lane_needs", "slow_lanes", "seed_evals",
                  "scan_waves", "full_scan_lanes", "wave_candidates", "faces_evaluated", "cyc_cull", "cyc_stage",
                  "cyc_plane", "cyc_fast", "cyc_slow", "cyc_iter", "cyc_reduce", "cyc_store", "cyc_scene",
                  "screen_fallbacks", "screen_rejects", "walk_steps", "seed_first_waves", "reserved_23")

    def kernel_stats(self, enable: bool):
        """enable=True: start counting; enable=False: stop, return the counters."""
        out = np.zeros(len(self.STAT_NAMES), np.uint64)
        check(self._lib.fsdf_kernel_stats(self._ctx, int(enable), ptr(out)), self._ctx, "kernel_stats")
        return None if enable else dict(zip(self.STAT_NAMES, (int(v) for v in out)))
