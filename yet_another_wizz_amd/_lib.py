"""ctypes binding of ``libyawhip.so`` (C ABI: ``include/yawhip.h``).

There is deliberately no CPU fallback: if the shared object is missing or no MI355X is visible the
calls raise ``YawhipError`` -- a measurement must never silently run somewhere else.
"""
from __future__ import annotations

import ctypes
import os
import weakref
from dataclasses import dataclass

import numpy as np

_PKG_DIR = os.path.dirname(os.path.abspath(__file__))
# YAW_AMD_LIB points experiments at a variant build (tools/build_variant.py); the product loads the in-tree library
LIB_PATH = os.environ.get("YAW_AMD_LIB") or os.path.join(_PKG_DIR, "libyawhip.so")

DEFAULT_STRIP_MICRO = 5000  # the library's default strip grid spacing, in 1e-6 rad of latitude (strip_grid = 1)
KERNEL_AUTO, KERNEL_EXACT, KERNEL_FILTER, KERNEL_SWEEP, KERNEL_BAND = 0, 1, 2, 3, 4
KERNEL_IDS = {"auto": KERNEL_AUTO, "exact": KERNEL_EXACT, "filter": KERNEL_FILTER, "sweep": KERNEL_SWEEP,
              "band": KERNEL_BAND}

# every symbol include/yawhip.h declares (tests check the export list against this)
ABI_SYMBOLS = (
    "yawhip_last_error",
    "yawhip_abi_version",
    "yawhip_device_count",
    "yawhip_ctx_create",
    "yawhip_ctx_create_multi",
    "yawhip_ctx_device_count",
    "yawhip_ctx_destroy",
    "yawhip_ctx_set_option",
    "yawhip_catalog_upload",
    "yawhip_catalog_upload_axis",
    "yawhip_catalog_upload_scalar",
    "yawhip_catalog_segment_sums",
    "yawhip_catalog_sort_axis",
    "yawhip_catalog_free",
    "yawhip_catalog_device_bytes",
    "yawhip_count_pairs",
    "yawhip_count_pairs_dense",
    "yawhip_count_pairs_dense_batch",
    "yawhip_count_pairs_rows_device",
    "yawhip_job_work",
    "yawhip_assign_patches",
    "yawhip_random_box",
    "yawhip_random_healpix",
    "yawhip_healpix_map",
    "yawhip_healpix_pixels",
    "yawhip_redshift_histogram",
    "yawhip_host_group_columns",
    "yawhip_host_scatter_rows",
    "yawhip_kmeans_open",
    "yawhip_kmeans_seed",
    "yawhip_kmeans_pick",
    "yawhip_kmeans_step",
    "yawhip_kmeans_query",
    "yawhip_kmeans_close",
    "yawhip_shear_upload",
    "yawhip_shear_free",
    "yawhip_shear_count",
    "yawhip_shear_upload_binned",
    "yawhip_shear_auto_count",
    "yawhip_shear_pair_count",
    "yawhip_dsigma_upload_lenses",
    "yawhip_dsigma_upload_sources",
    "yawhip_dsigma_count",
    "yawhip_dsigma_upload_lenses_radial",
    "yawhip_dsigma_count_radial",
    "yawhip_proj_upload",
    "yawhip_proj_count",
    "yawhip_proj_count_pi",
    "yawhip_proj_count_smu",
    "yawhip_proj_upload_shapes",
    "yawhip_proj_count_shear",
    "yawhip_proj_count_shapes",
    "yawhip_proj_count_pi_signed",
    "yawhip_proj_count_smu_signed",
)


class YawhipError(RuntimeError):
    """Raised when libyawhip.so is unavailable or a call into it fails."""


class _Stats(ctypes.Structure):
    _fields_ = [
        ("candidate_pairs", ctypes.c_int64),
        ("evaluated_pairs", ctypes.c_int64),
        ("algorithmic_bytes", ctypes.c_int64),
        ("n_workgroups", ctypes.c_int64),
        ("n_launches", ctypes.c_int32),
        ("kernel_used", ctypes.c_int32),
        ("kernel_ms", ctypes.c_double),
        ("total_ms", ctypes.c_double),
        ("count_ms", ctypes.c_double),
        ("layout_mode", ctypes.c_int32),
        ("n_orientations", ctypes.c_int32),
        ("exact_reevaluations", ctypes.c_int64),
        ("band_variant", ctypes.c_int32),
        ("merged_triples", ctypes.c_int32),
        ("count_variant", ctypes.c_int32),
        ("count_variant_weighted", ctypes.c_int32),
    ]


class _DenseRequest(ctypes.Structure):
    """``yawhip_dense_request`` of include/yawhip.h (pointers as plain addresses)."""
    _fields_ = [
        ("c1", ctypes.c_void_p),
        ("c2", ctypes.c_void_p),
        ("n_jobs", ctypes.c_int32),
        ("halve_diagonal", ctypes.c_int32),
        ("jobs", ctypes.c_void_p),
        ("dense", ctypes.c_void_p),
        ("stats", ctypes.c_void_p),
    ]


@dataclass
class CountStats:
    candidate_pairs: int = 0
    evaluated_pairs: int = 0
    algorithmic_bytes: int = 0
    n_workgroups: int = 0
    n_launches: int = 0
    kernel_used: int = 0
    kernel_ms: float = 0.0
    total_ms: float = 0.0
    count_ms: float = 0.0
    layout_mode: int = 0
    n_orientations: int = 0
    exact_reevaluations: int = 0
    band_variant: int = 0
    merged_triples: int = 0
    count_variant: int = 0           # variant code of the unweighted count launch (variant_name), 0 none, VARIANT_MIXED
    count_variant_weighted: int = 0  # ... of the weighted one

    @property
    def variants(self) -> set:
        """Names of the count kernels the call launched (``variant_name`` of both codes; none: empty)."""
        return {variant_name(c) for c in (self.count_variant, self.count_variant_weighted) if c != 0}


def _count_stats(st: _Stats) -> CountStats:
    return CountStats(**{f: getattr(st, f) for f, _ in _Stats._fields_})


# yawhip_stats.count_variant* (include/yawhip.h): family in bits 0-3, then the template arguments
VARIANT_MIXED = -1
VARIANT_FAMILIES = {1: "k_count", 2: "k_count_merged", 3: "k_count_merged_occ8", 4: "k_count_band", 5: "k_count_band32",
                    6: "k_count_band32_one", 7: "k_count_band32_fine"}
# template parameters of each family, in order
VARIANT_PARAMS = {"k_count": ("R", "WEIGHTED", "PRIV", "FILTER"), "k_count_merged": ("R", "WEIGHTED", "NF1", "MERGED"),
                  "k_count_merged_occ8": ("R", "WEIGHTED", "NF1", "MERGED"),
                  "k_count_band": ("R", "CAP", "WEIGHTED", "NE", "MERGED", "UNI"),
                  "k_count_band32": ("R", "CAP", "WEIGHTED", "NE", "MERGED", "UNI"),
                  "k_count_band32_one": ("R", "CAP", "WEIGHTED", "NE", "MERGED", "UNI"),
                  "k_count_band32_fine": ("R", "CAP", "WEIGHTED", "MERGED", "UNI")}
_VARIANT_FIELDS = {"R": (4, 3), "CAP": (8, 10), "WEIGHTED": (18, 1), "NE": (19, 3), "MERGED": (22, 1), "UNI": (23, 1),
                   "PRIV": (24, 1), "FILTER": (25, 1), "NF1": (26, 1)}  # (first bit, bits)


def variant_name(code: int) -> str:
    """A count-kernel variant code rendered as ``nm -C`` prints the kernel, e.g. ``k_count_band32_one<2, 512, false, 2, true,
    true>``; ``"mixed"`` for VARIANT_MIXED. Raises ValueError for 0 or a code that names no family."""
    if code == VARIANT_MIXED:
        return "mixed"
    family = VARIANT_FAMILIES.get(code & 0xF)
    if family is None:
        raise ValueError(f"not a count-kernel variant code: {code}")
    args = []
    for p in VARIANT_PARAMS[family]:
        lo, bits = _VARIANT_FIELDS[p]
        v = (code >> lo) & ((1 << bits) - 1)
        args.append(str(v) if bits > 1 else ("true" if v else "false"))
    return f"{family}<{', '.join(args)}>"


def variant_code(name: str) -> int:
    """Inverse of ``variant_name``: the code of a kernel named as ``nm -C`` prints it."""
    family, args = name.rstrip(">").split("<")
    code = {v: k for k, v in VARIANT_FAMILIES.items()}[family]
    for p, a in zip(VARIANT_PARAMS[family], (a.strip() for a in args.split(",")), strict=True):
        lo, bits = _VARIANT_FIELDS[p]
        v = {"true": 1, "false": 0}[a] if bits == 1 else int(a)
        if not 0 <= v < (1 << bits):
            raise ValueError(f"{p} = {a} does not fit the code")
        code |= v << lo
    return code


_dp = ctypes.POINTER(ctypes.c_double)
_i64p = ctypes.POINTER(ctypes.c_int64)
_i32p = ctypes.POINTER(ctypes.c_int32)
_vp = ctypes.c_void_p
_lib = None


def load_library() -> ctypes.CDLL:
    """Load libyawhip.so and declare its prototypes. Does not touch the GPU."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise YawhipError(
            f"{LIB_PATH} not found: build it with `python -m yet_another_wizz_amd.build` "
            "(hipcc, gfx950). There is no CPU fallback for the pair-count path."
        )
    try:
        lib = ctypes.CDLL(LIB_PATH)
    except OSError as err:  # e.g. libamdhip64 missing
        raise YawhipError(f"cannot load {LIB_PATH}: {err}") from err
    lib.yawhip_last_error.restype = ctypes.c_char_p
    lib.yawhip_last_error.argtypes = []
    lib.yawhip_abi_version.restype = ctypes.c_int
    lib.yawhip_abi_version.argtypes = []
    lib.yawhip_device_count.argtypes = [ctypes.POINTER(ctypes.c_int)]
    lib.yawhip_ctx_create.argtypes = [ctypes.c_int, ctypes.POINTER(_vp)]
    lib.yawhip_ctx_create_multi.argtypes = [ctypes.POINTER(ctypes.c_int), ctypes.c_int, ctypes.POINTER(_vp)]
    lib.yawhip_ctx_device_count.argtypes = [_vp, ctypes.POINTER(ctypes.c_int)]
    lib.yawhip_ctx_destroy.argtypes = [_vp]
    lib.yawhip_ctx_set_option.argtypes = [_vp, ctypes.c_char_p, ctypes.c_int64]
    lib.yawhip_catalog_upload.argtypes = [
        _vp, ctypes.c_int64, _dp, _dp, _dp, _dp, ctypes.c_int32, ctypes.c_int32, _i64p, ctypes.POINTER(_vp),
    ]
    lib.yawhip_catalog_upload_axis.argtypes = [
        _vp, ctypes.c_int64, _dp, _dp, _dp, _dp, ctypes.c_int32, ctypes.c_int32, _i64p, ctypes.c_int32, ctypes.POINTER(_vp),
    ]
    lib.yawhip_catalog_upload_scalar.argtypes = [
        _vp, ctypes.c_int64, _dp, _dp, _dp, _dp, _dp, ctypes.c_int32, ctypes.c_int32, _i64p, ctypes.c_int32, ctypes.POINTER(_vp),
        ctypes.POINTER(_vp),
    ]
    lib.yawhip_catalog_segment_sums.argtypes = [_vp, _dp]
    lib.yawhip_catalog_sort_axis.argtypes = [_vp, ctypes.POINTER(ctypes.c_int32)]
    lib.yawhip_catalog_free.argtypes = [_vp]
    lib.yawhip_catalog_device_bytes.argtypes = [_vp, _i64p]
    lib.yawhip_count_pairs.argtypes = [
        _vp, _vp, _vp, ctypes.c_int32, _i32p, ctypes.c_int32, ctypes.c_int32, _dp, ctypes.c_int32,
        _i64p, _dp, ctypes.POINTER(_Stats),
    ]
    lib.yawhip_count_pairs_dense.argtypes = [  # array arguments as plain addresses (_addr): this is the per-call hot path
        _vp, _vp, _vp, ctypes.c_int32, _vp, ctypes.c_int32, ctypes.c_int32, _vp, ctypes.c_int32,
        ctypes.c_int32, _vp, _vp, ctypes.c_int32, _vp, ctypes.POINTER(_Stats),
    ]
    lib.yawhip_count_pairs_dense_batch.argtypes = [
        _vp, ctypes.c_int32, ctypes.POINTER(_DenseRequest), ctypes.c_int32, ctypes.c_int32, _vp, ctypes.c_int32, ctypes.c_int32,
        _vp, _vp,
    ]
    lib.yawhip_count_pairs_rows_device.argtypes = [
        _vp, _vp, _vp, ctypes.c_int32, _i32p, ctypes.c_int32, ctypes.c_int32, _dp, ctypes.c_int32,
        ctypes.c_int64, _i32p, ctypes.POINTER(_vp), ctypes.POINTER(_Stats),
    ]
    lib.yawhip_assign_patches.argtypes = [_vp, ctypes.c_int64, _dp, _dp, _dp, ctypes.c_int32, _dp, _i32p]
    lib.yawhip_random_box.argtypes = [
        _vp, ctypes.c_int64, ctypes.c_int64, ctypes.POINTER(ctypes.c_uint64), ctypes.c_int32, ctypes.c_uint32, ctypes.c_double,
        ctypes.c_double, ctypes.c_double, ctypes.c_double, ctypes.c_int64, _dp, _dp, _dp, _dp, _dp, _dp, _i64p,
        ctypes.POINTER(ctypes.c_uint64), _i32p, ctypes.POINTER(ctypes.c_uint32),
    ]
    lib.yawhip_random_healpix.argtypes = [
        _vp, ctypes.c_int64, ctypes.c_int64, ctypes.POINTER(ctypes.c_uint64), ctypes.c_int32, ctypes.c_uint32, ctypes.c_int32,
        ctypes.c_int64, _i64p, _dp, ctypes.c_int64, _dp, _dp, _dp, _dp, _dp, _dp, _i64p, _i64p,
        ctypes.POINTER(ctypes.c_uint64), _i32p, ctypes.POINTER(ctypes.c_uint32),
    ]
    lib.yawhip_healpix_map.argtypes = [_vp, ctypes.c_int64, ctypes.c_int64, _dp, _dp, _dp, ctypes.c_int32, ctypes.c_int32, _i64p, _dp]
    lib.yawhip_healpix_pixels.argtypes = [_vp, ctypes.c_int64, ctypes.c_int64, _dp, _dp, ctypes.c_int32, ctypes.c_int32, ctypes.c_int64,
                                          _i64p, _dp, _dp, _dp, _dp, _i64p]
    lib.yawhip_redshift_histogram.argtypes = [
        _vp, ctypes.c_int64, _dp, _dp, ctypes.c_int32, _i64p, ctypes.c_int32, _dp, ctypes.c_int32, _dp,
    ]
    lib.yawhip_job_work.argtypes = [
        _vp, _vp, _vp, ctypes.c_int32, _i32p, ctypes.c_int32, ctypes.c_int32, _dp, ctypes.c_int32, _i64p,
    ]
    lib.yawhip_host_group_columns.argtypes = [
        ctypes.c_int64, _vp, ctypes.c_int32, ctypes.c_int64, ctypes.c_int32, ctypes.POINTER(_dp), ctypes.POINTER(_dp), _i64p,
        ctypes.c_int32,
    ]
    lib.yawhip_host_scatter_rows.argtypes = [ctypes.c_int64, ctypes.c_int64, _vp, ctypes.c_int64, _vp, _vp, ctypes.c_int64,
                                             ctypes.c_int64, _vp]
    lib.yawhip_kmeans_open.argtypes = [_vp, ctypes.c_int64, _dp, _dp, _dp, _dp, ctypes.c_double, ctypes.POINTER(_vp)]
    lib.yawhip_kmeans_seed.argtypes = [_vp, _dp, ctypes.c_int32, ctypes.POINTER(ctypes.c_uint64)]
    lib.yawhip_kmeans_pick.argtypes = [_vp, ctypes.c_uint64, _i64p]
    lib.yawhip_kmeans_step.argtypes = [_vp, ctypes.c_int32, _dp, _i64p, _i64p, ctypes.POINTER(ctypes.c_uint64), _i32p]
    lib.yawhip_kmeans_query.argtypes = [_vp, ctypes.c_int32, _i64p]
    lib.yawhip_kmeans_close.argtypes = [_vp]
    lib.yawhip_kmeans_close.restype = None
    lib.yawhip_shear_upload.argtypes = [_vp, ctypes.c_int64, _dp, _dp, _dp, _dp, _dp, _dp, ctypes.c_int32, _i64p, ctypes.c_int32,
                                        ctypes.POINTER(_vp)]
    lib.yawhip_shear_free.argtypes = [_vp]
    lib.yawhip_shear_count.argtypes = [_vp, _vp, _vp, ctypes.c_int32, _i32p, ctypes.c_int32, ctypes.c_int32, _dp, _dp, _dp, _dp,
                                       ctypes.POINTER(_Stats)]
    lib.yawhip_shear_upload_binned.argtypes = [_vp, ctypes.c_int64, _dp, _dp, _dp, _dp, _dp, _dp, ctypes.c_int32, ctypes.c_int32,
                                               _i64p, ctypes.c_int32, ctypes.POINTER(_vp)]
    lib.yawhip_shear_auto_count.argtypes = [_vp, _vp, ctypes.c_int32, _i32p, ctypes.c_int32, ctypes.c_int32, _dp, _dp, _dp, _dp, _dp,
                                            ctypes.POINTER(_Stats)]
    lib.yawhip_shear_pair_count.argtypes = [_vp, _vp, _vp, ctypes.c_int32, _i32p, ctypes.c_int32, ctypes.c_int32, _dp, _dp, _dp, _dp,
                                            _dp, ctypes.POINTER(_Stats)]
    lib.yawhip_dsigma_upload_lenses.argtypes = [_vp, ctypes.c_int64, _dp, _dp, _dp, _dp, _dp, _dp, ctypes.c_int32, ctypes.c_int32,
                                                _i64p, ctypes.c_int32, ctypes.POINTER(_vp)]
    lib.yawhip_dsigma_upload_sources.argtypes = [_vp, ctypes.c_int64, _dp, _dp, _dp, _dp, _dp, _dp, _dp, ctypes.c_int32, _i64p,
                                                 ctypes.c_int32, ctypes.POINTER(_vp)]
    lib.yawhip_dsigma_count.argtypes = [_vp, _vp, _vp, ctypes.c_int32, _i32p, ctypes.c_int32, ctypes.c_int32, _dp, _dp, _dp, _dp,
                                        ctypes.POINTER(_Stats)]
    lib.yawhip_dsigma_upload_lenses_radial.argtypes = [_vp, ctypes.c_int64, _dp, _dp, _dp, _dp, _dp, _dp, _dp, ctypes.c_int32,
                                                       ctypes.c_int32, _i64p, ctypes.c_int32, ctypes.POINTER(_vp)]
    lib.yawhip_dsigma_count_radial.argtypes = lib.yawhip_dsigma_count.argtypes
    lib.yawhip_proj_upload.argtypes = lib.yawhip_dsigma_upload_lenses.argtypes
    lib.yawhip_proj_count.argtypes = [_vp, _vp, _vp, ctypes.c_int32, _i32p, ctypes.c_int32, ctypes.c_int32, _dp, ctypes.c_double, _dp,
                                      ctypes.POINTER(_Stats)]
    lib.yawhip_proj_count_pi.argtypes = [_vp, _vp, _vp, ctypes.c_int32, _i32p, ctypes.c_int32, ctypes.c_int32, _dp, ctypes.c_int32, _dp,
                                         _dp, ctypes.POINTER(_Stats)]
    lib.yawhip_proj_count_smu.argtypes = lib.yawhip_proj_count_pi.argtypes
    lib.yawhip_proj_upload_shapes.argtypes = [_vp, ctypes.c_int64, _dp, _dp, _dp, _dp, _dp, _dp, _dp, _dp, ctypes.c_int32, ctypes.c_int32,
                                              _i64p, ctypes.c_int32, ctypes.POINTER(_vp)]
    lib.yawhip_proj_count_shear.argtypes = lib.yawhip_proj_count_pi.argtypes
    lib.yawhip_proj_count_shapes.argtypes = lib.yawhip_proj_count_pi.argtypes
    lib.yawhip_proj_count_pi_signed.argtypes = lib.yawhip_proj_count_pi.argtypes
    lib.yawhip_proj_count_smu_signed.argtypes = lib.yawhip_proj_count_pi.argtypes
    for name in ABI_SYMBOLS:
        fn = getattr(lib, name)
        if name not in ("yawhip_last_error", "yawhip_kmeans_close"):
            fn.restype = ctypes.c_int
    _lib = lib
    return lib


def _check(rc: int, what: str) -> None:
    if rc != 0:
        msg = load_library().yawhip_last_error()
        raise YawhipError(f"{what} failed (status {rc}): {msg.decode() if msg else 'unknown error'}")


def device_count() -> int:
    n = ctypes.c_int(0)
    rc = load_library().yawhip_device_count(ctypes.byref(n))
    return n.value if rc == 0 else 0


def _f64(a):
    return None if a is None else np.ascontiguousarray(a, dtype=np.float64)


def _ptr(a, typ):
    return None if a is None else a.ctypes.data_as(typ)


def _addr(a, dtype):
    """Address of a C-contiguous array of ``dtype`` for a ``c_void_p`` argument (half the cost of ``data_as``)."""
    if a is None:
        return None
    if a.dtype != dtype or not a.flags.c_contiguous:
        raise TypeError(f"expected a C-contiguous {np.dtype(dtype).name} array, got {a.dtype} (contiguous={a.flags.c_contiguous})")
    return a.ctypes.data


class Context:
    """One GPU (one HIP stream), or several GPUs of the node behind one handle (``device`` a sequence of ids:
    catalogues are replicated, ``count_pairs`` splits its jobs over the devices). ``yawhip_ctx`` of include/yawhip.h."""

    def __init__(self, device=0):
        self._h = _vp()
        if isinstance(device, (list, tuple)):
            ids = (ctypes.c_int * len(device))(*[int(d) for d in device])
            _check(load_library().yawhip_ctx_create_multi(ids, len(device), ctypes.byref(self._h)), "yawhip_ctx_create_multi")
            self.devices = tuple(int(d) for d in device)
        else:
            _check(load_library().yawhip_ctx_create(int(device), ctypes.byref(self._h)), "yawhip_ctx_create")
            self.devices = (int(device),)
        self.device = self.devices[0]
        self.strip_micro = DEFAULT_STRIP_MICRO
        self.strip_grid = 1  # the library's default: strip grid uniform in latitude
        self._catalogs = weakref.WeakSet()  # live catalogues: freed before the context (a catalogue's free reads its context)
        self._kmeans = weakref.WeakSet()    # live k-means handles: they use the context's stream
        self._shear = weakref.WeakSet()     # live shear-source handles: freed before the context, as the catalogues

    def set_option(self, key: str, value: int) -> None:
        _check(load_library().yawhip_ctx_set_option(self._h, key.encode(), int(value)), "yawhip_ctx_set_option")
        if key == "strip_width_micro":
            self.strip_micro = int(value)
        elif key == "strip_grid":
            self.strip_grid = int(value)

    def close(self) -> None:
        if getattr(self, "_h", None) is not None and self._h:
            for cat in list(self._catalogs):
                cat.free()
            for km in list(self._kmeans):
                km.close()
            for src in list(self._shear):
                src.free()
            load_library().yawhip_ctx_destroy(self._h)
            self._h = _vp()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class DeviceCatalog:
    """SoA catalogue resident in HBM, sorted by (patch, bin). ``yawhip_catalog``."""

    def __init__(self, ctx: Context, x, y, z, w, n_patches: int, n_bins_or_1: int, offsets, sort_axis: int = 2,
                 strip_micro: int | None = None):
        """``strip_micro``: spacing of the strip grid of the cross-correlation layout in 1e-6 rad of
        latitude -- 1e-6 chord units where the context's ``strip_grid`` option is 0 (linear in v) --
        (0 = no strips, None = whatever the context is set to)."""
        x, y, z, w, offsets = self._prepare(ctx, x, y, z, w, n_patches, n_bins_or_1, offsets, sort_axis, strip_micro)
        _check(
            load_library().yawhip_catalog_upload_axis(
                ctx._h, self.n, _ptr(x, _dp), _ptr(y, _dp), _ptr(z, _dp), _ptr(w, _dp), self.n_patches, self.n_bins,
                _ptr(offsets, _i64p), int(sort_axis), ctypes.byref(self._h),
            ),
            "yawhip_catalog_upload_axis",
        )
        ctx._catalogs.add(self)

    def _prepare(self, ctx, x, y, z, w, n_patches, n_bins_or_1, offsets, sort_axis, strip_micro, weighted=None):
        """Checks and attributes shared by the two ways a catalogue reaches the device; returns the arrays as the library
        takes them."""
        x, y, z, w = _f64(x), _f64(y), _f64(z), _f64(w)
        offsets = np.ascontiguousarray(offsets, dtype=np.int64)
        n = len(x)
        if not (len(y) == n and len(z) == n and (w is None or len(w) == n)):
            raise ValueError("catalogue columns differ in length")
        if len(offsets) != n_patches * n_bins_or_1 + 1:
            raise ValueError("offsets must have n_patches * n_bins_or_1 + 1 entries")
        self.ctx = ctx  # keep the context alive
        self.n, self.n_patches, self.n_bins = n, int(n_patches), int(n_bins_or_1)
        self.weighted = (w is not None) if weighted is None else bool(weighted)
        self._h = _vp()
        if strip_micro is not None:
            ctx.set_option("strip_width_micro", int(strip_micro))
            ctx.strip_micro = int(strip_micro)
        self.strip_micro = ctx.strip_micro
        self.strip_grid = ctx.strip_grid
        self.sort_axis = int(sort_axis)
        return x, y, z, w, offsets

    @classmethod
    def upload_scalar(cls, ctx: Context, x, y, z, w, kappa, n_patches: int, n_bins_or_1: int, offsets, sort_axis: int = 2,
                      strip_micro: int | None = None):
        """``yawhip_catalog_upload_scalar``: the plain catalogue and its twin weighted by ``kappa * w`` (``kappa`` without
        ``w``) from one copy of the coordinates and one segment sort -> ``(cat_n, cat_k)``."""
        cat_n, cat_k = cls.__new__(cls), cls.__new__(cls)
        kappa = _f64(kappa)
        x, y, z, w, offsets = cat_n._prepare(ctx, x, y, z, w, n_patches, n_bins_or_1, offsets, sort_axis, strip_micro)
        cat_k._prepare(ctx, x, y, z, w, n_patches, n_bins_or_1, offsets, sort_axis, None, weighted=True)
        if len(kappa) != cat_n.n:
            raise ValueError("catalogue columns differ in length")
        _check(
            load_library().yawhip_catalog_upload_scalar(
                ctx._h, cat_n.n, _ptr(x, _dp), _ptr(y, _dp), _ptr(z, _dp), _ptr(w, _dp), _ptr(kappa, _dp), cat_n.n_patches,
                cat_n.n_bins, _ptr(offsets, _i64p), int(sort_axis), ctypes.byref(cat_n._h), ctypes.byref(cat_k._h),
            ),
            "yawhip_catalog_upload_scalar",
        )
        ctx._catalogs.add(cat_n)
        ctx._catalogs.add(cat_k)
        return cat_n, cat_k

    def segment_sums(self) -> np.ndarray:
        """``yawhip_catalog_segment_sums``: float64[P, B_or_1] sum of the weight column per (patch, bin) segment, summed on
        the device in a fixed order (object counts for an unweighted catalogue)."""
        out = np.empty((self.n_patches, self.n_bins), dtype=np.float64)
        _check(load_library().yawhip_catalog_segment_sums(self._h, _ptr(out, _dp)), "yawhip_catalog_segment_sums")
        return out

    @property
    def device_bytes(self) -> int:
        b = ctypes.c_int64(0)
        _check(load_library().yawhip_catalog_device_bytes(self._h, ctypes.byref(b)), "yawhip_catalog_device_bytes")
        return b.value

    def free(self) -> None:
        if getattr(self, "_h", None) is not None and self._h:
            load_library().yawhip_catalog_free(self._h)
            self._h = _vp()

    def __del__(self):
        try:
            self.free()
        except Exception:
            pass


def count_pairs(ctx: Context, c1: DeviceCatalog, c2: DeviceCatalog, jobs, thresholds, *, kernel="auto",
                want_counts=None, want_sums=None):
    """Run ``yawhip_count_pairs``.

    jobs: int[n_jobs,2]; thresholds: f64[B,E]. Returns (counts int64[n_jobs,B,E-1] | None,
    sums f64[n_jobs,B,E-1] | None, CountStats)."""
    jobs = np.ascontiguousarray(jobs, dtype=np.int32).reshape(-1, 2)
    t = np.ascontiguousarray(thresholds, dtype=np.float64)
    if t.ndim != 2:
        raise ValueError("thresholds must be [n_bins, n_edges]")
    n_bins, n_edges = t.shape
    weighted = c1.weighted or c2.weighted
    if want_counts is None:
        want_counts = not weighted
    if want_sums is None:
        want_sums = weighted
    shape = (len(jobs), n_bins, max(n_edges - 1, 0))
    counts = np.empty(shape, dtype=np.int64) if want_counts else None   # the library writes every element it is asked for
    sums = np.empty(shape, dtype=np.float64) if want_sums else None
    st = _Stats()
    kid = KERNEL_IDS[kernel] if isinstance(kernel, str) else int(kernel)
    _check(
        load_library().yawhip_count_pairs(
            ctx._h, c1._h, c2._h, len(jobs), _ptr(jobs, _i32p), n_bins, n_edges, _ptr(t, _dp), kid,
            _ptr(counts, _i64p), _ptr(sums, _dp), ctypes.byref(st),
        ),
        "yawhip_count_pairs",
    )
    stats = _count_stats(st)
    return counts, sums, stats


def count_pairs_dense(ctx: Context, c1: DeviceCatalog, c2: DeviceCatalog, jobs, thresholds, slices, fine_factors, halve_diagonal,
                      *, kernel="auto"):
    """Run ``yawhip_count_pairs_dense``: the result tensor f64[S, B, P, P] of ``PatchLinkage.count_pairs`` in one call.

    jobs: int32[n_jobs, 2] (C contiguous); thresholds: f64[B, E]; slices: int32[B, S, 2]; fine_factors: f64[B, E-1] | None."""
    n_bins, n_edges = thresholds.shape
    n_scales = slices.shape[1]
    dense = np.empty((n_scales, n_bins, c1.n_patches, c1.n_patches), dtype=np.float64)  # the library writes every element
    st = _Stats()
    kid = KERNEL_IDS[kernel] if isinstance(kernel, str) else int(kernel)
    _check(
        load_library().yawhip_count_pairs_dense(
            ctx._h, c1._h, c2._h, len(jobs), _addr(jobs, np.int32), n_bins, n_edges, _addr(thresholds, np.float64), kid,
            n_scales, _addr(slices, np.int32), _addr(fine_factors, np.float64), 1 if halve_diagonal else 0, dense.ctypes.data,
            ctypes.byref(st),
        ),
        "yawhip_count_pairs_dense",
    )
    return dense, _count_stats(st)


def count_pairs_dense_batch(ctx: Context, requests, thresholds, slices, fine_factors, *, kernel="auto"):
    """Run ``yawhip_count_pairs_dense_batch``: several counts of one measurement (same thresholds and recombination) on the
    stream at once. ``requests``: sequence of ``(c1, c2, jobs int32[n, 2], halve_diagonal)``. Returns a list of
    ``(dense f64[S, B, P, P], CountStats)`` in the order of the requests."""
    n_bins, n_edges = thresholds.shape
    n_scales = slices.shape[1]
    reqs = (_DenseRequest * len(requests))()
    outs, stats, keep = [], [], []
    for i, (c1, c2, jobs, halve) in enumerate(requests):
        jobs = np.ascontiguousarray(jobs, dtype=np.int32).reshape(-1, 2)
        dense = np.empty((n_scales, n_bins, c1.n_patches, c1.n_patches), dtype=np.float64)  # the library writes every element
        st = _Stats()
        keep.append(jobs)
        outs.append(dense)
        stats.append(st)
        reqs[i].c1, reqs[i].c2 = c1._h, c2._h
        reqs[i].n_jobs, reqs[i].halve_diagonal = len(jobs), 1 if halve else 0
        reqs[i].jobs, reqs[i].dense = jobs.ctypes.data, dense.ctypes.data
        reqs[i].stats = ctypes.addressof(st)
    kid = KERNEL_IDS[kernel] if isinstance(kernel, str) else int(kernel)
    _check(
        load_library().yawhip_count_pairs_dense_batch(
            ctx._h, len(requests), reqs, n_bins, n_edges, _addr(thresholds, np.float64), kid, n_scales,
            _addr(slices, np.int32), _addr(fine_factors, np.float64)),
        "yawhip_count_pairs_dense_batch",
    )
    return [(d, _count_stats(st)) for d, st in zip(outs, stats)]


class DeviceRows:
    """float64[n] in the HBM of ``device``, owned by a context (valid until its next call); exposes
    ``__cuda_array_interface__`` so that torch wraps it without a copy (``torch.as_tensor(rows, device=...)``)."""

    def __init__(self, ptr: int, n: int, device: int):
        self.ptr, self.n, self.device = int(ptr), int(n), int(device)
        self.__cuda_array_interface__ = {"shape": (self.n,), "typestr": "<f8", "data": (self.ptr, False), "version": 3,
                                         "strides": None}


def count_pairs_rows_device(ctx: Context, c1: DeviceCatalog, c2: DeviceCatalog, jobs, thresholds, n_rows_total: int, row_index,
                            *, kernel="auto"):
    """Run ``yawhip_count_pairs_rows_device``: this rank's rows of a sharded count, in place in the full tensor, left on
    the device. Returns (DeviceRows of n_rows_total * B * (E-1) + 1 values, CountStats)."""
    jobs = np.ascontiguousarray(jobs, dtype=np.int32).reshape(-1, 2)
    t = np.ascontiguousarray(thresholds, dtype=np.float64)
    row_index = np.ascontiguousarray(row_index, dtype=np.int32)
    n_bins, n_edges = t.shape
    st = _Stats()
    out = _vp()
    kid = KERNEL_IDS[kernel] if isinstance(kernel, str) else int(kernel)
    _check(
        load_library().yawhip_count_pairs_rows_device(
            ctx._h, c1._h, c2._h, len(jobs), _ptr(jobs, _i32p), n_bins, n_edges, _ptr(t, _dp), kid,
            int(n_rows_total), _ptr(row_index, _i32p), ctypes.byref(out), ctypes.byref(st),
        ),
        "yawhip_count_pairs_rows_device",
    )
    n = int(n_rows_total) * n_bins * (n_edges - 1) + 1
    return DeviceRows(out.value, n, ctx.device), _count_stats(st)


def job_work(ctx: Context, c1: DeviceCatalog, c2: DeviceCatalog, jobs, thresholds, *, kernel="auto") -> np.ndarray:
    """Run ``yawhip_job_work``: evaluated pair distances per job (int64[n_jobs]), nothing is counted."""
    jobs = np.ascontiguousarray(jobs, dtype=np.int32).reshape(-1, 2)
    t = np.ascontiguousarray(thresholds, dtype=np.float64)
    work = np.zeros(len(jobs), dtype=np.int64)
    kid = KERNEL_IDS[kernel] if isinstance(kernel, str) else int(kernel)
    _check(
        load_library().yawhip_job_work(ctx._h, c1._h, c2._h, len(jobs), _ptr(jobs, _i32p), t.shape[0], t.shape[1],
                                       _ptr(t, _dp), kid, _ptr(work, _i64p)),
        "yawhip_job_work",
    )
    return work


RANDOM_MAX_DATA = 1 << 32  # yawhip_random_box / _healpix: most attached values (numpy's 32-bit bounded-integer path)


def _random_call(symbol: str, ctx: Context, n: int, chunksize: int, state: dict, shape_args, n_data: int, data_w, data_z,
                 want_idx: bool, want_pix: bool):
    """The call both generators make: ``shape_args`` are the arguments between the state and ``n_data`` (the box, or the
    map). Returns ``(x, y, w, z, idx, pix, end_state)``."""
    if state.get("bit_generator") != "PCG64":
        raise ValueError(f"{symbol} follows numpy's PCG64 stream only")
    data_w, data_z = _f64(data_w), _f64(data_z)
    n = int(n)
    x, y = np.empty(n, dtype=np.float64), np.empty(n, dtype=np.float64)
    w = None if data_w is None else np.empty(n, dtype=np.float64)
    z = None if data_z is None else np.empty(n, dtype=np.float64)
    idx = np.empty(n, dtype=np.int64) if want_idx else None
    pix = np.empty(n, dtype=np.int64) if want_pix else None
    mask = (1 << 64) - 1
    s, inc = int(state["state"]["state"]), int(state["state"]["inc"])
    words = (ctypes.c_uint64 * 4)(s >> 64, s & mask, inc >> 64, inc & mask)
    out = (ctypes.c_uint64 * 2)()
    has_out, uint_out = ctypes.c_int32(0), ctypes.c_uint32(0)
    outputs = [_ptr(x, _dp), _ptr(y, _dp), _ptr(w, _dp), _ptr(z, _dp), _ptr(idx, _i64p)]
    if symbol == "yawhip_random_healpix":
        outputs.append(_ptr(pix, _i64p))
    _check(
        getattr(load_library(), symbol)(
            ctx._h, n, int(chunksize), words, int(state["has_uint32"]), int(state["uinteger"]), *shape_args, int(n_data),
            _ptr(data_w, _dp), _ptr(data_z, _dp), *outputs, out, ctypes.byref(has_out), ctypes.byref(uint_out)),
        symbol,
    )
    end = {"bit_generator": "PCG64", "state": {"state": (int(out[0]) << 64) | int(out[1]), "inc": inc},
           "has_uint32": int(has_out.value), "uinteger": int(uint_out.value)}
    return x, y, w, z, idx, pix, end


def random_box(ctx: Context, n: int, chunksize: int, state: dict, x_min: float, x_range: float, y_min: float, y_range: float,
               n_data: int = -1, data_w=None, data_z=None, *, want_idx: bool = False):
    """Run ``yawhip_random_box``: ``n`` values of BoxRandoms drawn in chunks of ``chunksize`` from numpy's PCG64 stream.
    ``state`` is ``Generator.bit_generator.state`` before the first chunk. Returns ``(x, y, w, z, idx, end_state)``: float64[n]
    columns (``w`` / ``z`` None without ``data_w`` / ``data_z``), int64[n] indices (None unless ``want_idx``) and the
    bit-generator state numpy is left in after the same draws."""
    box = (float(x_min), float(x_range), float(y_min), float(y_range))
    x, y, w, z, idx, _, end = _random_call("yawhip_random_box", ctx, n, chunksize, state, box, n_data, data_w, data_z,
                                           want_idx, False)
    return x, y, w, z, idx, end


def random_healpix(ctx: Context, n: int, chunksize: int, state: dict, order: int, ipix_unmasked, cdf, n_data: int = -1, data_w=None,
                   data_z=None, *, want_idx: bool = False, want_pix: bool = False):
    """Run ``yawhip_random_healpix``: ``n`` values of HealPixRandoms drawn in chunks of ``chunksize`` from numpy's PCG64 stream,
    from the nested map of ``order`` whose unmasked pixels are ``ipix_unmasked`` with cumulative probabilities ``cdf``. Returns
    ``(x, y, w, z, idx, pix, end_state)`` as :func:`random_box` does, with the drawn order-29 pixels (None unless ``want_pix``)."""
    ipix, cdf = np.ascontiguousarray(ipix_unmasked, dtype=np.int64), _f64(cdf)
    if len(cdf) != len(ipix):
        raise ValueError("ipix_unmasked and cdf differ in length")
    shape_args = (int(order), len(ipix), _ptr(ipix, _i64p), _ptr(cdf, _dp))
    return _random_call("yawhip_random_healpix", ctx, n, chunksize, state, shape_args, n_data, data_w, data_z, want_idx, want_pix)


def group_columns(keys, num_groups: int, columns, n_threads: int = 0):
    """``yawhip_host_group_columns``: stable grouping of float64 columns by integer key (host threads, no device).
    Returns ``(grouped columns, sizes)``; entries with a negative key are dropped. Equivalent to
    ``order = np.flatnonzero(keys >= 0)[np.argsort(keys[keys >= 0], kind="stable")]; [c[order] for c in columns]``."""
    keys = np.ascontiguousarray(keys)
    if keys.dtype not in (np.dtype(np.int32), np.dtype(np.int64)):
        keys = keys.astype(np.int64)
    cols = [_f64(c) for c in columns]
    n = len(keys)
    if any(len(c) != n for c in cols):
        raise ValueError("columns and keys differ in length")
    outs = [np.empty(n, dtype=np.float64) for _ in cols]
    sizes = np.zeros(int(num_groups), dtype=np.int64)
    arr = _dp * max(len(cols), 1)
    _check(
        load_library().yawhip_host_group_columns(
            n, keys.ctypes.data_as(_vp), keys.dtype.itemsize, int(num_groups), len(cols),
            arr(*[_ptr(c, _dp) for c in cols]), arr(*[_ptr(o, _dp) for o in outs]), _ptr(sizes, _i64p), int(n_threads)),
        "yawhip_host_group_columns",
    )
    kept = int(sizes.sum())
    return [o[:kept] for o in outs], sizes


def scatter_rows(shape, cols, vals, col_factor=None) -> np.ndarray:
    """``yawhip_host_scatter_rows``: zeros(shape) viewed as [rows, row_len] with ``out[r, cols[j]] = vals[..., j]``
    (times ``col_factor[j]``). ``cols`` int64[n]; ``vals`` float64[..., n], its leading axes are the rows (any strides
    that make the rows equidistant, e.g. a transposed view of the job-major device result)."""
    out = np.empty(shape, dtype=np.float64)
    n_cols = len(cols)
    if n_cols == 0 or vals.size == 0:
        out[...] = 0.0
        return out
    vals2 = vals.reshape(-1, n_cols) if vals.ndim != 2 else vals  # a view whenever the strides allow it
    if vals2.dtype != np.float64 or vals2.strides[0] % 8 or vals2.strides[1] % 8:
        vals2 = np.ascontiguousarray(vals2, dtype=np.float64)
    n_rows = vals2.shape[0]
    if out.size % n_rows or cols.dtype != np.int64 or not cols.flags.c_contiguous:
        raise ValueError("scatter_rows: shape / cols do not fit the values")
    rc = load_library().yawhip_host_scatter_rows(
        n_rows, out.size // n_rows, out.ctypes.data, n_cols, cols.ctypes.data, vals2.ctypes.data,
        vals2.strides[0] // 8, vals2.strides[1] // 8, None if col_factor is None else col_factor.ctypes.data)
    _check(rc, "yawhip_host_scatter_rows")
    return out


def assign_patches(ctx: Context, x, y, z, centers_xyz) -> np.ndarray:
    """Run ``yawhip_assign_patches``: index of the nearest centre for every object (int32[n])."""
    x, y, z = _f64(x), _f64(y), _f64(z)
    centers = np.ascontiguousarray(centers_xyz, dtype=np.float64).reshape(-1, 3)
    out = np.empty(len(x), dtype=np.int32)
    _check(
        load_library().yawhip_assign_patches(ctx._h, len(x), _ptr(x, _dp), _ptr(y, _dp), _ptr(z, _dp), len(centers),
                                             _ptr(centers, _dp), _ptr(out, _i32p)),
        "yawhip_assign_patches",
    )
    return out


class KMeans:
    """``yawhip_kmeans``: the columns of a catalogue resident on the device for the full-catalogue k-means of ``patches.py``
    (the arithmetic is written out there). ``x, y, z``: float64 unit vectors; ``w``: finite float64 weights or None, with
    ``wscale`` the power of two that brings ``max |w|`` below 2^30. Closes on ``__exit__`` / ``__del__``; closing twice is
    harmless."""

    PATH_NAMES = {0: None, 1: "lds", 2: "global"}

    def __init__(self, ctx: Context, x, y, z, w=None, wscale: float = 0.0):
        self._h = _vp()
        x, y, z, w = _f64(x), _f64(y), _f64(z), _f64(w)
        n = len(x)
        if not (len(y) == n and len(z) == n and (w is None or len(w) == n)):
            raise ValueError("k-means columns differ in length")
        self.ctx, self.n, self.weighted = ctx, n, w is not None  # (keeps the context alive)
        _check(load_library().yawhip_kmeans_open(ctx._h, n, _ptr(x, _dp), _ptr(y, _dp), _ptr(z, _dp), _ptr(w, _dp), float(wscale),
                                                 ctypes.byref(self._h)), "yawhip_kmeans_open")
        ctx._kmeans.add(self)

    def seed(self, centre, first: bool) -> int:
        """One k-means++ step against ``centre`` (three float64): the exact total of ``q = floor(m 2^29)``."""
        c = np.ascontiguousarray(centre, dtype=np.float64).reshape(3)
        total = ctypes.c_uint64(0)
        _check(load_library().yawhip_kmeans_seed(self._h, _ptr(c, _dp), 1 if first else 0, ctypes.byref(total)), "yawhip_kmeans_seed")
        return int(total.value)

    def pick(self, r: int) -> int:
        """The smallest index whose inclusive prefix sum of the last seed's ``q`` exceeds ``r``."""
        index = ctypes.c_int64(-1)
        _check(load_library().yawhip_kmeans_pick(self._h, int(r), ctypes.byref(index)), "yawhip_kmeans_pick")
        return int(index.value)

    def step(self, centres, *, want_ids: bool = False):
        """One Lloyd round against ``centres`` float64[k, 3] -> ``(sums int64[k, 3], counts int64[k], inertia int, ids int32[n]
        or None)``."""
        centres = np.ascontiguousarray(centres, dtype=np.float64).reshape(-1, 3)
        k = len(centres)
        sums, counts = np.empty((k, 3), dtype=np.int64), np.empty(k, dtype=np.int64)
        ids = np.empty(self.n, dtype=np.int32) if want_ids else None
        inertia = ctypes.c_uint64(0)
        _check(load_library().yawhip_kmeans_step(self._h, k, _ptr(centres, _dp), _ptr(sums, _i64p), _ptr(counts, _i64p),
                                                 ctypes.byref(inertia), _ptr(ids, _i32p)), "yawhip_kmeans_step")
        return sums, counts, int(inertia.value), ids

    def _query(self, what: int) -> int:
        value = ctypes.c_int64(0)
        _check(load_library().yawhip_kmeans_query(self._h, what, ctypes.byref(value)), "yawhip_kmeans_query")
        return int(value.value)

    segment = property(lambda self: self._query(0), doc="objects per segment of the seed sums")
    last_path = property(lambda self: self.PATH_NAMES[self._query(1)], doc='"lds" / "global": where the last step kept its partials')
    max_centres_lds = property(lambda self: self._query(2), doc="largest k whose partials fit the LDS beside the centres")
    max_centres = property(lambda self: self._query(3), doc="largest k of step()")

    def close(self) -> None:
        if getattr(self, "_h", None) is not None and self._h:
            load_library().yawhip_kmeans_close(self._h)
            self._h = _vp()

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class ShearSources:
    """``yawhip_shear_sources``: a shear catalogue resident in HBM, every (patch, bin) segment sorted along ``sort_axis`` -- unit
    vectors, weights (or None) and the shear components ``g1, g2`` (east / north frame, include/yawhip.h); ``offsets``
    int64[P * n_bins + 1] over the segments. ``n_bins = 1`` is the unbinned catalogue ``shear_count`` takes
    (``yawhip_shear_upload``), more the binned one of ``shear_auto_count`` (``yawhip_shear_upload_binned``). ``u`` (unbinned
    handles only) is the extra column ``dsigma_count`` reads, finite and ``>= 0`` (``yawhip_dsigma_upload_sources``); the
    shear counts take such a handle and ignore the column."""

    def __init__(self, ctx: Context, x, y, z, w, g1, g2, n_patches: int, offsets, sort_axis: int = 2, n_bins: int = 1, u=None):
        upload = self._prepare(ctx, (x, y, z, w, g1, g2), u, n_patches, n_bins, offsets, sort_axis)
        if u is not None and n_bins != 1:
            raise ValueError("the column 'u' goes with an unbinned catalogue")
        if u is not None:
            upload("yawhip_dsigma_upload_sources", with_bins=False)
        else:
            upload("yawhip_shear_upload" if self.n_bins == 1 else "yawhip_shear_upload_binned", with_bins=self.n_bins != 1)

    def _prepare(self, ctx, columns, extra, n_patches, n_bins, offsets, sort_axis):
        """What every kind of handle shares: the columns ``x, y, z, w`` and the kind's two, with the column ``extra`` of some
        kinds where it is given, as float64 of one length; the offsets over ``n_patches * n_bins`` segments; the attributes.
        Returns ``upload(symbol, with_bins=True)``, which calls the entry point ``symbol(ctx, n, *columns, n_patches,
        [n_bins,] offsets, sort_axis, &handle)``."""
        self._h = _vp()
        columns = [_f64(c) for c in (columns if extra is None else (*columns, extra))]
        offsets = np.ascontiguousarray(offsets, dtype=np.int64)
        n = len(columns[0])
        if any(c is not None and len(c) != n for c in columns):
            raise ValueError("catalogue columns differ in length")
        if n_bins < 1 or len(offsets) != n_patches * n_bins + 1:
            raise ValueError("offsets must have n_patches * n_bins + 1 entries")
        self.ctx = ctx  # keep the context alive
        self.n, self.n_patches, self.weighted, self.sort_axis = n, int(n_patches), columns[3] is not None, int(sort_axis)
        self.n_bins = int(n_bins)

        def upload(symbol, with_bins=True):
            _check(getattr(load_library(), symbol)(ctx._h, n, *(_ptr(c, _dp) for c in columns), self.n_patches,
                                                   *((self.n_bins,) if with_bins else ()), _ptr(offsets, _i64p), self.sort_axis,
                                                   ctypes.byref(self._h)), symbol)
            ctx._shear.add(self)

        return upload

    def free(self) -> None:
        if getattr(self, "_h", None) is not None and self._h:
            load_library().yawhip_shear_free(self._h)
            self._h = _vp()

    def __del__(self):
        try:
            self.free()
        except Exception:
            pass


class DsigmaLenses(ShearSources):
    """The lenses of ``dsigma_count`` resident in HBM (``yawhip_dsigma_upload_lenses``): every (patch, bin) segment sorted along
    ``sort_axis`` -- unit vectors, weights (or None) and the two columns ``f, c`` (include/yawhip.h: ``D_A(z_l)`` and ``chi_l``
    in the driver), finite and ``>= 0``, kept as they come. The handle is a ``yawhip_shear_sources`` of the lens kind: it is
    freed like any, and the shear counts refuse it. With ``m`` (finite and ``> 0``: the squared transverse distance per radian
    of every lens, in the squared unit of the radii) it is the radial handle ``dsigma_count_radial`` needs
    (``yawhip_dsigma_upload_lenses_radial``); ``dsigma_count`` takes it too and ignores ``m``."""

    def __init__(self, ctx: Context, x, y, z, w, f, c, n_patches: int, n_bins: int, offsets, sort_axis: int = 2, m=None):
        upload = self._prepare(ctx, (x, y, z, w, f, c), m, n_patches, n_bins, offsets, sort_axis)
        self.radial = m is not None
        upload("yawhip_dsigma_upload_lenses_radial" if self.radial else "yawhip_dsigma_upload_lenses")


class ProjHandle(ShearSources):
    """The objects of ``proj_count`` resident in HBM (``yawhip_proj_upload``): every (patch, bin) segment sorted along
    ``sort_axis`` -- unit vectors, weights (or None) and the two columns ``d, c`` (include/yawhip.h: the transverse distance
    per radian, finite and ``> 0``, and the line-of-sight coordinate, finite), kept as they come. The handle is a
    ``yawhip_shear_sources`` of the projected kind: it is freed like any, and every other count refuses it."""

    def __init__(self, ctx: Context, x, y, z, w, d, c, n_patches: int, n_bins: int, offsets, sort_axis: int = 2):
        self._prepare(ctx, (x, y, z, w, d, c), None, n_patches, n_bins, offsets, sort_axis)("yawhip_proj_upload")


class ProjShapesHandle(ShearSources):
    """The shapes of ``proj_count_shear`` resident in HBM (``yawhip_proj_upload_shapes``): every (patch, bin) segment sorted
    along ``sort_axis`` -- unit vectors, weights (or None), the shear components ``g1, g2`` (east / north frame, finite; the
    handle keeps the products ``w g1, w g2`` as a ``ShearSources`` does) and the two columns ``d, c`` of a ``ProjHandle``, kept
    as they come. The handle is a ``yawhip_shear_sources`` of the shape kind: it is freed like any, and every other count
    refuses it."""

    def __init__(self, ctx: Context, x, y, z, w, g1, g2, d, c, n_patches: int, n_bins: int, offsets, sort_axis: int = 2):
        self._prepare(ctx, (x, y, z, w, g1, g2, d, c), None, n_patches, n_bins, offsets, sort_axis)("yawhip_proj_upload_shapes")


def _shear_counts(symbol: str, n_planes: int, handles, table, thresholds, *extra, width: int = 2,
                  rows: str = "thresholds must be [n_bins, n_edges]", stacked: bool = False):
    """What the twelve counts share: ``symbol(*handles, n, table, R, E, thresholds, *extra, n_planes output planes, stats)`` with
    ``table`` int32[n, width] -- jobs (width 2: a cell per job and row, planes f64[n, R, E-1]) or cells (wider: a cell per
    entry, planes f64[n, E-1]) -- and ``thresholds`` f64[R, E] (``rows``: what to say of another shape). Returns the planes
    and the ``CountStats``. ``stacked``: the symbol takes the planes as ONE array f64[n_planes, ...], which is what comes
    back in their place."""
    table = np.ascontiguousarray(table, dtype=np.int32).reshape(-1, width)
    t = np.ascontiguousarray(thresholds, dtype=np.float64)
    if t.ndim != 2:
        raise ValueError(rows)
    n_rows, n_edges = t.shape
    shape = (len(table), n_rows, max(n_edges - 1, 0)) if width == 2 else (len(table), max(n_edges - 1, 0))
    if stacked:
        out = [np.empty((n_planes, *shape), dtype=np.float64)]
    else:
        out = [np.empty(shape, dtype=np.float64) for _ in range(n_planes)]  # the library writes every element
    st = _Stats()
    _check(
        getattr(load_library(), symbol)(*handles, len(table), _ptr(table, _i32p), n_rows, n_edges, _ptr(t, _dp), *extra,
                                        *(_ptr(a, _dp) for a in out), ctypes.byref(st)),
        symbol,
    )
    return (*out, _count_stats(st))


def _pi_counts(symbol: str, per_bin: int, ctx: Context, a, b, cells, r2, pi_edges):
    """What the three counts with pi edges share: ``pi_edges`` as f64[n_pi + 1], ``symbol`` run on ``per_bin * n_pi`` stacked
    planes, and those as ``per_bin`` planes f64[n_pi, n_cells, E-1] each. Returns ``(planes, CountStats)``."""
    pe = np.ascontiguousarray(pi_edges, dtype=np.float64)
    if pe.ndim != 1:
        raise ValueError("pi_edges must be [n_pi + 1]")
    n_pi = len(pe) - 1
    fine, stats = _shear_counts(symbol, per_bin * max(n_pi, 0), (ctx._h, a._h, b._h), cells, r2, n_pi, _ptr(pe, _dp), width=4,
                                rows="r2 must be [n_rows, n_edges]", stacked=True)
    return tuple(fine.reshape(per_bin, max(n_pi, 0), *fine.shape[1:])), stats


def proj_count_pi(ctx: Context, a: ProjHandle, b: ProjHandle, cells, r2, pi_edges):
    """Run ``yawhip_proj_count_pi``: ``proj_count`` with the pairs binned in ``p = |c_a - c_b|`` besides; ``pi_edges``
    f64[n_pi + 1] starts at exactly 0 and ascends strictly, finite but for a last edge that may be ``inf``; bin 0 is
    ``[0, pe[1]]``, bin j ``(pe[j], pe[j + 1]]``. Returns ``(W, CountStats)``, W f64[n_pi, n_cells, E-1]; its sum over the pi
    bins is ``proj_count``'s W at ``pmax = pi_edges[-1]`` (exactly, for unit weights), and the statistics are that call's.
    ``n_pi (E - 1)`` is capped by the LDS of a workgroup (include/yawhip.h); beyond it the library refuses."""
    (fine,), stats = _pi_counts("yawhip_proj_count_pi", 1, ctx, a, b, cells, r2, pi_edges)
    return fine, stats


def proj_count_shear(ctx: Context, dens: ProjHandle, shapes: ProjShapesHandle, cells, r2, pi_edges):
    """Run ``yawhip_proj_count_shear``: the shapes of ``shapes`` rotated to the great circle through each pair with an object of
    ``dens``, binned as ``proj_count_pi`` bins the pair. cells int[n_cells, 4] = ``(segment of dens, segment of shapes, row,
    0)``; ``r2`` and ``pi_edges`` as ``proj_count_pi``. Returns ``((T, X, W), CountStats)``, each plane f64[n_pi, n_cells, E-1]:
    the sums of ``w_d w_s e_t``, ``w_d w_s e_x`` and ``w_d w_s`` with ``e_t`` the tangential ellipticity of the shape about the
    density object (negative where the shape points at it). ``3 n_pi (E - 1)`` is capped by the LDS of a workgroup
    (include/yawhip.h); beyond it the library refuses."""
    return _pi_counts("yawhip_proj_count_shear", 3, ctx, dens, shapes, cells, r2, pi_edges)


def proj_count_shapes(ctx: Context, a: ProjShapesHandle, b: ProjShapesHandle, cells, r2, pi_edges):
    """Run ``yawhip_proj_count_shapes`` on two shape handles (``a is b`` allowed): the shapes of both rotated to the great circle
    through each pair, binned as ``proj_count_pi`` bins the pair. cells int[n_cells, 4] = ``(segment of a, segment of b, row,
    diagonal)`` with ``proj_count``'s rules -- a diagonal cell holds every unordered pair once; ``r2`` and ``pi_edges`` as
    ``proj_count_pi``. Returns ``((PP, XX, PX, W), CountStats)``, each plane f64[n_pi, n_cells, E-1]: the sums of
    ``w_a w_b et_a et_b``, ``w_a w_b ex_a ex_b``, ``w_a w_b (et_a ex_b + ex_a et_b)`` and ``w_a w_b`` with ``et`` the TANGENTIAL
    ellipticity of a shape about its partner, as ``proj_count_shear`` has it: ``e+ = -et``, so PP and XX are the ``++`` and
    ``xx`` products and PX is MINUS the ``+x`` product. ``4 n_pi (E - 1)`` is capped by the LDS of a workgroup
    (include/yawhip.h); beyond it the library refuses."""
    return _pi_counts("yawhip_proj_count_shapes", 4, ctx, a, b, cells, r2, pi_edges)


def proj_count_smu(ctx: Context, a: ProjHandle, b: ProjHandle, cells, s2, m2):
    """Run ``yawhip_proj_count_smu``: the pairs of ``proj_count``'s cells binned by ``S2 = R2 + P2`` (``P2`` the square of
    ``p = |c_a - c_b|``) over the rows ``s2`` f64[n_rows, E] of SQUARED s edges, and by ``mu^2 = P2 / S2`` over the squared mu
    edges ``m2`` f64[n_mu + 1], from exactly 0 to exactly 1 and strictly ascending: a pair is in the plane j that counts the
    inner edges k with ``fl(m2[k] S2) < P2``. There is no line-of-sight cut. Returns ``(W, CountStats)``, W f64[n_mu, n_cells,
    E-1]; the statistics are ``proj_count``'s on the same cells and table. ``n_mu (E - 1)`` is capped by the LDS of a
    workgroup as ``proj_count_pi``'s ``n_pi (E - 1)`` is (include/yawhip.h); beyond it the library refuses."""
    m2 = np.ascontiguousarray(m2, dtype=np.float64)
    if m2.ndim != 1:
        raise ValueError("m2 must be [n_mu + 1]")
    n_mu = len(m2) - 1
    return _shear_counts("yawhip_proj_count_smu", max(n_mu, 0), (ctx._h, a._h, b._h), cells, s2, n_mu, _ptr(m2, _dp), width=4,
                         rows="s2 must be [n_rows, n_edges]", stacked=True)


def proj_count_pi_signed(ctx: Context, a: ProjHandle, b: ProjHandle, cells, r2, pi_edges):
    """Run ``yawhip_proj_count_pi_signed``: ``proj_count_pi`` between two samples with the pairs binned in the SIGNED
    ``ps = c_b - c_a`` (object of ``b`` minus object of ``a``: the sign belongs to the handle order); ``pi_edges`` f64[n_pi + 1]
    finite and strictly ascending, of any sign; a pair counts iff ``pe[0] <= ps <= pe[n_pi]``, bin 0 is ``[pe[0], pe[1]]``, bin j
    ``(pe[j], pe[j + 1]]``. No cell may be diagonal or pair a segment of one handle with itself. Returns ``(W, CountStats)``, W
    f64[n_pi, n_cells, E-1]; over edges mirrored about 0, planes ``n + j`` and ``n - 1 - j`` sum to ``proj_count_pi``'s plane
    j (exactly, for unit weights and no pair at ``ps == 0`` or on an edge). The cap is ``proj_count_pi``'s."""
    (fine,), stats = _pi_counts("yawhip_proj_count_pi_signed", 1, ctx, a, b, cells, r2, pi_edges)
    return fine, stats


def proj_count_smu_signed(ctx: Context, a: ProjHandle, b: ProjHandle, cells, s2, sm2):
    """Run ``yawhip_proj_count_smu_signed``: ``proj_count_smu`` between two samples with mu signed by ``ps = c_b - c_a``. The
    edges ``sm2`` f64[n_mu + 1] are the signed squares ``copysign(mu mu, mu)``, from exactly -1 to exactly 1 and strictly
    ascending: a pair is in the plane j that counts the inner edges k with ``fl(sm2[k] S2) < copysign(P2, ps)``. No cell may
    be diagonal or pair a segment of one handle with itself. Returns ``(W, CountStats)``, W f64[n_mu, n_cells, E-1]. The cap
    is ``proj_count_smu``'s."""
    sm2 = np.ascontiguousarray(sm2, dtype=np.float64)
    if sm2.ndim != 1:
        raise ValueError("sm2 must be [n_mu + 1]")
    n_mu = len(sm2) - 1
    return _shear_counts("yawhip_proj_count_smu_signed", max(n_mu, 0), (ctx._h, a._h, b._h), cells, s2, n_mu, _ptr(sm2, _dp), width=4,
                         rows="s2 must be [n_rows, n_edges]", stacked=True)


def proj_count(ctx: Context, a: ProjHandle, b: ProjHandle, cells, r2, pmax: float):
    """Run ``yawhip_proj_count`` on two projected handles (``a is b`` allowed): cells int[n_cells, 4] = ``(segment of a, segment
    of b, row, diagonal)`` with a segment ``patch * n_bins + bin`` of its handle and ``diagonal`` non-zero iff the cell pairs
    a segment of one handle with itself; ``r2`` f64[n_rows, E] squared radius edges; ``pmax >= 0`` the largest
    ``|c_a - c_b|`` of a pair that counts (``inf``: no cut). Returns ``(W, CountStats)``, W f64[n_cells, E-1]: the sums of
    ``w_a w_b``, a diagonal cell holding every unordered pair once."""
    return _shear_counts("yawhip_proj_count", 1, (ctx._h, a._h, b._h), cells, r2, float(pmax), width=4,
                         rows="r2 must be [n_rows, n_edges]")


def shear_count(ctx: Context, lenses: DeviceCatalog, sources: ShearSources, jobs, thresholds):
    """Run ``yawhip_shear_count``: jobs int[n_jobs, 2] = (lens patch, source patch); thresholds f64[B, E]. Returns
    ``(T, X, W, CountStats)``: the tangential, cross and weight sums, f64[n_jobs, B, E-1] each."""
    return _shear_counts("yawhip_shear_count", 3, (ctx._h, lenses._h, sources._h), jobs, thresholds)


def dsigma_count(ctx: Context, lenses: DsigmaLenses, sources: ShearSources, jobs, thresholds):
    """Run ``yawhip_dsigma_count``: ``lenses`` a ``DsigmaLenses``, ``sources`` a ``ShearSources`` with ``u``; jobs int[n_jobs, 2] =
    (lens patch, source patch); thresholds f64[B, E]. Returns ``(T, X, W, CountStats)``, f64[n_jobs, B, E-1] each: the sums of
    ``w_l w_s S gamma_t``, ``w_l w_s S gamma_x`` and ``w_l w_s S^2`` over the pairs with ``S = f (1 - c u) > 0``."""
    return _shear_counts("yawhip_dsigma_count", 3, (ctx._h, lenses._h, sources._h), jobs, thresholds)


def dsigma_count_radial(ctx: Context, lenses: DsigmaLenses, sources: ShearSources, jobs, r2):
    """Run ``yawhip_dsigma_count_radial``: ``dsigma_count`` with the pairs binned by ``R^2 = m_l theta^2`` of each lens against
    the squared radius edges ``r2`` f64[B, E]; ``lenses`` a ``DsigmaLenses`` with ``m``. Returns ``(T, X, W, CountStats)``."""
    return _shear_counts("yawhip_dsigma_count_radial", 3, (ctx._h, lenses._h, sources._h), jobs, r2)


def shear_auto_count(ctx: Context, sources: ShearSources, jobs, thresholds):
    """Run ``yawhip_shear_auto_count`` on a binned handle: jobs int[n_jobs, 2] = patch pairs with ``p <= q``; thresholds
    f64[B, E]. Returns ``(P, M, C, W, CountStats)``: the numerators of xi_plus, xi_minus and xi_cross and the weight sums,
    f64[n_jobs, B, E-1] each; a diagonal job holds every unordered pair once."""
    return _shear_counts("yawhip_shear_auto_count", 4, (ctx._h, sources._h), jobs, thresholds)


def shear_pair_count(ctx: Context, a: ShearSources, b: ShearSources, cells, thresholds):
    """Run ``yawhip_shear_pair_count`` on two binned handles (``a is b`` allowed): cells int[n_cells, 5] = ``(p, q, ka, kb, row)``
    -- segment ``(p, ka)`` of ``a`` against ``(q, kb)`` of ``b``, classified against thresholds row ``row``; thresholds
    f64[n_rows, E]. Returns ``(P, M, C, W, CountStats)``, f64[n_cells, E-1] each; a cell of one handle with ``ka == kb`` and
    ``p == q`` holds every unordered pair once."""
    return _shear_counts("yawhip_shear_pair_count", 4, (ctx._h, a._h, b._h), cells, thresholds, width=5,
                         rows="thresholds must be [n_rows, n_edges]")


def healpix_map(ctx: Context, phi, z, w, order: int, nested: bool, *, want_pixels: bool = False, want_map: bool = True,
                chunksize: int = 0):
    """Run ``yawhip_healpix_map``: ``(pix, map)`` of the points ``(phi, z)`` at ``order`` -- int64[n] pixels (-1 for a point
    with a non-finite coordinate or ``|z| > 1``) and the float64[12 * 4^order] map of object counts, or of summed ``w`` --
    each ``None`` unless wanted. The arrays go to the library as they are: it checks sizes, not values."""
    phi, z, w = _f64(phi), _f64(z), _f64(w)
    if len(z) != len(phi) or (w is not None and len(w) != len(phi)):
        raise ValueError("phi, z and weights differ in length")
    pix = np.empty(len(phi), dtype=np.int64) if want_pixels else None
    out = np.empty(12 << (2 * order), dtype=np.float64) if want_map and 0 <= order <= 13 else None
    _check(
        load_library().yawhip_healpix_map(ctx._h, len(phi), int(chunksize), _ptr(phi, _dp), _ptr(z, _dp), _ptr(w, _dp), int(order),
                                          int(bool(nested)), _ptr(pix, _i64p), _ptr(out, _dp)),
        "yawhip_healpix_map",
    )
    return pix, out


def healpix_pixels(ctx: Context, values, weights, order: int, nested: bool, capacity: int, *, chunksize: int = 0, outputs=None):
    """Run ``yawhip_healpix_pixels``: the selected pixels of the map ``values`` (with the weight map ``weights``, or None) at
    ``order`` -> ``(n_selected, ipix, phi, z, kappa, w)``, columns of ``capacity`` entries (``w`` None without ``weights``).
    ``capacity`` is the number of selected pixels, counted by the caller; the library raises when it selects another number
    and writes nothing beyond it. ``outputs``: the five arrays (int64, then four float64; the last may be None without
    weights) to write to instead of new ones, each of at least ``capacity`` entries. The maps go to the library as they are."""
    values, weights = _f64(values), _f64(weights)
    capacity = int(capacity)
    if outputs is None:
        outputs = (np.empty(capacity, dtype=np.int64), *(np.empty(capacity, dtype=np.float64) for _ in range(3)),
                   None if weights is None else np.empty(capacity, dtype=np.float64))
    ipix, phi, z, kappa, w = outputs
    for out, dtype in ((ipix, np.int64), (phi, np.float64), (z, np.float64), (kappa, np.float64), (w, np.float64)):
        if out is not None and (out.dtype != dtype or not out.flags.c_contiguous or len(out) < capacity):
            raise ValueError("healpix_pixels: an output is not a contiguous array of its type with 'capacity' entries")
    n_selected = ctypes.c_int64(0)
    _check(
        load_library().yawhip_healpix_pixels(ctx._h, len(values), int(chunksize), _ptr(values, _dp), _ptr(weights, _dp), int(order),
                                             int(bool(nested)), capacity, _ptr(ipix, _i64p), _ptr(phi, _dp), _ptr(z, _dp),
                                             _ptr(kappa, _dp), _ptr(w, _dp), ctypes.byref(n_selected)),
        "yawhip_healpix_pixels",
    )
    return int(n_selected.value), ipix, phi, z, kappa, w


def redshift_histogram(ctx: Context, z, w, offsets, edges, closed_right: bool) -> np.ndarray:
    """Run ``yawhip_redshift_histogram``: per-patch histogram (float64[P, B]) of the redshifts ``z`` grouped by patch
    (``offsets`` int64[P + 1]); object counts without ``w``, sums of weights with it."""
    z, w, edges = _f64(z), _f64(w), _f64(edges)
    offsets = np.ascontiguousarray(offsets, dtype=np.int64)
    if w is not None and len(w) != len(z):
        raise ValueError("redshifts and weights differ in length")
    n_patches, n_edges = len(offsets) - 1, len(edges)
    out = np.empty((max(n_patches, 0), max(n_edges - 1, 0)), dtype=np.float64)
    _check(
        load_library().yawhip_redshift_histogram(ctx._h, len(z), _ptr(z, _dp), _ptr(w, _dp), n_patches, _ptr(offsets, _i64p), n_edges,
                                                 _ptr(edges, _dp), int(bool(closed_right)), _ptr(out, _dp)),
        "yawhip_redshift_histogram",
    )
    return out
