"""Device session: one ``yawhip`` context per process, catalogue layouts uploaded once and kept
resident in HBM, and the call that counts the fine-bin pairs for a list of jobs.

``count_fine`` is the single seam between the host driver (measurements.py) and the HIP library.
It has no CPU fallback; the multi-process CPU tests replace it with the oracle to exercise the
sharding / reduction logic without a GPU.
"""
from __future__ import annotations

import numpy as np

import os
import re

from . import _lib
from .parallel import local_device_index, world

__all__ = ["get_context", "device_catalog", "count_fine", "count_shear_fine", "count_shear_auto_fine", "count_shear_pair_fine", "count_dsigma_fine", "dsigma_columns", "count_dsigma_radial_fine", "dsigma_radial_columns", "radial_kind", "radial_reach", "check_radial_reach", "proj_columns", "check_proj_redshifts", "check_pi_max", "check_pi_edges", "check_mu_edges", "check_signed_pi_edges", "check_signed_mu_edges", "count_projected_pi_signed_fine", "count_smu_signed_fine", "count_projected_fine", "count_projected_pi_fine", "count_projected_shear_fine", "count_projected_shapes_fine", "max_shape_pi_bins", "count_smu_fine", "check_projected_reach", "count_dense", "count_dense_batch", "job_work", "assign_patches", "kmeans_open", "draw_box_randoms", "draw_healpix_randoms",
           "healpix_map", "healpix_pixels", "redshift_histogram", "scalar_segment_sums", "release", "default_kernel"]

_contexts: dict = {}
default_kernel = "auto"
forced_strip_micro: int | None = None  # set to pin the strip grid spacing (bench / experiments)


def default_devices(max_workers: int | None = None) -> tuple:
    """GPUs one process counts on. Inside a ``torch.distributed`` group (one process per GPU) that is the process'
    own device; a single process takes every visible GPU (``YAW_AMD_DEVICES="0,1,2"`` picks them explicitly, an id
    may repeat) -- the counterpart of the reference's worker pool, so ``max_workers`` caps their number
    (src/yaw/utils/parallel.py:145-150). Launchers that start one process per GPU without setting LOCAL_RANK (mpirun,
    srun) must set ``YAW_AMD_DEVICE`` (or a one-id ``YAW_AMD_DEVICES``) per process, or every process takes every GPU.
    Inside a group the collectives run on the counting context's device (``Context.device``); a context of SEVERAL
    devices inside a group counts through the host route (``PatchLinkage.count_pairs``)."""
    env = os.environ.get("YAW_AMD_DEVICES")
    if env:
        devices = [int(v) for v in env.split(",") if v.strip() != ""]
    elif world()[1] > 1 or "LOCAL_RANK" in os.environ or "YAW_AMD_DEVICE" in os.environ:
        devices = [local_device_index()]
    else:
        devices = list(range(max(_lib.device_count(), 1)))
    if max_workers is not None and max_workers >= 1:
        devices = devices[: int(max_workers)]
    return tuple(devices)


def get_context(device=None, max_workers: int | None = None) -> "_lib.Context":
    """The context of ``device`` (an id or a sequence of ids), by default of :func:`default_devices`."""
    if device is None:
        device = default_devices(max_workers)
    key = tuple(int(d) for d in device) if isinstance(device, (list, tuple)) else (int(device),)
    ctx = _contexts.get(key)
    if ctx is None:
        ctx = _contexts[key] = _lib.Context(key[0] if len(key) == 1 else list(key))
    return ctx


def release() -> None:
    """Destroy all contexts (device catalogues must have been freed before)."""
    for ctx in _contexts.values():
        ctx.close()
    _contexts.clear()


_strip_micro_cache: dict = {}


def strip_micro_for(thresholds) -> int:
    """Spacing of the strip grid (1e-6 rad of latitude) that suits the widest separation of a threshold
    table: just above the largest separation angle, so that a run has partners in three strips only and
    those are as narrow as possible. Measured on the 10M x 10M headline (chord 2909): 2950 -> 2.09 ms per step,
    3600 -> 2.16, 4400 -> 2.21, 5200 -> 2.28; below the chord five strips take part (2000: 30 % slower)."""
    key = (id(thresholds), thresholds.shape)
    hit = _strip_micro_cache.get(key)
    if hit is not None and hit[0] is thresholds:  # threshold tables are built once per configuration and never modified
        return hit[1]
    theta = 2.0 * float(np.arcsin(min(1.0, 0.5 * float(np.sqrt(np.max(thresholds))))))  # chord -> angle
    micro = int(min(max(np.ceil(1.02e6 * theta / 50.0) * 50.0, 1000), 100000))
    if len(_strip_micro_cache) > 16:
        _strip_micro_cache.clear()
    _strip_micro_cache[key] = (thresholds, micro)
    return micro


def device_catalog(layout, ctx=None, sort_axis: int = 2, strip_micro: int | None = None,
                   exact: bool = False) -> "_lib.DeviceCatalog":
    """Upload (once per context) and return the device copy of a layout. ``sort_axis`` is the
    coordinate the library sorts segments by for its window culling; ``strip_micro`` the wanted
    spacing of the strip grid. A copy made for another axis, or for a grid more than 1.6 x off the
    wanted spacing (``exact``: any other spacing), is replaced. A layout with a scalar field and its ``ScalarTwin`` reach the
    device together (``yawhip_catalog_upload_scalar``: one copy of the coordinates, one segment sort, two catalogues), and
    are replaced together."""
    ctx = ctx or get_context()
    dev = layout.device.get(id(ctx))
    if dev is not None:
        stale = dev.sort_axis != sort_axis or dev.strip_grid != ctx.strip_grid
        if strip_micro is not None and not stale:
            have = dev.strip_micro
            stale = have != strip_micro if (exact or have == 0 or strip_micro == 0) else \
                not (strip_micro / 1.6 <= have <= strip_micro * 1.6)
        if stale:
            dev.free()
            dev = None
    if dev is None:
        base = getattr(layout, "base", layout)  # (of a ScalarTwin: the layout it weights)
        if base.kappa is None:
            dev = _lib.DeviceCatalog(ctx, layout.x, layout.y, layout.z, layout.w, layout.num_patches, layout.num_bins,
                                     layout.offsets, sort_axis=sort_axis, strip_micro=strip_micro)
            layout.device[id(ctx)] = dev
        else:
            for held in (base, base.twin):
                old = held.device.pop(id(ctx), None)
                if old is not None:
                    old.free()
            base.device[id(ctx)], base.twin.device[id(ctx)] = _lib.DeviceCatalog.upload_scalar(
                ctx, base.x, base.y, base.z, base.w, base.kappa, base.num_patches, base.num_bins, base.offsets,
                sort_axis=sort_axis, strip_micro=strip_micro)
            dev = layout.device[id(ctx)]
    return dev


def count_fine(layout1, layout2, jobs, thresholds, *, kernel: str | None = None, sort_axis: int = 2,
               max_workers: int | None = None):
    """Fine-bin pair counts for ``jobs`` (int[n,2]) -> (f64[n_jobs, B, E-1], CountStats).

    Unweighted catalogues are counted in int64 on the device and converted exactly
    (the reference's ``.astype(np.float64)``, trees.py:353). With several GPUs in the process' context the library
    splits the jobs over them; ``max_workers`` caps how many are used."""
    ctx, d1, d2 = _device_pair(layout1, layout2, thresholds, sort_axis, max_workers)
    counts, sums, stats = _lib.count_pairs(ctx, d1, d2, jobs, thresholds, kernel=kernel or default_kernel)
    fine = sums if sums is not None else counts.astype(np.float64)
    return fine, stats


def count_dense(layout1, layout2, jobs, thresholds, slices, fine_factors, halve_diagonal, *, kernel: str | None = None,
                sort_axis: int = 2, max_workers: int | None = None):
    """The result tensor f64[S, B, P, P] of one pair count from ONE library call (``yawhip_count_pairs_dense``) and its
    ``CountStats``; ``slices`` / ``fine_factors`` describe the per-scale recombination (``CombinePlan.dense_spec``)."""
    ctx, d1, d2 = _device_pair(layout1, layout2, thresholds, sort_axis, max_workers)
    return _lib.count_pairs_dense(ctx, d1, d2, np.ascontiguousarray(jobs, dtype=np.int32).reshape(-1, 2),
                                  np.ascontiguousarray(thresholds, dtype=np.float64), slices, fine_factors, halve_diagonal,
                                  kernel=kernel or default_kernel)


def count_dense_batch(pairs, thresholds, slices, fine_factors, *, kernel: str | None = None, sort_axis: int = 2,
                      max_workers: int | None = None):
    """Several counts of one measurement from ONE library call (``yawhip_count_pairs_dense_batch``): ``pairs`` is a
    sequence of ``(layout1, layout2, jobs, halve_diagonal)``; all catalogues are uploaded (once) first, then every count is
    put on the stream. Returns ``[(f64[S, B, P, P], CountStats), ...]`` in the order of ``pairs``."""
    requests, ctx = [], None
    for _ in range(3):  # an upload may replace a copy made for another strip grid -- one an earlier pair refers to: look again
        requests = []
        for layout1, layout2, jobs, halve in pairs:
            ctx, d1, d2 = _device_pair(layout1, layout2, thresholds, sort_axis, max_workers)
            requests.append((d1, d2, jobs, halve))
        if all(d1._h and d2._h for d1, d2, _, _ in requests):
            break
    else:
        raise _lib.YawhipError("count_dense_batch: the catalogues of the batch do not settle on one strip grid")
    if not requests:
        return []
    return _lib.count_pairs_dense_batch(ctx, requests, np.ascontiguousarray(thresholds, dtype=np.float64), slices, fine_factors,
                                        kernel=kernel or default_kernel)


def count_rows_device(layout1, layout2, jobs, thresholds, n_rows_total: int, row_index, *, kernel: str | None = None,
                      sort_axis: int = 2):
    """This rank's share of a sharded count, left on the device in its place of the full [jobs, B, E-1] tensor
    (``yawhip_count_pairs_rows_device``) -> (``_lib.DeviceRows``, CountStats)."""
    ctx, d1, d2 = _device_pair(layout1, layout2, thresholds, sort_axis)
    return _lib.count_pairs_rows_device(ctx, d1, d2, jobs, thresholds, n_rows_total, row_index, kernel=kernel or default_kernel)


def _require_shear(*layouts) -> None:
    if any(layout.g1 is None or layout.g2 is None for layout in layouts):
        raise ValueError("catalog has no 'g1'/'g2' attached")


def count_shear_fine(lens_layout, source_layout, jobs, thresholds, *, sort_axis: int = 2):
    """Fine-bin shear sums for ``jobs`` (int[n, 2] = (lens patch, source patch)) -> ``(T, X, W, CountStats)``, f64[n_jobs, B, E-1]
    each: tangential and cross shear sums and the sum of ``w_l * w_s`` of the pairs (``yawhip_shear_count``). The lenses are the
    resident catalogue of ``lens_layout``; the sources (an unbinned layout with ``g1`` / ``g2``) reach the device once per
    context as a ``_lib.ShearSources`` kept on the layout, replaced when another sort axis is asked for. On a context of
    several devices the count runs on its first one. No CPU fallback; the CPU tests replace this function."""
    _require_shear(source_layout)
    ctx = get_context()
    micro = forced_strip_micro if forced_strip_micro is not None else strip_micro_for(thresholds)
    lenses = device_catalog(lens_layout, ctx, sort_axis, micro, exact=forced_strip_micro is not None)
    return _lib.shear_count(ctx, lenses, _shear_handle(source_layout, ctx, sort_axis), jobs, thresholds)


def count_shear_auto_fine(layout, jobs, thresholds, *, sort_axis: int = 2):
    """Fine-bin shear-shear sums of ONE catalogue inside its redshift bins for ``jobs`` (int[n, 2] patch pairs with ``p <= q``)
    -> ``(P, M, C, W, CountStats)``, f64[n_jobs, B, E-1] each: the numerators of xi_plus, xi_minus and xi_cross and the sum of
    ``w_a * w_b`` of the pairs, a diagonal job holding every unordered pair once (``yawhip_shear_auto_count``). ``layout`` is a
    binned layout with ``g1`` / ``g2`` (``build_trees(edges, with_shear=True)``); it reaches the device once per context as a
    binned ``_lib.ShearSources`` kept on the layout, replaced when another sort axis is asked for. On a context of several
    devices the count runs on its first one. No CPU fallback; the CPU tests replace this function."""
    _require_shear(layout)
    ctx = get_context()
    return _lib.shear_auto_count(ctx, _shear_handle(layout, ctx, sort_axis), jobs, thresholds)


def count_shear_pair_fine(layout_a, layout_b, cells, thresholds, *, sort_axis: int = 2):
    """Fine-bin shear-shear sums between (patch, bin) segments of one or two catalogues for ``cells`` (int[n, 5] =
    ``(p, q, ka, kb, row)``: segment ``(p, ka)`` of ``layout_a`` against ``(q, kb)`` of ``layout_b``, thresholds row ``row``) ->
    ``(P, M, C, W, CountStats)``, f64[n_cells, E-1] each (``yawhip_shear_pair_count``). Both are binned layouts with ``g1`` /
    ``g2``, resident as for ``count_shear_auto_fine``; the same layout twice is ONE handle passed twice, and only then a cell
    with ``p == q`` and ``ka == kb`` holds every unordered pair once. No CPU fallback; the CPU tests replace this function."""
    _require_shear(layout_a, layout_b)
    ctx = get_context()
    a = _shear_handle(layout_a, ctx, sort_axis)
    b = a if layout_b is layout_a else _shear_handle(layout_b, ctx, sort_axis)
    return _lib.shear_pair_count(ctx, a, b, cells, thresholds)


def dsigma_columns(lens_layout, source_layout, cosmology):
    """The three columns ``yawhip_dsigma_count`` reads (include/yawhip.h), from the layouts' redshifts
    (``build_trees(with_redshifts=True)``) and ``cosmology`` (assumed flat): ``(f, c, u)`` = ``D_A(z_l)`` and ``chi(z_l)`` of
    the lenses and ``1 / chi(z_s)`` of the sources, Mpc and 1/Mpc, each in its layout's order. Redshifts must be finite and
    ``>= 0``, the distances finite, and a source needs ``chi_s > 0`` (``ValueError`` otherwise). A side given as ``None`` is
    skipped (``None`` in its place)."""
    from .cosmology import distance_column

    def redshifts(layout, what):
        z = layout.redshifts
        if z is None:
            raise ValueError(f"the {what} carry no redshifts: build_trees(..., with_redshifts=True)")
        if not (np.all(np.isfinite(z)) and np.all(z >= 0.0)):
            raise ValueError(f"the redshifts of the {what} must be finite and >= 0")
        return z

    f = c = u = None
    if lens_layout is not None:
        z = redshifts(lens_layout, "lenses")
        f, c = distance_column(cosmology, z, kind="angular"), distance_column(cosmology, z, kind="comoving")
        if not (np.all(np.isfinite(f)) and np.all(f >= 0.0) and np.all(np.isfinite(c)) and np.all(c >= 0.0)):
            raise ValueError("the cosmology gives lens distances that are not finite numbers >= 0")
    if source_layout is not None:
        chi = distance_column(cosmology, redshifts(source_layout, "sources"), kind="comoving")
        if not (np.all(np.isfinite(chi)) and np.all(chi > 0.0)):
            raise ValueError("a source needs a finite comoving distance > 0 (a redshift > 0)")
        u = 1.0 / chi
    return f, c, u


def count_dsigma_fine(lens_layout, source_layout, jobs, thresholds, *, cosmology, sort_axis: int = 2):
    """Fine-bin excess-surface-density sums for ``jobs`` (int[n, 2] = (lens patch, source patch)) -> ``(T, X, W, CountStats)``,
    f64[n_jobs, B, E-1] each: the sums of ``w_l w_s S gamma_t``, ``w_l w_s S gamma_x`` and ``w_l w_s S^2`` over the pairs with
    ``S = D_A(z_l) (1 - chi_l / chi_s) > 0`` in Mpc (``yawhip_dsigma_count``; ``dsigma_columns`` makes the three columns).
    Both layouts carry redshifts (``build_trees(..., with_redshifts=True)``), the sources ``g1`` / ``g2`` besides and no
    bins. Each reaches the device once per context as a handle kept on the layout (``_lib.DsigmaLenses``, ``_lib.ShearSources``
    with ``u``), replaced when another sort axis or another cosmology is asked for. On a context of several devices the count
    runs on its first one. No CPU fallback; the CPU tests replace this function."""
    return _count_dsigma(lens_layout, source_layout, jobs, thresholds, cosmology, sort_axis)


S2_CAP = 0.01  # the largest squared chord yawhip_dsigma_count_radial accepts as the reach of a lens (5.73 degrees)


def radial_kind(unit) -> str:
    """"physical" (kpc, Mpc: ``R = D_A(z_l) theta``) or "comoving" (kpc/h, Mpc/h: ``R = D_A(z_l) (1 + z_l) theta``, the
    conversion of ``Scales.get_angle_radian``); an angular unit has no radius: ``ValueError``."""
    from .options import COMOVING_UNITS, PHYSICAL_UNITS, Unit

    unit = Unit.parse(unit)
    if unit in PHYSICAL_UNITS:
        return "physical"
    if unit in COMOVING_UNITS:
        return "comoving"
    raise ValueError(f"radius='lens' needs scales in a physical or comoving unit, not '{unit}'")


def dsigma_radial_columns(lens_layout, source_layout, cosmology, unit, *, unit_columns: bool = False):
    """The four columns ``yawhip_dsigma_count_radial`` reads: ``(f, c, m, u)`` = ``dsigma_columns`` with the lenses' squared
    transverse distance per radian ``m`` in Mpc^2 besides: ``f * f`` for the physical units, ``(f * (1 + z_l))**2`` for the
    comoving ones (``radial_kind``). Every lens needs ``m > 0``, a redshift ``> 0`` (``ValueError`` otherwise).
    ``unit_columns`` replaces ``f, c, u`` by ``1, 0, 0`` -- the tangential shear itself, for which the sources need no
    redshifts. A side given as ``None`` is skipped."""
    kind = radial_kind(unit)
    f, c, u = dsigma_columns(lens_layout, None if unit_columns else source_layout, cosmology)
    m = None
    if lens_layout is not None:
        reach = f if kind == "physical" else f * (1.0 + lens_layout.redshifts)
        m = reach * reach
        if not (np.all(np.isfinite(m)) and np.all(m > 0.0)):
            raise ValueError("a lens needs a finite transverse distance > 0 (a redshift > 0) to have a radius")
        if unit_columns:
            f, c = np.ones_like(f), np.zeros_like(c)
    if unit_columns and source_layout is not None:
        u = np.zeros(len(source_layout.x), dtype=np.float64)
    return f, c, m, u


def radial_reach(lens_layout, m, r2):
    """``smax`` f64[B] of the library's contract: the largest squared chord of a pair in range per redshift bin, from the
    nearest lens of the bin over all patches (a bin without lenses: 0), and that lens's index per bin (-1: none)."""
    r2 = np.asarray(r2, dtype=np.float64)
    num_bins = len(r2)
    smax, nearest = np.zeros(num_bins), np.full(num_bins, -1, dtype=np.int64)
    offsets, nb = lens_layout.offsets, lens_layout.num_bins
    for k in range(num_bins):
        bins = [0] if nb == 1 else [k]
        idx = np.concatenate([np.arange(offsets[p * nb + b], offsets[p * nb + b + 1]) for p in range(lens_layout.num_patches) for b in bins])
        if len(idx):
            nearest[k] = idx[np.argmin(m[idx])]
            smax[k] = r2[k, -1] / m[nearest[k]] * (1.0 + 1e-12)
    return smax, nearest


def check_radial_reach(lens_layout, m, r2):
    """Turn the library's cap (a reach beyond a squared chord of 0.01) into a ``ValueError`` that names the nearest lens and
    the largest radius; returns ``smax`` of ``radial_reach``."""
    smax, nearest = radial_reach(lens_layout, m, r2)
    for k in np.flatnonzero(smax > S2_CAP):
        z = lens_layout.redshifts[nearest[k]] if getattr(lens_layout, "redshifts", None) is not None else float("nan")
        raise ValueError(f"a lens is too close for the largest radius: the nearest lens of redshift bin {k} at z = {z:.6g} sees "
                         f"R = {np.sqrt(np.asarray(r2)[k, -1]):.6g} Mpc under {np.degrees(2.0 * np.arcsin(0.5 * np.sqrt(smax[k]))):.3g} "
                         f"degrees; a per-lens count reaches 5.73 degrees at most")
    return smax


def count_dsigma_radial_fine(lens_layout, source_layout, jobs, r2, *, cosmology, unit, sort_axis: int = 2, unit_columns: bool = False):
    """``count_dsigma_fine`` with the pairs binned in each lens's own radius: ``r2`` f64[B, E] are squared radius edges in
    Mpc^2 and a pair falls into the fine bin that holds ``R^2 = m_l theta^2`` (``yawhip_dsigma_count_radial``;
    ``dsigma_radial_columns`` makes the columns from the redshifts, ``unit`` says whether the radii are physical or
    comoving). ``unit_columns``: the sums of ``count_shear_fine`` in that binning (the sources need no redshifts). The lens
    handle is kept on the layout per context, sort axis, cosmology, kind of unit and ``unit_columns``; the sources' is that of
    ``count_dsigma_fine``. A reach beyond the library's cap is a ``ValueError`` (``check_radial_reach``). No CPU fallback;
    the CPU tests replace this function."""
    return _count_dsigma(lens_layout, source_layout, jobs, r2, cosmology, sort_axis, unit, unit_columns)


def _count_dsigma(lens_layout, source_layout, jobs, table, cosmology, sort_axis, unit=None, unit_columns=False):
    """The body of ``count_dsigma_fine`` (``unit`` None: ``table`` holds thresholds) and of ``count_dsigma_radial_fine`` (``table``
    holds squared radii in ``unit``): the checks of the sources, the two resident handles, the count."""
    _require_shear(source_layout)
    if source_layout.num_bins != 1:
        raise ValueError("the sources of an excess-surface-density count are not binned in redshift")
    ctx = get_context()

    def columns(lens_side, source_side):  # (f, c, m, u)
        if unit is not None:
            return dsigma_radial_columns(lens_side, source_side, cosmology, unit, unit_columns=unit_columns)
        f, c, u = dsigma_columns(lens_side, source_side, cosmology)
        return f, c, None, u

    def lenses():
        f, c, m, _ = columns(lens_layout, None)
        return _lib.DsigmaLenses(ctx, lens_layout.x, lens_layout.y, lens_layout.z, lens_layout.w, f, c, lens_layout.num_patches,
                                 lens_layout.num_bins, lens_layout.offsets, sort_axis=sort_axis, m=m)

    def sources():
        u = columns(None, source_layout)[3]
        return _lib.ShearSources(ctx, source_layout.x, source_layout.y, source_layout.z, source_layout.w, source_layout.g1,
                                 source_layout.g2, source_layout.num_patches, source_layout.offsets, sort_axis=sort_axis, u=u)

    suffix = " unit" if unit_columns else ""
    lens_role = "lenses" if unit is None else f"lenses radial {radial_kind(unit)}{suffix}"
    lens_handle = _handle(lens_layout, ctx, sort_axis, lens_role, lenses, cosmology)
    source_handle = _handle(source_layout, ctx, sort_axis, "sources" + suffix, sources, cosmology)
    if unit is None:
        return _lib.dsigma_count(ctx, lens_handle, source_handle, jobs, table)
    try:
        return _lib.dsigma_count_radial(ctx, lens_handle, source_handle, jobs, table)
    except _lib.YawhipError as err:
        if "too close for the largest radius" not in str(err):
            raise
        check_radial_reach(lens_layout, columns(lens_layout, None)[2], table)  # the same refusal, with the lens's redshift and the radius
        raise


def proj_columns(layout, cosmology, unit):
    """The two columns ``yawhip_proj_count`` reads (include/yawhip.h), from the layout's redshifts
    (``build_trees(edges, with_redshifts=True)``) and ``cosmology`` (assumed flat), each in the layout's order: ``(d, c)`` =
    the transverse distance per radian in Mpc -- ``D_A(z)`` for ``kpc`` / ``Mpc``, ``D_A(z) (1 + z)`` for ``kpc/h`` /
    ``Mpc/h`` (``radial_kind``, the conversions of ``dsigma_radial_columns``) -- and the comoving distance ``chi(z)`` in Mpc.
    ``Scales`` reads a ``/h`` unit as a comoving length in the cosmology's own Mpc (it applies no factor ``h``), and so do
    the radii of ``radial_plans``; ``c`` and ``pi_max`` are lengths of that kind too, for all four units. Redshifts must be
    finite and ``> 0`` and the distances finite (``ValueError`` otherwise)."""
    from .cosmology import distance_column

    kind = radial_kind(unit)
    z = check_proj_redshifts(layout)
    d, c = distance_column(cosmology, z, kind="angular"), distance_column(cosmology, z, kind="comoving")
    if kind == "comoving":
        d = d * (1.0 + z)
    if not (np.all(np.isfinite(d)) and np.all(d > 0.0) and np.all(np.isfinite(c))):
        raise ValueError("the cosmology gives distances that are not finite numbers > 0")
    return d, c


def check_proj_redshifts(layout):
    """The redshifts of a layout for a projected count: present, finite and ``> 0`` (``ValueError`` otherwise)."""
    z = layout.redshifts
    if z is None:
        raise ValueError("the catalogue carries no redshifts: build_trees(..., with_redshifts=True)")
    if not (np.all(np.isfinite(z)) and np.all(z > 0.0)):
        raise ValueError("the redshifts of a projected count must be finite and > 0")
    return z


def check_pi_max(pi_max) -> float:
    """``pi_max`` of a projected count as a float: a length ``> 0`` and finite (``ValueError`` otherwise)."""
    pi_max = float(pi_max)
    if not (np.isfinite(pi_max) and pi_max > 0.0):
        raise ValueError(f"pi_max must be a finite length > 0, not {pi_max}")
    return pi_max


def check_pi_edges(pi_bins, pi_max) -> np.ndarray:
    """The line-of-sight bin edges f64[n_pi + 1] of a pi-binned projected count from ``pi_bins``: an int ``n >= 1`` gives
    ``np.linspace(0.0, pi_max, n + 1)``; a sequence of edges must start at 0, ascend strictly, be finite and end at ``pi_max``
    (``ValueError`` otherwise)."""
    pi_max = check_pi_max(pi_max)
    if isinstance(pi_bins, (bool, np.bool_)):
        raise ValueError("pi_bins must be a number of bins >= 1 or a sequence of edges")
    if isinstance(pi_bins, (int, np.integer)):
        if pi_bins < 1:
            raise ValueError(f"pi_bins must be >= 1, not {pi_bins}")
        return np.linspace(0.0, pi_max, int(pi_bins) + 1)
    try:
        edges = np.array(pi_bins, dtype=np.float64)
    except (TypeError, ValueError) as err:
        raise ValueError("pi_bins must be a number of bins >= 1 or a sequence of edges") from err
    if edges.ndim != 1 or len(edges) < 2:
        raise ValueError("pi_bins as edges must be a sequence of at least two numbers")
    if not np.all(np.isfinite(edges)):
        raise ValueError("the pi edges must be finite")
    if edges[0] != 0.0:
        raise ValueError(f"the pi edges must start at 0, not {edges[0]}")
    if not np.all(np.diff(edges) > 0.0):
        raise ValueError("the pi edges must ascend strictly")
    if edges[-1] != pi_max:
        raise ValueError(f"the pi edges must end at pi_max = {pi_max}, not {edges[-1]}")
    return edges


def _proj_handles(layout_a, layout_b, cosmology, unit, sort_axis):
    """The context and the two resident ``_lib.ProjHandle`` of a projected count (role "projected <kind of unit>"): the same
    layout twice is ONE handle passed twice."""
    ctx = get_context()
    role = f"projected {radial_kind(unit)}"

    def handle(layout):
        def upload():
            d, c = proj_columns(layout, cosmology, unit)
            return _lib.ProjHandle(ctx, layout.x, layout.y, layout.z, layout.w, d, c, layout.num_patches, layout.num_bins,
                                   layout.offsets, sort_axis=sort_axis)

        return _handle(layout, ctx, sort_axis, role, upload, cosmology)

    a = handle(layout_a)
    return ctx, a, a if layout_b is layout_a else handle(layout_b)


def _run_projected(count, layouts, cosmology, unit, table, cap=None):
    """``count()``, a ``_lib`` call over projected cells with the edge table ``table`` of ``layouts``, with the library's two
    refusals as ``ValueError``: more bins of a second binning than a workgroup's LDS holds -- ``cap = (n, bins, rows, planes)``,
    the words of the message -- and a reach beyond the library's cap (``check_projected_reach``, with the redshift and the
    radius). Anything else is raised as it came."""
    try:
        return count()
    except _lib.YawhipError as err:
        if cap is not None and "do not fit the LDS" in str(err):
            n, bins, rows, planes = cap
            most = re.search(rf"at most (\d+) {bins} bins", str(err)).group(1)
            raise ValueError(f"{n} {bins} bins are too many for {np.shape(table)[1]} {rows} edges (the fine bins of the "
                             f"configuration's resolution){planes}: at most {most} {bins} bins fit; use fewer {bins} bins or a lower "
                             "resolution") from err
        if "too close for the largest radius" not in str(err):
            raise
        check_projected_reach(layouts, cosmology, unit, table)  # the same refusal, with the redshift and the radius
        raise


def count_projected_pi_fine(layout_a, layout_b, cells, r2, *, pi_edges, cosmology, unit, sort_axis: int = 2):
    """``count_projected_fine`` with the pairs binned in ``|chi_a - chi_b|`` by ``pi_edges`` f64[n_pi + 1]
    (``check_pi_edges``; bin 0 is ``[0, pe[1]]``, bin j ``(pe[j], pe[j + 1]]``) -> ``(W, CountStats)``, W f64[n_pi, n_cells,
    E-1] (``yawhip_proj_count_pi``). Handles, their role and the reach translation are ``count_projected_fine``'s. More pi
    bins than a workgroup's LDS holds at this number of radius edges is a ``ValueError`` that states the cap; the library
    does not split a call and neither does this. No CPU fallback; the CPU tests replace this function."""
    ctx, a, b = _proj_handles(layout_a, layout_b, cosmology, unit, sort_axis)
    return _run_projected(lambda: _lib.proj_count_pi(ctx, a, b, cells, r2, pi_edges), (layout_a, layout_b), cosmology, unit, r2,
                          cap=(len(pi_edges) - 1, "pi", "radius", ""))


def count_projected_shear_fine(dens_layout, shape_layout, cells, r2, *, pi_edges, cosmology, unit, sort_axis: int = 2):
    """Fine-bin projected position-shape sums for ``cells`` (int[n, 4] = ``(segment of dens_layout, segment of shape_layout,
    row of r2, 0)``) -> ``((T, X, W), CountStats)``, each plane f64[n_pi, n_cells, E-1]: over the pairs that
    ``count_projected_pi_fine`` puts into a radius and pi bin, the sums of ``w_d w_s e_t``, ``w_d w_s e_x`` and ``w_d w_s``
    with ``e_t``, ``e_x`` the shape's ellipticity rotated to the great circle through the pair -- ``e_t`` is negative where
    the shape points at the density object (``yawhip_proj_count_shear``). ``shape_layout`` carries shear and redshifts
    (``build_trees(edges, with_shear=True, with_redshifts=True)``); the columns of both come from ``proj_columns``. The
    density side is the resident handle of role "projected <kind>", the one ``count_projected_fine`` uses: a layout counted
    for ``w_p`` is not uploaded again. The shapes get a handle of their own (role "projected shapes <kind>"), also when
    the layout is the density layout. Cap and reach refusals become ``ValueError`` as in ``count_projected_pi_fine``. No CPU
    fallback; the CPU tests replace this function."""
    _require_shear(shape_layout)
    ctx, dens, _ = _proj_handles(dens_layout, dens_layout, cosmology, unit, sort_axis)
    shapes = _proj_shape_handle(shape_layout, ctx, cosmology, unit, sort_axis)
    return _run_projected(lambda: _lib.proj_count_shear(ctx, dens, shapes, cells, r2, pi_edges), (dens_layout, shape_layout), cosmology,
                          unit, r2, cap=(len(pi_edges) - 1, "pi", "radius", " with three planes each"))


def _proj_shape_handle(layout, ctx, cosmology, unit, sort_axis):
    """The resident ``_lib.ProjShapesHandle`` of a layout with shear and redshifts (role "projected shapes <kind of unit>"):
    what ``count_projected_shear_fine`` keeps in its lanes and ``count_projected_shapes_fine`` on either side."""

    def upload():
        d, c = proj_columns(layout, cosmology, unit)
        return _lib.ProjShapesHandle(ctx, layout.x, layout.y, layout.z, layout.w, layout.g1, layout.g2, d, c, layout.num_patches,
                                     layout.num_bins, layout.offsets, sort_axis=sort_axis)

    return _handle(layout, ctx, sort_axis, f"projected shapes {radial_kind(unit)}", upload, cosmology)


def max_shape_pi_bins(n_edges: int) -> int:
    """The largest number of pi bins of a shape-shape count at ``n_edges`` radius edges: the formula of include/yawhip.h for
    ``yawhip_proj_count_shapes`` -- two stages of 64-byte objects, the edges, four planes per pi bin and wave -- within 64 KiB
    of LDS. 0: not even one pi bin fits (above 241 edges)."""
    n_pi = 0
    while 32768 + 8 * (((n_edges + 1) & ~1) + ((n_pi + 3) & ~1)) + 128 * (n_pi + 1) * (n_edges - 1) <= 65536:
        n_pi += 1
    return n_pi


def count_projected_shapes_fine(layout_a, layout_b, cells, r2, *, pi_edges, cosmology, unit, sort_axis: int = 2):
    """Fine-bin projected shape-shape sums for ``cells`` (int[n, 4] = ``(segment of layout_a, segment of layout_b, row of r2,
    diagonal)``, ``count_projected_fine``'s) -> ``((PP, XX, PX, W), CountStats)``, each plane f64[n_pi, n_cells, E-1]: over the
    pairs that ``count_projected_pi_fine`` puts into a radius and pi bin, the sums of ``w_a w_b et_a et_b``,
    ``w_a w_b ex_a ex_b``, ``w_a w_b (et_a ex_b + ex_a et_b)`` and ``w_a w_b``, with ``et``, ``ex`` the ellipticity of either
    shape rotated to the great circle through the pair (``yawhip_proj_count_shapes``). ``et`` is the tangential ellipticity
    of ``count_projected_shear_fine``, ``e+ = -et``: the two signs cancel in PP, and PX is minus the ``+x`` product. Both layouts carry shear and redshifts (``build_trees(edges, with_shear=True, with_redshifts=True)``)
    and are the resident shape handles of ``count_projected_shear_fine`` (role "projected shapes <kind>"): a catalogue
    uploaded for ``w_g+`` is not uploaded again, and the same layout twice is ONE handle passed twice -- only then a cell
    may be diagonal. More pi bins than ``max_shape_pi_bins`` gives at this number of radius edges is a ``ValueError`` that
    states the cap, raised before anything reaches the device; the reach refusal becomes one as in
    ``count_projected_pi_fine``. No CPU fallback; the CPU tests replace this function."""
    _require_shear(layout_a, layout_b)
    check_shape_pi_cap(len(pi_edges) - 1, np.shape(r2)[1])
    ctx = get_context()
    a = _proj_shape_handle(layout_a, ctx, cosmology, unit, sort_axis)
    b = a if layout_b is layout_a else _proj_shape_handle(layout_b, ctx, cosmology, unit, sort_axis)
    return _run_projected(lambda: _lib.proj_count_shapes(ctx, a, b, cells, r2, pi_edges), (layout_a, layout_b), cosmology, unit, r2)


def check_shape_pi_cap(n_pi: int, n_edges: int) -> None:
    """The cap of ``count_projected_shapes_fine`` as a ``ValueError`` that states it."""
    cap = max_shape_pi_bins(n_edges)
    if n_pi > cap:
        fits = f"at most {cap} pi bins fit" if cap else "not even one pi bin fits above 241 radius edges"
        raise ValueError(f"{n_pi} pi bins are too many for {n_edges} radius edges (the fine bins of the configuration's resolution) "
                         f"with four planes each: {fits}; use fewer pi bins or a lower resolution")


def check_mu_edges(mu_bins) -> np.ndarray:
    """The edges f64[n_mu + 1] of the bins in ``mu = pi / s`` of a redshift-space count from ``mu_bins``: an int ``n >= 1``
    gives ``np.linspace(0.0, 1.0, n + 1)``; a sequence of edges must start at 0, ascend strictly, be finite and end at 1
    (``ValueError`` otherwise)."""
    if isinstance(mu_bins, (bool, np.bool_)):
        raise ValueError("mu_bins must be a number of bins >= 1 or a sequence of edges")
    if isinstance(mu_bins, (int, np.integer)):
        if mu_bins < 1:
            raise ValueError(f"mu_bins must be >= 1, not {mu_bins}")
        return np.linspace(0.0, 1.0, int(mu_bins) + 1)
    try:
        edges = np.array(mu_bins, dtype=np.float64)
    except (TypeError, ValueError) as err:
        raise ValueError("mu_bins must be a number of bins >= 1 or a sequence of edges") from err
    if edges.ndim != 1 or len(edges) < 2:
        raise ValueError("mu_bins as edges must be a sequence of at least two numbers")
    if not np.all(np.isfinite(edges)):
        raise ValueError("the mu edges must be finite")
    if edges[0] != 0.0:
        raise ValueError(f"the mu edges must start at 0, not {edges[0]}")
    if not np.all(np.diff(edges) > 0.0):
        raise ValueError("the mu edges must ascend strictly")
    if edges[-1] != 1.0:
        raise ValueError(f"the mu edges must end at 1, not {edges[-1]}")
    return edges


def count_smu_fine(layout_a, layout_b, cells, s2, *, mu_edges, cosmology, unit, sort_axis: int = 2):
    """Fine-bin redshift-space pair counts for ``cells`` (``count_projected_fine``'s) -> ``(W, CountStats)``, W f64[n_mu,
    n_cells, E-1]: the sums of ``w_a w_b`` over the pairs whose ``S^2 = R^2 + (chi_a - chi_b)^2`` lies in the fine bin of the
    row of ``s2`` f64[n_rows, E] (squared s edges in Mpc^2) and whose ``mu = |chi_a - chi_b| / S`` lies in the mu bin of
    ``mu_edges`` f64[n_mu + 1] (``check_mu_edges``; bin 0 is ``[0, mu_1]``, bin j ``(mu_j, mu_{j+1}]``), with no line-of-sight
    cut (``yawhip_proj_count_smu``). The library receives the squares ``mu_edges * mu_edges`` as float64 products and refuses
    them if they no longer ascend strictly. Handles, their role and the reach translation are ``count_projected_fine``'s:
    a layout that was counted in ``r_p`` is not uploaded again. More mu bins than a workgroup's LDS holds at this number of
    s edges is a ``ValueError`` that states the cap; the library does not split a call and neither does this. No CPU
    fallback; the CPU tests replace this function."""
    ctx, a, b = _proj_handles(layout_a, layout_b, cosmology, unit, sort_axis)
    mu_edges = np.asarray(mu_edges, dtype=np.float64)
    return _run_projected(lambda: _lib.proj_count_smu(ctx, a, b, cells, s2, mu_edges * mu_edges), (layout_a, layout_b), cosmology, unit, s2,
                          cap=(len(mu_edges) - 1, "mu", "s", ""))


def _check_signed_edges(bins, name: str, top: float, top_name: str) -> np.ndarray:
    """What the two signed edge checks share: ``bins`` as an int ``n >= 1`` gives ``np.linspace(-top, top, n + 1)``, each edge
    averaged with minus its mirror -- at most an ulp from ``linspace``, and exactly antisymmetric with an exact 0 in the middle
    of an even number of bins, which is what folding the result asks for; a sequence must run from ``-top`` to ``top``, finite
    and strictly ascending, symmetric inside or not (``ValueError`` otherwise)."""
    if isinstance(bins, (bool, np.bool_)):
        raise ValueError(f"{name}_bins must be a number of bins >= 1 or a sequence of edges")
    if isinstance(bins, (int, np.integer)):
        if bins < 1:
            raise ValueError(f"{name}_bins must be >= 1, not {bins}")
        edges = np.linspace(-top, top, int(bins) + 1)
        return 0.5 * (edges - edges[::-1])
    try:
        edges = np.array(bins, dtype=np.float64)
    except (TypeError, ValueError) as err:
        raise ValueError(f"{name}_bins must be a number of bins >= 1 or a sequence of edges") from err
    if edges.ndim != 1 or len(edges) < 2:
        raise ValueError(f"{name}_bins as edges must be a sequence of at least two numbers")
    if not np.all(np.isfinite(edges)):
        raise ValueError(f"the signed {name} edges must be finite")
    if edges[0] != -top:
        raise ValueError(f"the signed {name} edges must start at -{top_name} = {-top}, not {edges[0]}")
    if not np.all(np.diff(edges) > 0.0):
        raise ValueError(f"the signed {name} edges must ascend strictly")
    if edges[-1] != top:
        raise ValueError(f"the signed {name} edges must end at {top_name} = {top}, not {edges[-1]}")
    return edges


def check_signed_pi_edges(pi_bins, pi_max) -> np.ndarray:
    """The edges f64[n + 1] of a SIGNED line-of-sight binning from ``pi_bins``: an int ``n >= 1`` gives
    ``np.linspace(-pi_max, pi_max, n + 1)`` (made exactly antisymmetric: ``_check_signed_edges``); a sequence of edges must run from ``-pi_max`` to ``pi_max``, finite and strictly
    ascending -- it need not be symmetric inside (``ValueError`` otherwise)."""
    return _check_signed_edges(pi_bins, "pi", check_pi_max(pi_max), "pi_max")


def check_signed_mu_edges(mu_bins) -> np.ndarray:
    """The edges f64[n + 1] of a SIGNED binning in ``mu = pi / s`` from ``mu_bins``: ``check_signed_pi_edges`` from -1 to 1."""
    return _check_signed_edges(mu_bins, "mu", 1.0, "1")


def count_projected_pi_signed_fine(layout_a, layout_b, cells, r2, *, pi_edges, cosmology, unit, sort_axis: int = 2):
    """``count_projected_pi_fine`` between two different layouts with the pairs binned in the SIGNED
    ``chi_b - chi_a`` -- object of ``layout_b`` minus object of ``layout_a`` -- by ``pi_edges`` f64[n + 1], finite and strictly
    ascending, of any sign (bin 0 is ``[pe[0], pe[1]]``, bin j ``(pe[j], pe[j + 1]]``) -> ``(W, CountStats)``, W f64[n, n_cells,
    E-1] (``yawhip_proj_count_pi_signed``). No cell is diagonal. The handles are the resident ones of role "projected <kind>":
    a layout counted for the unsigned ``w_p`` is not uploaded again. Cap and reach refusals become ``ValueError`` as in
    ``count_projected_pi_fine``. No CPU fallback; the CPU tests replace this function."""
    ctx, a, b = _proj_handles(layout_a, layout_b, cosmology, unit, sort_axis)
    return _run_projected(lambda: _lib.proj_count_pi_signed(ctx, a, b, cells, r2, pi_edges), (layout_a, layout_b), cosmology, unit, r2,
                          cap=(len(pi_edges) - 1, "pi", "radius", ""))


def count_smu_signed_fine(layout_a, layout_b, cells, s2, *, mu_edges, cosmology, unit, sort_axis: int = 2):
    """``count_smu_fine`` between two different layouts with ``mu`` signed by ``chi_b - chi_a`` -- object of ``layout_b`` minus
    object of ``layout_a`` -- over ``mu_edges`` f64[n + 1] from -1 to 1 (``check_signed_mu_edges``; bin 0 is ``[-1, mu_1]``, bin
    j ``(mu_j, mu_{j+1}]``) -> ``(W, CountStats)``, W f64[n, n_cells, E-1] (``yawhip_proj_count_smu_signed``). The library
    receives the signed squares ``copysign(mu mu, mu)`` and refuses them if they no longer ascend strictly. No cell is
    diagonal. Handles, cap and reach refusals: as ``count_smu_fine``. No CPU fallback; the CPU tests replace this function."""
    ctx, a, b = _proj_handles(layout_a, layout_b, cosmology, unit, sort_axis)
    mu_edges = np.asarray(mu_edges, dtype=np.float64)
    return _run_projected(lambda: _lib.proj_count_smu_signed(ctx, a, b, cells, s2, np.copysign(mu_edges * mu_edges, mu_edges)),
                          (layout_a, layout_b), cosmology, unit, s2, cap=(len(mu_edges) - 1, "mu", "s", ""))


def count_projected_fine(layout_a, layout_b, cells, r2, *, pi_max, cosmology, unit, sort_axis: int = 2):
    """Fine-bin projected pair counts for ``cells`` (int[n, 4] = ``(segment of layout_a, segment of layout_b, row of r2,
    diagonal)``, a segment ``patch * num_bins + bin``; ``diagonal`` non-zero iff the cell pairs a segment with itself, which
    takes ``layout_b is layout_a``) -> ``(W, CountStats)``, W f64[n_cells, E-1]: the sums of ``w_a w_b`` over the pairs
    with ``|chi_a - chi_b| <= pi_max`` in the fine bin that holds ``R^2 = (0.5 (d_a + d_b))^2 theta^2``, a diagonal cell
    holding every unordered pair once (``yawhip_proj_count``; ``proj_columns`` makes the columns, ``r2`` f64[n_rows, E] are
    squared radius edges in Mpc^2). Both are layouts with redshifts; each reaches the device once as a ``_lib.ProjHandle``
    kept on the layout per context, sort axis, cosmology and kind of unit; the same layout twice is ONE handle passed
    twice. A reach beyond the library's cap is ``check_radial_reach``'s ``ValueError`` with the object's redshift. No CPU
    fallback; the CPU tests replace this function."""
    ctx, a, b = _proj_handles(layout_a, layout_b, cosmology, unit, sort_axis)
    return _run_projected(lambda: _lib.proj_count(ctx, a, b, cells, r2, pi_max), (layout_a, layout_b), cosmology, unit, r2)


def check_projected_reach(layouts, cosmology, unit, r2):
    """``check_radial_reach`` for the layouts of a projected count whose cells pair bin ``k`` with bin ``k`` and row ``k``: the
    pair's ``D = (d_a + d_b) / 2`` is no less than the nearest object's ``d``, so ``m = d^2`` of either side bounds the
    reach. Returns the largest ``smax`` per bin over the layouts."""
    smax = np.zeros(len(r2))
    for layout in layouts:
        d = proj_columns(layout, cosmology, unit)[0]
        smax = np.maximum(smax, check_radial_reach(layout, d * d, r2))
    return smax


def _handle(layout, ctx, sort_axis, role, upload, cosmology=None):
    """The resident handle of ``layout`` in ``role`` on ``ctx`` (``layout.handles``), made by ``upload()`` on first use and
    anew where the one held has another sort axis, was freed, or was made with another ``cosmology`` than the one asked for
    (None, the same for every call of a role whose columns need none, equals only None)."""
    from .cosmology import cosmology_is_equal

    held = layout.handles.get((id(ctx), role))
    if held is not None and (held[0].sort_axis != sort_axis or not held[0]._h or not cosmology_is_equal(held[1], cosmology)):
        held[0].free()
        held = None
    if held is None:
        held = layout.handles[(id(ctx), role)] = (upload(), cosmology)
    return held[0]


def _shear_handle(layout, ctx, sort_axis):
    """The role "shear": the ``_lib.ShearSources`` of a layout with shear columns, binned as the layout is."""
    return _handle(layout, ctx, sort_axis, "shear", lambda: _lib.ShearSources(
        ctx, layout.x, layout.y, layout.z, layout.w, layout.g1, layout.g2, layout.num_patches, layout.offsets, sort_axis=sort_axis,
        n_bins=layout.num_bins))


def _device_pair(layout1, layout2, thresholds, sort_axis, max_workers=None):
    ctx = get_context(max_workers=max_workers)
    micro = forced_strip_micro if forced_strip_micro is not None else strip_micro_for(thresholds)
    d1 = device_catalog(layout1, ctx, sort_axis, micro, exact=forced_strip_micro is not None)
    d2 = d1 if layout2 is layout1 else device_catalog(layout2, ctx, sort_axis, d1.strip_micro, exact=True)
    return ctx, d1, d2


def scalar_segment_sums(layout, *, sort_axis: int | None = None):
    """``(sum kappa * w, sum w)`` per (patch, bin) segment of a layout with a scalar field, float64[P, B_or_1] each, summed
    on the device from its two resident catalogues (``yawhip_catalog_segment_sums``; uploaded first if they are not). There
    is no host fallback."""
    if layout.kappa is None:
        raise ValueError("catalog has no 'kappa' attached")
    ctx = get_context()
    have = layout.device.get(id(ctx))
    axis = sort_axis if sort_axis is not None else (have.sort_axis if have is not None else 2)
    dev_n = device_catalog(layout, ctx, axis)
    dev_k = device_catalog(layout.twin, ctx, axis)
    return dev_k.segment_sums(), dev_n.segment_sums()


def job_work(layout1, layout2, jobs, thresholds, *, kernel: str | None = None, sort_axis: int = 2) -> np.ndarray:
    """Pair distances the device will evaluate for every job (int64[n_jobs]; ``yawhip_job_work``): the
    cost ``PatchLinkage.count_pairs`` balances when it shards the job list over GPUs. It is an exact
    function of the inputs, so every rank derives the same partition."""
    ctx, d1, d2 = _device_pair(layout1, layout2, thresholds, sort_axis)
    return _lib.job_work(ctx, d1, d2, jobs, thresholds, kernel=kernel or default_kernel)


def _preparation_context():
    """The context catalogue preparation runs on (patch assignment and creation, randoms, HEALPix maps), or ``None`` when
    there is no library or device: the caller then takes its host route. One device does it: no reason to span (and
    replicate on) every GPU."""
    try:
        if _lib.device_count() < 1:
            return None
        return get_context(default_devices()[0])
    except _lib.YawhipError:
        return None


def assign_patches(xyz, centers_xyz):
    """Nearest patch centre per object on the device (``yawhip_assign_patches``), or ``None`` when no
    GPU / library is available -- patch assignment is catalogue preparation, which the reference does on
    the host too, so unlike the pair counts it may fall back to scipy there."""
    ctx = _preparation_context()
    if ctx is None:
        return None
    if isinstance(xyz, tuple):  # three columns
        x, y, z = (np.ascontiguousarray(c, dtype=np.float64) for c in xyz)
    else:
        xyz = np.asarray(xyz, dtype=np.float64)
        x, y, z = (np.ascontiguousarray(xyz[:, a]) for a in range(3))
    ids = _lib.assign_patches(ctx, x, y, z, centers_xyz)
    return ids.astype(np.int64)


def kmeans_open(x, y, z, weights=None, wscale: float = 0.0):
    """The unit vectors (and weights) of a catalogue uploaded once for the full-catalogue k-means of ``patches.py``
    (``yawhip_kmeans_open``) -> ``_lib.KMeans``, or ``None`` when no GPU / library is available: patch creation is
    catalogue preparation, as ``assign_patches``, and ``patches.py`` then runs the same arithmetic with numpy. One device
    does it."""
    ctx = _preparation_context()
    if ctx is None:
        return None
    return _lib.KMeans(ctx, x, y, z, weights, wscale)


def _random_context(generator):
    """The context random catalogues are drawn on, or ``None`` when there is no library or device, or the generator has
    more than 2^32 attached values (numpy's 64-bit bounded-integer path)."""
    if generator.data_size > _lib.RANDOM_MAX_DATA:
        return None
    return _preparation_context()


def draw_box_randoms(generator, num: int, chunksize: int):
    """``num`` points of a ``BoxRandoms`` drawn on the device (``yawhip_random_box``) in calls of ``chunksize`` from the
    generator's current state, as ``Catalog.from_random`` calls it on the host. Returns ``((x, y, w, z), end_state)`` --
    float64 host columns, ``w`` / ``z`` None without attached values, and the bit-generator state the calls end in, which
    the generator is left in too -- or ``None`` when there is no library or device, or more than 2^32 attached values
    (numpy's 64-bit bounded-integer path). Drawing randoms is catalogue preparation: like ``assign_patches`` it may fall
    back to the host, the pair counts may not."""
    ctx = _random_context(generator)
    if ctx is None:
        return None
    x, y, w, z, _, end = _lib.random_box(
        ctx, num, chunksize, generator.rng.bit_generator.state, generator.x_min, generator.x_max - generator.x_min,
        generator.y_min, generator.y_max - generator.y_min, generator.data_size, generator.weights, generator.redshifts)
    generator.rng.bit_generator.state = end
    return (x, y, w, z), end


def draw_healpix_randoms(generator, num: int, chunksize: int):
    """``num`` points of a ``HealPixRandoms`` drawn on the device (``yawhip_random_healpix``): the contract of
    :func:`draw_box_randoms`, with ``x = ra`` and ``y = sin(dec)`` of order-29 pixel centres inside the generator's map."""
    ctx = _random_context(generator)
    if ctx is None:
        return None
    x, y, w, z, _, _, end = _lib.random_healpix(
        ctx, num, chunksize, generator.rng.bit_generator.state, generator.order, generator._ipix_unmasked, generator._cdf,
        generator.data_size, generator.weights, generator.redshifts)
    generator.rng.bit_generator.state = end
    return (x, y, w, z), end


def healpix_map(phi, z, weights, order: int, nested: bool, *, want_pixels: bool = False, want_map: bool = True, chunksize: int = 0):
    """HEALPix pixels and map of the points ``(phi, z)`` on the device (``yawhip_healpix_map``): ``(pix, map)``, each ``None``
    unless wanted (see ``_lib.healpix_map``), or ``None`` when no GPU / library is available -- like patch assignment this is
    catalogue preparation, and ``healpix.ang2pix`` / ``healpix.healpix_map`` then compute the same values with numpy."""
    ctx = _preparation_context()
    if ctx is None:
        return None
    return _lib.healpix_map(ctx, phi, z, weights, order, nested, want_pixels=want_pixels, want_map=want_map, chunksize=chunksize)


def healpix_pixels(values, weights, order: int, nested: bool, *, chunksize: int = 0):
    """The unmasked pixels of the scalar map ``values`` (and its weight map, or None) compacted on the device
    (``yawhip_healpix_pixels``): ``(ipix, phi, z, kappa, w)`` as ``healpix.map_pixels`` returns them, or ``None`` when no GPU /
    library is available -- catalogue preparation, as :func:`healpix_map`, and ``healpix.map_pixels`` then computes the same
    values with numpy. The number of selected pixels is counted here, on the host, and the outputs are sized by it; the
    library raises if it selects another number. ValueError when every pixel is masked."""
    from . import healpix

    ctx = _preparation_context()
    if ctx is None:
        return None
    capacity = healpix.count_selected(values, weights)
    if capacity == 0:
        raise ValueError("every pixel is masked")
    return _lib.healpix_pixels(ctx, values, weights, order, nested, capacity, chunksize=chunksize)[1:]


def redshift_histogram(z, w, offsets, edges, closed_right: bool) -> np.ndarray:
    """Per-patch redshift histogram on the device (``yawhip_redshift_histogram``): float64[P, B] object counts, or sums of
    weights with ``w``. One device does it, as for ``assign_patches``; unlike that there is no host fallback -- a
    missing library or GPU raises ``YawhipError``."""
    ctx = get_context(default_devices()[0])
    return _lib.redshift_histogram(ctx, z, w, offsets, edges, closed_right)
