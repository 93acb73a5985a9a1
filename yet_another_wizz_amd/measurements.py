"""Cross- and autocorrelation drivers on the MI355X pair-count engine.

Drop-in for the nn path of ``yaw.correlation.measurements`` (src/yaw/correlation/measurements.py):
``crosscorrelate`` (:529-628), ``autocorrelate`` (:455-525), ``PatchLinkage`` (:171-392) keep their
call shapes, error behaviour and result types.  What changes is the execution model: the
reference farms one Python task per patch pair to a process pool, each task unpickles KD-trees
and loops over redshift bins (:88-128, :344-364); here the whole job list of one pair count goes
to the GPU in a single ``yawhip_count_pairs`` call against catalogues resident in HBM, the jobs
are sharded over the processes of a ``torch.distributed`` group (one per GPU) and the dense
``[B, E-1, P, P]`` tensor is combined with one all-reduce.
"""
from __future__ import annotations

import functools
import logging
from itertools import compress

import numpy as np

from . import _lib, engine, parallel
from .angular_bins import plan_for_limits, radial_plan_for_limits
from .catalog import Catalog, InconsistentPatchesError
from .coordinates import AngularDistances
from .corrfunc import (AlignmentCorrFunc, CorrFunc, MultipoleCorrFunc, ProjectedCorrFunc, ScalarCorrFunc, ShapeShapeCorrFunc,
                       SignedMultipoleCorrFunc, SignedProjectedCorrFunc)
from .cosmology import DELTA_SIGMA_UNIT
from .options import CountMode
from .paircounts import NormalisedCounts, NormalisedScalarCounts, PatchedCounts, PatchedSumWeights

__all__ = ["autocorrelate", "autocorrelate_projected", "autocorrelate_multipoles", "crosscorrelate", "crosscorrelate_projected", "crosscorrelate_multipoles", "autocorrelate_scalar", "crosscorrelate_scalar", "crosscorrelate_scalar_map",
           "crosscorrelate_shear", "crosscorrelate_delta_sigma", "crosscorrelate_alignment", "autocorrelate_alignment", "autocorrelate_shear", "correlate_shear_tomographic", "compute_scalar_normalisation",
           "PatchLinkage", "get_max_angle", "radial_plans", "radial_max_angle", "check_patch_conistency"]

logger = logging.getLogger("yet_another_wizz_amd")


def _log_info(*args) -> None:
    if parallel.world()[0] == 0:
        logger.info(*args)


def check_patch_conistency(catalog: Catalog, *catalogs: Catalog, rtol: float = 0.5) -> None:
    """Patch centres of the other catalogues must lie within ``rtol`` patch radii of
    ``catalog``'s centres (measurements.py:131-149; the reference's spelling is kept)."""
    centers, radii = catalog.get_centers(), catalog.get_radii()
    for other in catalogs:
        offset = centers.distance(other.get_centers())
        if np.any(offset.data / radii.data > rtol):
            raise InconsistentPatchesError("patch centers are not aligned")


def get_max_angle(config, redshift_limit: float = 0.05) -> AngularDistances:
    """Largest separation any pair can contribute at: the upper scale limits evaluated at
    max(zmin, redshift_limit) (measurements.py:152-168)."""
    z = max(config.binning.zmin, redshift_limit)
    _, ang_max = config.scales.scales.get_angle_radian(z, cosmology=config.cosmology)
    return AngularDistances(np.max(ang_max))


def angular_plans(config):
    """One :class:`AngularBinPlan` per redshift bin: scale limits at the bin centre
    (measurements.py:99,110-112) -> edges -> thresholds."""
    scales, cosmology = config.scales.scales, config.cosmology
    return [
        plan_for_limits(*scales.get_angle_radian(zmid, cosmology=cosmology), config.scales.rweight,
                        config.scales.resolution)
        for zmid in config.binning.binning.mids
    ]


def radial_plans(config):
    """One :class:`RadialBinPlan` for every redshift bin (the same object): the scale limits as radii in Mpc (physical for
    ``kpc`` / ``Mpc``, comoving for ``kpc/h`` / ``Mpc/h``, as ``Scales.get_angle_radian`` reads them) -> edges -> squared
    radii. No redshift enters: a count with ``radius="lens"`` bins every pair by its lens's own distance. Angular units are a
    ``ValueError``."""
    from .options import Unit

    scales = config.scales.scales
    engine.radial_kind(scales.unit)
    per_mpc = 1000.0 if scales.unit in (Unit.kpc, Unit.kpc_h) else 1.0
    plan = radial_plan_for_limits(scales.scale_min / per_mpc, scales.scale_max / per_mpc, config.scales.rweight, config.scales.resolution)
    return [plan] * len(config.binning.binning)


def radial_max_angle(config, *lens_layouts) -> float:
    """The largest angle (radian) of a pair that a count with ``radius="lens"`` holds: that under which the nearest lens of
    any redshift bin of ``lens_layouts`` (layouts with redshifts: the lenses and, where given, the random lenses) sees the
    largest radius. A lens too close for the library's cap (5.73 degrees) is a ``ValueError`` that names its redshift and the
    radius."""
    r2 = threshold_table(radial_plans(config))
    smax = 0.0
    for layout in lens_layouts:
        m = engine.dsigma_radial_columns(layout, None, config.cosmology, config.scales.scales.unit, unit_columns=True)[2]
        smax = max(smax, float(np.max(engine.check_radial_reach(layout, m, r2))))
    return 2.0 * np.arcsin(0.5 * np.sqrt(smax))


class CombinePlan:
    """``AngularBinPlan.combine`` for all redshift bins of one configuration, prepared once: bins whose plans share
    the edge count, the per-scale slices and the separation weights (always the case for angular units) are handled
    in one vectorised pass over fine[B, E-1, J] -> [S, B, J]."""

    __slots__ = ("plans", "num_scales", "uniform", "num_fine", "slices", "scale_factors", "single")

    def __init__(self, plans):
        first = plans[0]
        self.plans = plans
        self.num_scales = first.num_scales
        self.uniform = all(
            p.num_edges == first.num_edges and p._slices == first._slices
            and (p._scale_factor is None) == (first._scale_factor is None)
            for p in plans
        )
        self.num_fine = first.num_edges - 1
        self.slices = list(first._slices)
        self.scale_factors = None
        if self.uniform and first._scale_factor is not None:
            self.scale_factors = np.stack([p._scale_factor for p in plans])[:, :, np.newaxis]
        # the common case: one scale made of the one fine bin the device counted
        self.single = self.uniform and self.scale_factors is None and self.slices == [(0, 1)] and self.num_fine == 1

    def dense_spec(self, num_fine: int):
        """The recombination as ``yawhip_count_pairs_dense`` takes it: ``slices`` int32[B, S, 2] (fine bins [first, last)
        of every scale and bin) and ``factors`` f64[B, num_fine] (separation weights, 0 for the padded fine bins of a bin
        with fewer edges) or None."""
        slices = np.ascontiguousarray([p._slices for p in self.plans], dtype=np.int32)
        factors = None
        if any(p._scale_factor is not None for p in self.plans):
            factors = np.zeros((len(self.plans), num_fine), dtype=np.float64)
            for k, p in enumerate(self.plans):
                factors[k, : p.num_edges - 1] = 1.0 if p._scale_factor is None else p._scale_factor
        return slices, factors

    def __call__(self, fine_bej) -> np.ndarray:
        if self.single:
            return fine_bej[:, 0][np.newaxis]  # a view: [1, B, J]
        num_bins, _, num_jobs = fine_bej.shape
        out = np.empty((self.num_scales, num_bins, num_jobs), dtype=np.float64)
        if self.uniform:
            block = fine_bej[:, : self.num_fine]
            if self.scale_factors is not None:
                block = block * self.scale_factors
            for s, (lo, hi) in enumerate(self.slices):
                out[s] = block[:, lo:hi].sum(axis=1)
            return out
        for k, plan in enumerate(self.plans):
            out[:, k] = plan.combine(fine_bej[k, : plan.num_edges - 1].T).T
        return out


def combine_all(plans, fine_bej) -> np.ndarray:
    """One-off form of :class:`CombinePlan` (``PatchLinkage`` keeps the prepared object)."""
    return CombinePlan(plans)(fine_bej)


def threshold_table(plans) -> np.ndarray:
    """f64[B, Emax]. Bins with fewer edges are padded by repeating their last threshold: the
    padded fine bins (t < s <= t) are empty by construction."""
    n_edges = max(p.num_edges for p in plans)
    table = np.empty((len(plans), n_edges), dtype=np.float64)
    for k, plan in enumerate(plans):
        table[k, : plan.num_edges] = plan.thresholds
        table[k, plan.num_edges :] = plan.thresholds[-1]
    return table


FORCE_DEVICE_REDUCE = False  # tests: take the device-resident reduce of the nccl route in any group

JOB_FIXED_COST = 2.0e5  # evaluated-pair equivalent of touching a job at all (launch share, empty windows)


def job_costs(layout1, layout2, jobs, thresholds, tile: int = 1024) -> np.ndarray:
    """Host-side estimate of the device work per job (no GPU involved). ``PatchLinkage.count_pairs``
    balances the exact figure from the device instead (``engine.job_work``); this one serves the CPU
    tests of the sharding logic and as a documented model of the culling.

    Brute force would cost N1*N2; the z-window culling of the device path only evaluates the part
    of patch 1 within (tile extent + 2 r_max) in z of each lane tile of patch 2, so a job costs about
    N2 * N1 * min(1, (zext2 * tile / N2 + 2 r_max) / zext1)."""
    n1 = layout1.segment_sizes()[jobs[:, 0]].sum(axis=1, dtype=np.float64)
    n2 = layout2.segment_sizes()[jobs[:, 1]].sum(axis=1, dtype=np.float64)
    r_max = float(np.sqrt(np.max(thresholds)))
    z1 = np.maximum(layout1.z_extent[jobs[:, 0]], 1e-12)
    z2 = layout2.z_extent[jobs[:, 1]]
    window = np.minimum(1.0, (z2 * np.minimum(1.0, tile / np.maximum(n2, 1.0)) + 2.0 * r_max) / z1)
    return n1 * n2 * window + 1e3 * (n1 + n2)  # + per-object cost of touching the patches at all


def best_sort_axis(center_xyz, num_records) -> int:
    """Coordinate axis (0 = x, 1 = y, 2 = z) most perpendicular to the footprint's mean direction:
    patches are widest along it, so the device's 1-d window culling removes the most pairs. A
    footprint without a preferred direction (full sky) keeps z."""
    mean = (center_xyz * num_records[:, np.newaxis]).sum(axis=0) / max(float(num_records.sum()), 1.0)
    if np.linalg.norm(mean) < 0.2:
        return 2
    return int(np.argmin(np.abs(mean)))


_PLAN_CACHE: list = []  # (config, plans, thresholds, combine) of the last few configurations (they are immutable)


def _plans_for(config):
    """Angular plans, threshold table and recombination plan of a configuration; every measurement with the
    same configuration object (each builds its own PatchLinkage) shares them."""
    for cfg, plans, thresholds, combine in _PLAN_CACHE:
        if cfg is config:
            return plans, thresholds, combine
    plans = angular_plans(config)
    thresholds = threshold_table(plans)
    combine = CombinePlan(plans)
    _PLAN_CACHE.append((config, plans, thresholds, combine))
    del _PLAN_CACHE[:-4]
    return plans, thresholds, combine


class PatchLinkage:
    """Which patch pairs can contain pairs of objects within the largest scale.

    Patches i, j are linked if their centres are closer than r_i + r_j + theta_max
    (measurements.py:193-237); every pair count of one measurement shares the linkage."""

    def __init__(self, config, patch_links: dict) -> None:
        self.config = config
        self.patch_links = patch_links
        self.last_stats = None
        self.sort_axis = 2  # coordinate the device sorts by for its window culling (set by from_catalogs)
        # derived once per linkage (the configuration is immutable): thresholds and job tables
        self._plans = None
        self._thresholds = None
        self._combine = None
        self._job_tables: dict = {}
        self._scatter: dict = {}
        self._partitions: dict = {}
        self.last_rank_info: dict | None = None
        self.last_batch_stats: dict = {}  # count_pairs_batch: CountStats of every count of the last submission, by its name
        self._dense_spec = None

    def _angular_setup(self):
        if self._plans is None:
            self._plans, self._thresholds, self._combine = _plans_for(self.config)
        return self._plans, self._thresholds

    @classmethod
    def from_catalogs(cls, config, catalog: Catalog, *catalogs: Catalog, max_angle: float | None = None):
        """``max_angle`` (radian): the largest separation of a pair that counts, where it is not that of the scales at
        ``max(zmin, 0.05)`` -- a count binned per lens reaches as far as its nearest lens sees its largest radius."""
        if any(set(cat.keys()) != set(catalog.keys()) for cat in catalogs):
            raise InconsistentPatchesError("patch IDs do not match")
        if max_angle is None:
            max_angle = get_max_angle(config).data[0]
        # the catalogue with the most records constrains centres / radii best (measurements.py:220-225)
        ranked = sorted([catalog, *catalogs], key=lambda cat: cat.get_num_records(), reverse=True)
        ref_cat, others = ranked[0], ranked[1:]
        check_patch_conistency(ref_cat, *others)
        patch_ids = list(ref_cat.keys())
        centers, radii = ref_cat.get_centers(), ref_cat.get_radii().data
        # all P x P centre separations at once, with the arithmetic of AngularCoordinates.distance
        # (squares summed over x, y, z, sqrt, 2 asin(r/2)), so the comparison decides exactly as the per-patch loop
        xyz = centers.to_3d()
        chord = np.sqrt(((xyz[:, np.newaxis, :] - xyz[np.newaxis, :, :]) ** 2).sum(axis=2))
        linked = 2.0 * np.arcsin(chord / 2.0) < (radii[np.newaxis, :] + radii[:, np.newaxis] + max_angle)
        links = {pid: set(compress(patch_ids, row)) for pid, row in zip(patch_ids, linked)}
        new = cls(config, links)
        new.sort_axis = best_sort_axis(centers.to_3d(), np.asarray(ref_cat.get_num_records(), dtype=np.float64))
        return new

    @property
    def num_total(self) -> int:
        return len(self.patch_links) ** 2

    @property
    def num_links(self) -> int:
        return sum(len(v) for v in self.patch_links.values())

    @property
    def density(self) -> float:
        return self.num_links / self.num_total

    def __repr__(self) -> str:
        return f"{type(self).__name__}(num_links={self.num_links}, density={self.density:.0%})"

    def iter_patch_id_pairs(self, *, auto: bool):
        """All linked (i, j): every ordered pair for a cross count, i <= j for an auto count
        (measurements.py:258-289). Same set as the reference; the order (diagonal jobs first, then
        by patch id) only matters for scheduling, which happens in ``partition_jobs``."""
        for i in sorted(self.patch_links):
            if i in self.patch_links[i]:
                yield (i, i)
        for i in sorted(self.patch_links):
            for j in sorted(self.patch_links[i]):
                if j != i and (not auto or j > i):
                    yield (i, j)

    def get_patch_pairs(self, catalog1: Catalog, catalog2: Catalog | None = None) -> np.ndarray:
        """int32[n_jobs, 2] job table (stands in for the tuple of ``PatchPair`` objects,
        measurements.py:291-305)."""
        auto = catalog2 is None
        if auto not in self._job_tables:
            pairs = list(self.iter_patch_id_pairs(auto=auto))
            table = np.array(pairs, dtype=np.int32).reshape(-1, 2)
            table.setflags(write=False)
            self._job_tables[auto] = table
        return self._job_tables[auto]

    # ------------------------------------------------------------------ the hot path
    def count_pairs(self, main_catalog: Catalog, *optional_catalog: Catalog, progress: bool = False,
                    max_workers: int | None = None, mode: str = "nn", count_type_info: str | None = None):
        """Pair counts between the patches of one (auto) or two catalogues -> one
        ``NormalisedCounts`` per scale (measurements.py:307-367). ``mode`` ("nn", "nk", "kn", "kk") picks per side the
        catalogue's weights ("n") or its weights times its scalar field ("k": the κ-weighted twin on the device); the
        normalisation is the plain sum of weights in every mode, as in the reference."""
        mode = CountMode.parse(mode)
        if len(optional_catalog) > 1:
            raise TypeError("count_pairs() takes at most two catalogues")
        if count_type_info is not None:
            _log_info("counting %s from patch pairs", count_type_info)
        auto = len(optional_catalog) == 0
        cat2 = main_catalog if auto else optional_catalog[0]
        binning = self.config.binning.binning
        num_bins, num_patches = len(binning), len(main_catalog)
        layout1, layout2 = _active_layout(main_catalog, num_bins), _active_layout(cat2, num_bins)
        side1, side2 = _count_sides(layout1, layout2, mode)  # what the device counts on: the layouts or their κ-weighted twins

        jobs = self.get_patch_pairs(main_catalog, None if auto else cat2)
        plans, thresholds = self._angular_setup()
        num_fine = thresholds.shape[1] - 1

        # Several GPUs, two ways. One process (the drop-in case): the library splits the job list over the devices of
        # its context, ``max_workers`` caps how many (the reference's worker pool, measurements.py:344-350). One process
        # per GPU under torch.distributed: the jobs are sharded over the ranks here and one sum all-reduce combines
        # the result (every slot is non-zero on exactly one rank: the sum is exact and order independent).
        rank, size = parallel.world()
        if size == 1 and not FORCE_DEVICE_REDUCE:
            # one process: the library returns the result tensor [S, B, P, P] from ONE call (yawhip_count_pairs_dense:
            # counting on the GPU(s), then separation weights, per-scale sums, the x 0.5 of an autocorrelation's diagonal
            # jobs and the scatter into the slots in C)
            if self._dense_spec is None:
                self._dense_spec = self._combine.dense_spec(num_fine)
            slices, factors = self._dense_spec
            counts, stats = engine.count_dense(side1, side2, jobs, thresholds, slices, factors, auto,
                                               sort_axis=self.sort_axis, max_workers=max_workers)
            self.last_stats = stats
            self._report(count_type_info, len(jobs), stats, progress)
            return _normalised_counts(binning, counts, layout1, layout2, auto)
        # Several ranks: balance what the device will really evaluate (lane tile x window sizes, from the item builder); the
        # partition is a plan: rank 0 derives it once per (catalogue pair, thresholds, group size) and broadcasts it.
        # The key is rank independent (every rank enters the broadcast below, or none does) and identifies the catalogue pair
        # by content that every rank shares -- per-patch sizes and the sum of weights, not an object id -- and the thresholds.
        import hashlib
        import time as _time

        devices = engine.default_devices(max_workers)  # the devices of the context the counts below run on
        group_device = devices[0]
        timings = dict(partition_ms=0.0, allreduce_ms=0.0, copy_back_ms=0.0)
        digest = hashlib.blake2b(digest_size=16)
        for part in (layout1.offsets, layout2.offsets, thresholds, jobs):
            digest.update(np.ascontiguousarray(part).tobytes())
        key = (digest.hexdigest(), side1.weighted, side2.weighted, auto, size)
        if key not in self._partitions:
            t_part = _time.perf_counter()
            parts = None
            if rank == 0:
                try:
                    work = engine.job_work(side1, side2, jobs, thresholds, sort_axis=self.sort_axis)
                    parts = parallel.partition_jobs(work.astype(np.float64) + JOB_FIXED_COST, size)
                except Exception as err:  # noqa: BLE001 -- the other ranks wait in the broadcast: tell them
                    parts = f"{type(err).__name__}: {err}"  # (as text: an exception object may not pickle)
            parts = parallel.broadcast_object(parts, device=group_device)
            if isinstance(parts, str):
                raise RuntimeError(f"the job partition could not be derived on rank 0: {parts}")
            if len(self._partitions) > 32:
                self._partitions.clear()
            self._partitions[key] = parts
            timings["partition_ms"] = (_time.perf_counter() - t_part) * 1e3
        mine = self._partitions[key][rank]
        failure, fine, rows = None, None, None
        n_compact = len(jobs) * num_bins * num_fine + 1
        # the device-resident route needs ONE device per rank; a context of several devices inside a group (YAW_AMD_DEVICES
        # naming several ids) counts with the library's in-process split and reduces through the host
        on_device = (parallel.device_collectives() or FORCE_DEVICE_REDUCE) and len(devices) == 1
        try:
            if on_device:  # this rank's rows stay in HBM, in their place of the full tensor (zero elsewhere)
                rows, stats = engine.count_rows_device(side1, side2, jobs[mine], thresholds, len(jobs), mine,
                                                       sort_axis=self.sort_axis)
            else:
                fine, stats = engine.count_fine(side1, side2, jobs[mine], thresholds, sort_axis=self.sort_axis,
                                                max_workers=max_workers)
            self.last_stats = stats
        except Exception as err:  # noqa: BLE001 -- with several ranks the others must not wait for this one forever
            failure = err

        id1, id2 = jobs[:, 0], jobs[:, 1]
        # only linked patch pairs carry counts: the tensor travels in its compact [jobs, B, E-1] form (every rank holds
        # the same job table), 9x smaller than the dense [B, E-1, P, P] at 64 patches; every row is non-zero on exactly
        # one rank, so ONE sum all-reduce (RCCL over xGMI) yields the complete tensor, exactly; one extra element carries
        # the number of ranks that failed, so that all of them raise instead of one leaving the rest blocked in the collective
        if on_device:
            compact = parallel.allreduce_device_rows(rows, n_compact, status=1.0 if failure is not None else 0.0,
                                                     device=group_device, timings=timings)
        else:
            compact = np.zeros(n_compact, dtype=np.float64)
            if failure is not None:
                compact[-1] = 1.0
            elif len(mine):
                compact[:-1].reshape(len(jobs), num_bins, num_fine)[mine] = fine
            t_red = _time.perf_counter()
            compact = parallel.allreduce_sum(compact, device=group_device)
            timings["allreduce_ms"] = (_time.perf_counter() - t_red) * 1e3
        # what a rank's call consisted of, for bench.py's self-verifying multi-GPU line (rank-local; gathered there)
        self.last_rank_info = dict(rank=rank, device=group_device, jobs=int(len(mine)), route="device" if on_device else "host",
                                   count_kernel_ms=float(self.last_stats.count_ms) if failure is None and self.last_stats else None,
                                   **timings)
        if compact[-1] > 0:
            raise RuntimeError(f"pair counting failed on {int(compact[-1])} of {size} ranks") from failure
        fine_bej = np.moveaxis(compact[:-1].reshape(len(jobs), num_bins, num_fine), 0, -1)

        # host epilogue, O(jobs * B * E): separation weights, per-scale recombination, halving of the doubly
        # counted diagonal of an autocorrelation (trees.py:358-362, measurements.py:361-364), scatter into [B, P, P]
        num_scales = self.config.scales.num_scales
        per_scale = self._combine(fine_bej)  # [S, B, n_jobs]
        skey = (auto, num_patches)
        if skey not in self._scatter:  # position of every job in a [P, P] slice and the diagonal factor
            flat = np.ascontiguousarray(id1.astype(np.int64) * num_patches + id2)
            halve = np.where(id1 == id2, 0.5, 1.0) if auto else None
            self._scatter[skey] = (flat, halve)
        flat, halve = self._scatter[skey]
        # [S, B, jobs] -> [S, B, i * P + j], zero elsewhere (one pass in the library: yawhip_host_scatter_rows)
        counts = _lib.scatter_rows((num_scales, num_bins, num_patches, num_patches), flat, per_scale, halve)
        if failure is None and self.last_stats is not None:
            self._report(count_type_info, len(jobs), self.last_stats, progress)
        return _normalised_counts(binning, counts, layout1, layout2, auto)

    def count_pairs_batch(self, requests, *, progress: bool = False, max_workers: int | None = None) -> list:
        """The pair counts of ONE measurement -- ``requests`` = ``[(catalogs, info), ...]`` or ``[(catalogs, info, mode), ...]``
        (``mode`` as in ``count_pairs``, "nn" if left out) with ``catalogs`` a tuple of one
        (auto count) or two catalogues, e.g. DD, DR, RD, RR of ``crosscorrelate``
        (src/yaw/correlation/measurements.py:617-628) -- as one submission: every count is put on the GPU's stream at once
        (``yawhip_count_pairs_dense_batch``), the host prepares count k + 1 and writes the tensor of count k while the
        device counts. Returns what ``count_pairs`` returns for each request, in order (``None`` per scale for a request
        with a missing catalogue, as ``count_pairs_optional``). With several ranks, or when the device-resident reduce is
        forced, the counts run one after the other through ``count_pairs``."""
        num_scales = self.config.scales.num_scales
        rank, size = parallel.world()
        results: list = [[None] * num_scales for _ in requests]
        todo = []
        for i, (catalogs, info, *mode) in enumerate(requests):
            mode = CountMode.parse(mode[0] if mode else "nn")
            if len(catalogs) not in (1, 2):
                raise TypeError("a count takes one or two catalogues")
            if any(cat is None for cat in catalogs):
                continue  # (count_pairs_optional: a missing random sample)
            todo.append((i, catalogs[0], catalogs[1] if len(catalogs) == 2 else None, info, mode))
        if size > 1 or FORCE_DEVICE_REDUCE or len(todo) <= 1:
            for i, main, other, info, mode in todo:
                args = (main,) if other is None else (main, other)
                results[i] = self.count_pairs(*args, progress=progress, max_workers=max_workers, mode=mode, count_type_info=info)
            return results
        binning = self.config.binning.binning
        num_bins = len(binning)
        plans, thresholds = self._angular_setup()
        if self._dense_spec is None:
            self._dense_spec = self._combine.dense_spec(thresholds.shape[1] - 1)
        slices, factors = self._dense_spec
        pairs, meta = [], []
        for i, main, other, info, mode in todo:
            auto = other is None
            cat2 = main if auto else other
            layout1, layout2 = _active_layout(main, num_bins), _active_layout(cat2, num_bins)
            side1, side2 = _count_sides(layout1, layout2, mode)
            jobs = self.get_patch_pairs(main, None if auto else cat2)
            if info is not None:
                _log_info("counting %s from patch pairs", info)
            pairs.append((side1, side2, jobs, auto))
            meta.append((i, layout1, layout2, auto, info, len(jobs)))
        outs = engine.count_dense_batch(pairs, thresholds, slices, factors, sort_axis=self.sort_axis, max_workers=max_workers)
        self.last_batch_stats = {}
        for (i, layout1, layout2, auto, info, n_jobs), (counts, stats) in zip(meta, outs):
            self.last_stats = stats
            self.last_batch_stats[info or str(i)] = stats
            self._report(info, n_jobs, stats, progress)
            results[i] = _normalised_counts(binning, counts, layout1, layout2, auto)
        return results

    def count_scalar_pairs(self, main_catalog: Catalog, *optional_catalog: Catalog, progress: bool = False,
                           max_workers: int | None = None, mode: str = "nn", count_type_info: str | None = None) -> list:
        """Pair counts of a scalar-field correlation -> one ``NormalisedScalarCounts`` per scale
        (measurements.py:394-429): the count in ``mode`` (typically "kn" or "kk") and the plain "nn" count that normalises
        it, over the same patch pairs. Both go out as ONE batch submission (``last_batch_stats`` holds the two, named
        "<info> (<mode>)" and "<info> (nn)"); several ranks count them one after the other."""
        return self._count_scalar_batch([((main_catalog, *optional_catalog), count_type_info)], mode, progress=progress,
                                        max_workers=max_workers)[0]

    def _count_scalar_batch(self, counts, mode, *, progress: bool = False, max_workers: int | None = None) -> list:
        """``count_scalar_pairs`` for several catalogue pairs of one measurement (DD and DR of ``crosscorrelate_scalar``):
        ``counts`` = ``[(catalogs, info), ...]``; two requests each, all in one ``count_pairs_batch`` submission."""
        mode = CountMode.parse(mode)
        requests = []
        for k, (catalogs, info) in enumerate(counts):
            name = info if info is not None else f"count {k}"
            requests += [(catalogs, f"{name} ({mode})", mode), (catalogs, f"{name} (nn)", CountMode.nn)]
        results = self.count_pairs_batch(requests, progress=progress, max_workers=max_workers)
        return [[NormalisedScalarCounts(kk.counts, nn.counts) for kk, nn in zip(results[2 * k], results[2 * k + 1])]
                for k in range(len(counts))]

    def count_shear_pairs(self, lenses: Catalog, sources: Catalog, *, progress: bool = False, max_workers: int | None = None,
                          count_type_info: str | None = None) -> list:
        """Shear of ``sources`` (unbinned, with ``g1`` / ``g2``) around ``lenses`` (binned in redshift) over the linked patch
        pairs -> per scale ``(NormalisedScalarCounts(T, W), NormalisedScalarCounts(X, W))``: the sums of the tangential and of
        the cross shear of the pairs, each over the sum of their weights ``w_l * w_s``. Thresholds, separation weights and
        per-scale sums are those of ``count_pairs``; ONE library call counts all jobs (``engine.count_shear_fine``), on one
        device of one process: several ranks raise ``NotImplementedError`` (``max_workers`` is accepted and has no effect)."""
        return self._count_lens_pairs(lenses, sources, count_type_info, progress, "count_shear_fine")

    def count_dsigma_pairs(self, lenses: Catalog, sources: Catalog, *, progress: bool = False, max_workers: int | None = None,
                           count_type_info: str | None = None) -> list:
        """Excess surface density of ``sources`` (unbinned, with ``g1`` / ``g2`` and redshifts) around ``lenses`` (binned, with
        redshifts), both laid out by ``build_trees(..., with_redshifts=True)``, over the linked patch pairs -> per scale
        ``(NormalisedScalarCounts(K T, W), NormalisedScalarCounts(K X, W))``: the sums of ``w_l w_s S gamma_t`` and
        ``w_l w_s S gamma_x`` over the pairs with the source behind its lens, times ``K = cosmology.DELTA_SIGMA_UNIT``, each
        over the sum of ``w_l w_s S^2``, ``S = D_A(z_l) (1 - chi_l / chi_s)`` in Mpc from the configuration's cosmology: the
        ratio is Delta Sigma in M_sun / pc^2. Everything else is ``count_shear_pairs``'; ONE library call counts all jobs
        (``engine.count_dsigma_fine``)."""
        return self._count_lens_pairs(lenses, sources, count_type_info, progress, "count_dsigma_fine", needs="excess surface density",
                                      K=DELTA_SIGMA_UNIT, cosmology=self.config.cosmology)

    def count_dsigma_radial_pairs(self, lenses: Catalog, sources: Catalog, *, shear_only: bool = False, progress: bool = False,
                                  max_workers: int | None = None, count_type_info: str | None = None) -> list:
        """``count_dsigma_pairs`` with every pair binned in its lens's OWN radius ``R = D(z_l) theta`` (physical or comoving,
        as the unit of the scales says) instead of one angle per redshift slice: the edges are the radii of ``radial_plans``,
        the same in every redshift bin (``engine.count_dsigma_radial_fine``). ``shear_only``: the sums of
        ``count_shear_pairs`` in that binning -- no factor ``S``, no ``K``, and the sources need no redshifts. The linkage must
        reach as far as the nearest lens sees the largest radius (``from_catalogs(max_angle=radial_max_angle(...))``)."""
        return self._count_lens_pairs(lenses, sources, count_type_info, progress, "count_dsigma_radial_fine", needs="a count binned per lens",
                                      source_redshifts=not shear_only, K=1.0 if shear_only else DELTA_SIGMA_UNIT, radial=True,
                                      cosmology=self.config.cosmology, unit=self.config.scales.scales.unit, unit_columns=shear_only)

    def _count_lens_pairs(self, lenses, sources, count_type_info, progress, count: str, *, needs: str | None = None,
                          source_redshifts: bool = True, K: float = 1.0, radial: bool = False, **count_args) -> list:
        """What ``count_shear_pairs``, ``count_dsigma_pairs`` and ``count_dsigma_radial_pairs`` share: the layout checks
        (``needs``: the count takes lens layouts with redshifts and unbinned sources, with redshifts too unless
        ``source_redshifts`` is off; the word opens the ``ValueError``), the engine's function ``count`` with ``count_args``
        (looked up at call time: the CPU tests replace it) and the two ratios per scale, the numerators times ``K``."""
        def layouts(num_bins):
            lens_layout, source_layout = _active_layout(lenses, num_bins), _active_layout(sources, num_bins)
            if source_layout.g1 is None or source_layout.g2 is None:
                raise ValueError("catalog has no 'g1'/'g2' attached")
            if needs is not None and (lens_layout.redshifts is None or (source_layout.redshifts is None and source_redshifts)
                                      or source_layout.num_bins != 1):
                raise ValueError(f"{needs} needs layouts with redshifts and unbinned sources: build_trees(..., with_redshifts=True)")
            return functools.partial(getattr(engine, count), **count_args), (lens_layout, source_layout)

        binning, _, (T, X, W) = self._count_shear_planes((lenses, sources), layouts, count_type_info, progress, radial=radial)
        return [tuple(NormalisedScalarCounts(PatchedCounts(binning, K * num[s], auto=False), PatchedCounts(binning, W[s], auto=False))
                      for num in (T, X))
                for s in range(len(W))]

    def count_shear_auto_pairs(self, sources: Catalog, *, progress: bool = False, max_workers: int | None = None,
                               count_type_info: str | None = None) -> list:
        """Shear-shear sums of ``sources`` (binned in redshift with ``g1`` / ``g2``: ``build_trees(edges, with_shear=True)``)
        inside every redshift bin over the linked patch pairs ``i <= j`` -> per scale ``(NormalisedScalarCounts(P, W),
        NormalisedScalarCounts(M, W), NormalisedScalarCounts(C, W))``: the numerators of xi_plus, xi_minus and xi_cross, each
        over the sum of the pair weights ``w_a * w_b``. A diagonal slot holds every unordered pair of its patch once, what an
        autocorrelation count holds after its x 0.5. Thresholds, separation weights and per-scale sums are those of
        ``count_pairs``; ONE library call counts all jobs (``engine.count_shear_auto_fine``), on one device of one process:
        several ranks raise ``NotImplementedError`` (``max_workers`` is accepted and has no effect)."""
        def layouts(num_bins):
            layout = _active_layout(sources, num_bins)
            if layout.g1 is None or layout.g2 is None:
                raise ValueError("catalog has no 'g1'/'g2' attached")
            if layout.num_bins != num_bins:
                raise ValueError("shear-shear counts need the sources binned in redshift")
            return engine.count_shear_auto_fine, (layout,)

        binning, _, (P, M, C, W) = self._count_shear_planes((sources,), layouts, count_type_info, progress)
        return [tuple(NormalisedScalarCounts(PatchedCounts(binning, num[s], auto=True), PatchedCounts(binning, W[s], auto=True))
                      for num in (P, M, C))
                for s in range(len(W))]

    def count_shear_tomographic_pairs(self, sources: Catalog, sources2: Catalog | None = None, *, bin_pairs=None,
                                      progress: bool = False, max_workers: int | None = None,
                                      count_type_info: str | None = None) -> list:
        """Shear-shear sums between redshift bin ``i`` of ``sources`` and bin ``j`` of ``sources2`` (of ``sources`` itself when
        it is left out), both binned with ``g1`` / ``g2`` (``build_trees(edges, with_shear=True)``) -> per scale a list of
        ``B`` rows, row ``i`` = ``(NormalisedScalarCounts(P, W), NormalisedScalarCounts(M, W), NormalisedScalarCounts(C, W))``
        whose ``B`` bins run over ``j``; the pair term is that of ``count_shear_auto_pairs``.

        ``bin_pairs`` lists the ``(i, j)`` to count: all ``i <= j`` of one catalogue (only those are accepted), all ``B * B``
        ordered pairs of two. Pair ``(i, i)`` of one catalogue runs over the linked patch pairs ``p <= q`` and its diagonal
        slots hold every unordered pair once, exactly what ``count_shear_auto_pairs`` stores; every other pair runs over all
        linked ``(p, q)`` in both orders, since the two bins differ. For one catalogue slot ``j < i`` of row ``i`` is the
        mirror of slot ``i`` of row ``j``, the patch axes transposed. Slots not asked for hold zeros.

        A pair is classified against the thresholds of bin ``min(i, j)``: for physical scales the angle is evaluated at the
        middle of the NEARER of the two bins (for angular scales every bin has the same). Separation weights and per-scale
        sums are ``CombinePlan``'s over those plans. ONE library call counts all cells (``engine.count_shear_pair_fine``),
        on one device of one process: several ranks raise ``NotImplementedError`` (``max_workers`` has no effect)."""
        if parallel.world()[1] > 1:
            raise NotImplementedError("shear counts run in one process on one device")
        if count_type_info is not None:
            _log_info("counting %s from patch pairs", count_type_info)
        one = sources2 is None
        binning = self.config.binning.binning
        num_bins, num_patches, num_scales = len(binning), len(sources), self.config.scales.num_scales
        layouts = [_active_layout(cat, num_bins) for cat in ((sources,) if one else (sources, sources2))]
        for layout in layouts:
            if layout.g1 is None or layout.g2 is None:
                raise ValueError("catalog has no 'g1'/'g2' attached")
            if layout.num_bins != num_bins:
                raise ValueError("shear-shear counts need the sources binned in redshift")
        if bin_pairs is None:
            bin_pairs = [(i, j) for i in range(num_bins) for j in range(i if one else 0, num_bins)]
        bin_pairs = list(dict.fromkeys((int(i), int(j)) for i, j in bin_pairs))
        for i, j in bin_pairs:
            if not (0 <= i < num_bins and 0 <= j < num_bins):
                raise ValueError(f"bin pair ({i}, {j}) is outside the {num_bins} redshift bins")
            if one and i > j:
                raise ValueError(f"bin pair ({i}, {j}): the pairs of one catalogue are given with i <= j")
        plans, thresholds = self._angular_setup()
        # the job list of a pair: p <= q inside one bin of one catalogue, every linked (p, q) otherwise
        job_lists = [self.get_patch_pairs(sources) if one and i == j else self.get_patch_pairs(sources, sources if one else sources2)
                     for i, j in bin_pairs]
        cells = np.concatenate([np.column_stack([jobs, np.full(len(jobs), i), np.full(len(jobs), j), np.full(len(jobs), min(i, j))])
                                for (i, j), jobs in zip(bin_pairs, job_lists)] or [np.empty((0, 5))]).astype(np.int32)
        *fine, stats = engine.count_shear_pair_fine(layouts[0], layouts[-1], cells, thresholds, sort_axis=self.sort_axis)
        self.last_stats = stats
        self._report(count_type_info, len(cells), stats, progress)

        planes = np.zeros((4, num_scales, num_bins, num_bins, num_patches, num_patches))  # [plane, S, i, j, p, q]
        first = np.cumsum([0] + [len(jobs) for jobs in job_lists])
        for same_bin in (True, False):  # the two job lists: pairs of each kind are combined in one pass
            group = [n for n, (i, j) in enumerate(bin_pairs) if (one and i == j) == same_bin]
            if not group:
                continue
            combine = CombinePlan([plans[min(bin_pairs[n])] for n in group])
            jobs = job_lists[group[0]]
            i_of, j_of = (np.array([bin_pairs[n][c] for n in group])[:, np.newaxis] for c in (0, 1))
            for plane, f in zip(planes, fine):
                fine_bej = np.stack([f[first[n]:first[n + 1]].T for n in group])  # [pairs, E-1, jobs]
                per_scale = combine(fine_bej)  # [S, pairs, jobs]
                plane[:, i_of, j_of, jobs[:, 0], jobs[:, 1]] = per_scale
                if one and not same_bin:
                    plane[:, j_of, i_of, jobs[:, 1], jobs[:, 0]] = per_scale
        P, M, C, W = planes
        return [[tuple(NormalisedScalarCounts(PatchedCounts(binning, num[s, i], auto=False), PatchedCounts(binning, W[s, i], auto=False))
                       for num in (P, M, C))
                 for i in range(num_bins)]
                for s in range(num_scales)]

    def count_projected_pairs(self, main_catalog: Catalog, second_catalog: Catalog | None = None, *, pi_max: float, progress: bool = False,
                              max_workers: int | None = None, count_type_info: str | None = None, pi_bins=None, signed: bool = False) -> list:
        """Pair counts of one (auto) or two catalogues with every pair binned in its OWN transverse radius
        ``R = (d_a + d_b) / 2 * theta`` (physical or comoving, as the unit of the scales says) and kept only if its
        line-of-sight separation ``|chi_a - chi_b|`` is at most ``pi_max`` (a comoving length in Mpc) -> one
        ``NormalisedCounts`` per scale on the configuration's binning, as ``count_pairs`` returns them. Both catalogues are
        binned with redshifts (``build_trees(edges, with_redshifts=True)``); bin ``k`` of one side is paired with bin ``k`` of
        the other over the linked patch pairs (``i <= j`` for an auto count). The edges are the radii of ``radial_plans``,
        the same in every redshift bin, separation weights and per-scale sums ``CombinePlan``'s. A diagonal slot of an auto
        count holds every unordered pair of its patch once -- what ``count_pairs`` holds there after its x 0.5 -- and the
        normalisation is ``count_pairs``' ``PatchedSumWeights``. The linkage must reach as far as the nearest object sees the
        largest radius (``from_catalogs(max_angle=radial_max_angle(...))``). ONE library call counts all cells
        (``engine.count_projected_fine``), on one device of one process: several ranks raise ``NotImplementedError``
        (``max_workers`` is accepted and has no effect).

        ``pi_bins`` (``engine.check_pi_edges``: a number of equal bins up to ``pi_max``, or their edges from 0 to ``pi_max``)
        bins the kept pairs in ``|chi_a - chi_b|`` besides, bin 0 ``[0, pe[1]]`` and bin j ``(pe[j], pe[j + 1]]``: the result
        is then a list over scales of lists over pi bins of ``NormalisedCounts``, every plane recombined like the one of
        ``pi_bins=None`` and all over ONE ``PatchedSumWeights``, still from one library call
        (``engine.count_projected_pi_fine``).

        ``signed=True`` keeps the sign of the line of sight between TWO catalogues: ``pi = chi(object of second_catalog) -
        chi(object of main_catalog)``, binned by ``pi_bins`` as ``engine.check_signed_pi_edges`` reads them (a number of equal
        bins from ``-pi_max`` to ``pi_max``, or edges between the two), bin 0 ``[pe[0], pe[1]]`` and bin j ``(pe[j], pe[j + 1]]``
        (``engine.count_projected_pi_signed_fine``). It needs the second catalogue and ``pi_bins`` (``ValueError``); cells and
        result are those of the unsigned count of two catalogues."""
        if parallel.world()[1] > 1:
            raise NotImplementedError("projected counts run in one process on one device")
        pi_max = engine.check_pi_max(pi_max)
        if signed:
            if second_catalog is None or pi_bins is None:
                raise ValueError("a signed projected count needs a second catalogue and pi_bins: one catalogue against itself "
                                 "has no order, and the sign lives in the pi bins")
            pi_edges = engine.check_signed_pi_edges(pi_bins, pi_max)
        else:
            pi_edges = None if pi_bins is None else engine.check_pi_edges(pi_bins, pi_max)

        def call(layout1, layout2, cells, r2, **kwargs):
            if signed:
                return engine.count_projected_pi_signed_fine(layout1, layout2, cells, r2, pi_edges=pi_edges, **kwargs)
            if pi_edges is not None:  # one plane per pi bin
                return engine.count_projected_pi_fine(layout1, layout2, cells, r2, pi_edges=pi_edges, **kwargs)
            fine, stats = engine.count_projected_fine(layout1, layout2, cells, r2, pi_max=pi_max, **kwargs)
            return np.asarray(fine, dtype=np.float64)[None], stats

        planes = self._count_projected_cells(main_catalog, second_catalog, call, count_type_info, progress)
        return planes[0] if pi_edges is None else [list(per_pi) for per_pi in zip(*planes)]

    def count_smu_pairs(self, main_catalog: Catalog, second_catalog: Catalog | None = None, *, mu_bins, progress: bool = False,
                        max_workers: int | None = None, count_type_info: str | None = None, signed: bool = False) -> list:
        """Pair counts of one (auto) or two catalogues binned in the redshift-space separation ``s`` and in ``mu = pi / s``:
        ``s^2 = r_p^2 + pi^2`` with ``r_p = (d_a + d_b) / 2 * theta`` and ``pi = |chi_a - chi_b|`` of
        ``count_projected_pairs``, and no line-of-sight cut -> a list over scales of lists over mu bins of
        ``NormalisedCounts``. The scales of the configuration are read as ``s``; ``mu_bins`` (``engine.check_mu_edges``) is
        a number of equal bins of ``mu`` in [0, 1] or their edges, bin 0 ``[0, mu_1]`` and bin j ``(mu_j, mu_{j+1}]``.
        Catalogues, cells, recombination (``CombinePlan`` of ``radial_plans``), diagonal slots, linkage and the one-process
        rule are ``count_projected_pairs``'; every plane is recombined alike and all are over ONE ``PatchedSumWeights``,
        from one library call (``engine.count_smu_fine``).

        ``signed=True`` keeps the sign of ``mu`` between TWO catalogues: ``pi = chi(object of second_catalog) - chi(object of
        main_catalog)`` and ``mu_bins`` as ``engine.check_signed_mu_edges`` reads them, from -1 to 1
        (``engine.count_smu_signed_fine``). It needs the second catalogue (``ValueError``)."""
        if parallel.world()[1] > 1:
            raise NotImplementedError("projected counts run in one process on one device")
        if signed and second_catalog is None:
            raise ValueError("a signed redshift-space count needs a second catalogue: one catalogue against itself has no order")
        mu_edges = engine.check_signed_mu_edges(mu_bins) if signed else engine.check_mu_edges(mu_bins)
        count_fine = engine.count_smu_signed_fine if signed else engine.count_smu_fine

        def call(layout1, layout2, cells, s2, **kwargs):
            return count_fine(layout1, layout2, cells, s2, mu_edges=mu_edges, **kwargs)

        planes = self._count_projected_cells(main_catalog, second_catalog, call, count_type_info, progress)
        return [list(per_mu) for per_mu in zip(*planes)]

    def count_alignment_pairs(self, shapes: Catalog, density: Catalog, *, pi_max: float, pi_bins=None, progress: bool = False,
                              max_workers: int | None = None, count_type_info: str | None = None) -> list:
        """The projected position-shape sums of the catalogue ``shapes`` (shear and redshifts: ``build_trees(edges,
        with_shear=True, with_redshifts=True)``) about the objects of ``density`` (redshifts): every pair is binned in its own
        radius and in ``pi = |chi_a - chi_b|`` as ``count_projected_pairs(pi_bins=...)`` bins it (``pi_bins=None``: one bin
        ``[0, pi_max]``), and adds its weight times the shape's ellipticity rotated to the great circle through the pair ->
        a list over scales of lists over pi bins of ``(T, X, W)``, three ``NormalisedCounts`` over the ONE
        ``PatchedSumWeights`` of (density, shapes). T is the tangential ellipticity about the density object, negative for
        a shape that points at it; T and X are signed sums. All linked patch pairs ``(p, q)`` are counted, never ``p <= q``
        only, also where the two catalogues hold the same objects: slot ``[bin, p, q]`` pairs patch ``p`` of ``density`` with
        patch ``q`` of ``shapes``. Cells, recombination, linkage and the one-process rule are ``count_projected_pairs``';
        ONE library call counts all cells (``engine.count_projected_shear_fine``)."""
        if parallel.world()[1] > 1:
            raise NotImplementedError("projected counts run in one process on one device")
        _require_distinct(shapes, density)
        pi_edges = engine.check_pi_edges(1 if pi_bins is None else pi_bins, pi_max)

        def call(dens_layout, shape_layout, cells, r2, **kwargs):
            if shape_layout.g1 is None or shape_layout.g2 is None:
                raise ValueError("the shape catalogue carries no shear: build_trees(edges, with_shear=True, with_redshifts=True)")
            planes, stats = engine.count_projected_shear_fine(dens_layout, shape_layout, cells, r2, pi_edges=pi_edges, **kwargs)
            return np.concatenate([np.asarray(plane, dtype=np.float64) for plane in planes]), stats  # [3 n_pi, n_cells, E-1]

        planes = self._count_projected_cells(density, shapes, call, count_type_info, progress)
        n_pi = len(pi_edges) - 1
        return [[(t[s], x[s], w[s]) for t, x, w in zip(planes[:n_pi], planes[n_pi:2 * n_pi], planes[2 * n_pi:])]
                for s in range(self.config.scales.num_scales)]

    def count_shape_pairs(self, shapes: Catalog, shapes2: Catalog | None = None, *, pi_max: float, pi_bins=None, progress: bool = False,
                          max_workers: int | None = None, count_type_info: str | None = None) -> list:
        """The projected shape-shape sums of the catalogue ``shapes`` with itself (``shapes2=None``: the linked patch pairs
        ``p <= q``, a diagonal slot holding every unordered pair of its patch once, as ``count_projected_pairs`` counts an
        auto count) or with a second shape catalogue (all linked patch pairs): every pair is binned in its own radius and in
        ``pi = |chi_a - chi_b|`` as ``count_projected_pairs(pi_bins=...)`` bins it (``pi_bins=None``: one bin ``[0, pi_max]``),
        and BOTH ellipticities are rotated to the great circle through the pair -> a list over scales of lists over pi bins
        of ``(PP, XX, PX, W)``, four ``NormalisedCounts`` over ONE ``PatchedSumWeights``: the sums of ``w_a w_b et_a et_b``,
        ``w_a w_b ex_a ex_b``, ``w_a w_b (et_a ex_b + ex_a et_b)`` (signed; ``et = -e+`` the tangential ellipticity of
        ``count_alignment_pairs``, so PX is minus the ``+x`` product) and of ``w_a w_b``. The catalogues carry shear and
        redshifts (``build_trees(edges, with_shear=True, with_redshifts=True)``). Cells, recombination, linkage and the
        one-process rule are ``count_projected_pairs``'; ONE library call counts all cells
        (``engine.count_projected_shapes_fine``)."""
        if parallel.world()[1] > 1:
            raise NotImplementedError("projected counts run in one process on one device")
        _require_distinct(shapes, shapes2)
        pi_edges = engine.check_pi_edges(1 if pi_bins is None else pi_bins, pi_max)

        def call(layout_a, layout_b, cells, r2, **kwargs):
            if any(layout.g1 is None or layout.g2 is None for layout in (layout_a, layout_b)):
                raise ValueError("a shape catalogue carries no shear: build_trees(edges, with_shear=True, with_redshifts=True)")
            planes, stats = engine.count_projected_shapes_fine(layout_a, layout_b, cells, r2, pi_edges=pi_edges, **kwargs)
            return np.concatenate([np.asarray(plane, dtype=np.float64) for plane in planes]), stats  # [4 n_pi, n_cells, E-1]

        planes = self._count_projected_cells(shapes, shapes2, call, count_type_info, progress)
        n_pi = len(pi_edges) - 1
        return [[tuple(planes[c * n_pi + j][s] for c in range(4)) for j in range(n_pi)] for s in range(self.config.scales.num_scales)]

    def _count_projected_cells(self, main_catalog, second_catalog, call, count_type_info, progress) -> list:
        """What the counts over projected handles share: the layout checks, the cell list of the linked patch pairs and
        ``_count_shear_planes`` on the radial plan. ``call(layout1, layout2, cells, r2, cosmology=, unit=, sort_axis=)`` is the
        engine's count and returns ``(f64[n_planes, n_cells, E-1], CountStats)``. Returns per plane the list over scales of
        ``NormalisedCounts``, all over one ``PatchedSumWeights``."""
        auto = second_catalog is None

        def layouts(num_bins):
            layout1, layout2 = _active_layout(main_catalog, num_bins), _active_layout(main_catalog if auto else second_catalog, num_bins)
            for layout in (layout1, layout2):
                if layout.redshifts is None or layout.num_bins != num_bins:
                    raise ValueError("a projected count needs layouts binned in redshift that carry redshifts: "
                                     "build_trees(edges, with_redshifts=True)")

            def count(layout1, layout2, jobs, r2, *, sort_axis):
                # cell (job, k): segment (p, k) of the first side against (q, k) of the second, row k; diagonal iff one segment twice
                seg1 = (jobs[:, :1].astype(np.int64) * num_bins + np.arange(num_bins)).ravel()
                seg2 = (jobs[:, 1:].astype(np.int64) * num_bins + np.arange(num_bins)).ravel()
                diagonal = (seg1 == seg2) if auto else np.zeros(len(seg1), dtype=bool)
                cells = np.column_stack([seg1, seg2, np.tile(np.arange(num_bins), len(jobs)), diagonal]).astype(np.int32).reshape(-1, 4)
                fine, stats = call(layout1, layout2, cells, r2, cosmology=self.config.cosmology, unit=self.config.scales.scales.unit,
                                   sort_axis=sort_axis)
                fine = np.asarray(fine, dtype=np.float64)
                return (*fine.reshape(len(fine), len(jobs), num_bins, r2.shape[1] - 1), stats)

            return count, (layout1, layout2)

        catalogs = (main_catalog,) if auto else (main_catalog, second_catalog)
        binning, (layout1, layout2), planes = self._count_shear_planes(catalogs, layouts, count_type_info, progress, radial=True)
        return _normalised_counts(binning, planes, layout1, layout2, auto)

    def _count_shear_planes(self, catalogs, layouts, count_type_info, progress, radial: bool = False):
        """What the lensing and projected counts share. ``layouts(num_bins)`` makes the caller's layout checks and returns the
        count (a function of the engine, looked up at call time: the CPU tests replace them) with the layouts it takes; its job
        list is ``get_patch_pairs(*catalogs)``. Returns the binning, those layouts and one f64[S, B, P, P] per plane of the
        count, zero outside the jobs. ``radial``: edges and recombination are those of the configuration's radial plan
        (``radial_plans``), the same for every redshift bin."""
        if parallel.world()[1] > 1:
            raise NotImplementedError("shear counts run in one process on one device")
        if count_type_info is not None:
            _log_info("counting %s from patch pairs", count_type_info)
        binning = self.config.binning.binning
        num_bins, num_patches = len(binning), len(catalogs[0])
        count_fine, count_layouts = layouts(num_bins)
        jobs = self.get_patch_pairs(*catalogs)
        if radial:
            plans = radial_plans(self.config)
            thresholds, combine = threshold_table(plans), CombinePlan(plans)
        else:
            _, thresholds = self._angular_setup()
            combine = self._combine
        *fine, stats = count_fine(*count_layouts, jobs, thresholds, sort_axis=self.sort_axis)
        self.last_stats = stats
        self._report(count_type_info, len(jobs), stats, progress)
        flat = np.ascontiguousarray(jobs[:, 0].astype(np.int64) * num_patches + jobs[:, 1])
        shape = (self.config.scales.num_scales, num_bins, num_patches, num_patches)
        # [jobs, B, E-1] -> separation weights and per-scale sums [S, B, jobs] -> [S, B, i * P + j], zero elsewhere
        return binning, count_layouts, [_lib.scatter_rows(shape, flat, combine(np.moveaxis(f, 0, -1))) for f in fine]

    @staticmethod
    def _report(what, n_jobs, stats, progress) -> None:
        """The reference logs every pair count and shows a progress bar over its patch-pair tasks
        (src/yaw/correlation/measurements.py:53-62,344-350); one GPU call has no tasks to tick off, so ``progress`` prints
        one summary line per count instead. Rank 0 only."""
        if not progress and not logger.isEnabledFor(logging.INFO):
            return  # nobody listens: the line is not even formatted (a pair count can be a 0.5 ms call)
        if parallel.world()[0] != 0:
            return
        secs = max(stats.total_ms, 1e-6) / 1e3
        line = (f"{what or 'pair count'}: {n_jobs} patch pairs, {stats.candidate_pairs:.4g} candidate pairs in "
                f"{stats.total_ms:.2f} ms ({stats.candidate_pairs / secs:.3g} pairs/s)")
        logger.info(line)
        if progress:
            print(line, flush=True)

    def count_pairs_optional(self, main_catalog, *optional_catalog, **kwargs):
        """``count_pairs`` that yields ``None`` per scale if any catalogue is missing
        (measurements.py:369-392)."""
        if any(cat is None for cat in (main_catalog, *optional_catalog)):
            return [None] * self.config.scales.num_scales
        return self.count_pairs(main_catalog, *optional_catalog, **kwargs)


def _active_layout(catalog: Catalog, num_bins: int):
    layout = catalog._active_layout
    if layout is None:  # the reference fails in BinnedTrees.__init__ (trees.py:473-474)
        raise FileNotFoundError("no trees found for catalog: call build_trees() first")
    if layout.num_bins not in (1, num_bins):
        raise ValueError(f"catalog was binned into {layout.num_bins} redshift bins, configuration has {num_bins}")
    return layout


def _normalised_counts(binning, counts, layout1, layout2, auto: bool) -> list:
    """The result tensor ``counts`` f64[S, B, P, P] of a pair count between two layouts as one ``NormalisedCounts`` per scale,
    all over the one ``PatchedSumWeights`` of the layouts. A list of such tensors (the planes of one count) gives a list of
    such lists, over the same ``PatchedSumWeights``."""
    num_bins = len(binning)
    sum_weights = PatchedSumWeights(binning, layout1.sum_weights_for(num_bins), layout2.sum_weights_for(num_bins), auto=auto)

    def per_scale(tensor):
        return [NormalisedCounts(PatchedCounts(binning, tensor[s], auto=auto), sum_weights) for s in range(len(tensor))]

    return [per_scale(tensor) for tensor in counts] if isinstance(counts, list) else per_scale(counts)


def _count_sides(layout1, layout2, mode):
    """The layouts a count in ``mode`` runs on: per side the layout itself ("n") or its κ-weighted twin ("k"). A "k" side
    without a scalar field raises as ``AngularTree.get_pair_weights`` does (trees.py:284-301)."""
    k1, k2 = mode[0] == "k", mode[1] == "k"
    if k1 and k2:
        if layout1.kappa is None or layout2.kappa is None:
            raise ValueError("missing required 'kappa' for both tree.")
    elif k1 and layout1.kappa is None:
        raise ValueError("missing required 'kappa' for first tree.")
    elif k2 and layout2.kappa is None:
        raise ValueError("missing required 'kappa' for second tree.")
    return (layout1.twin if k1 else layout1), (layout2.twin if k2 else layout2)


def _require_distinct(*catalogs) -> None:
    """Counterpart of ``ensure_unique_catalogs`` (measurements.py:432-448): the reference rejects
    catalogues that share a cache directory; here the state that must not be shared is the active
    layout of a catalogue object."""
    present = [cat for cat in catalogs if cat is not None]
    if len({id(cat) for cat in present}) != len(present):
        raise ValueError("each catalog must be a separate Catalog instance to avoid interference.")


def autocorrelate(config, data: Catalog, random: Catalog, *, count_rr: bool = True, progress: bool = False,
                  max_workers: int | None = None) -> list:
    """Angular autocorrelation in redshift slices: DD, DR and (optionally) RR -> ``[CorrFunc]``, one
    per scale (measurements.py:455-525)."""
    _require_distinct(data, random)
    edges, closed = config.binning.edges, config.binning.closed
    _log_info("building data trees")
    data.build_trees(edges, closed=closed)
    _log_info("building random trees")
    random.build_trees(edges, closed=closed)
    _log_info("computing auto-correlation from DD, DR" + (", RR" if count_rr else ""))
    links = PatchLinkage.from_catalogs(config, data, random)
    # the reference issues DD, DR, RR one after the other (measurements.py:517-523); here they are ONE submission
    DD, DR, RR = links.count_pairs_batch(
        [((data,), "DD"), ((data, random), "DR"), ((random if count_rr else None,), "RR")],
        progress=progress, max_workers=max_workers)
    return [CorrFunc(dd, dr, None, rr) for dd, dr, rr in zip(DD, DR, RR)]


def autocorrelate_projected(config, data: Catalog, random: Catalog, *, pi_max: float, count_rr: bool = True, progress: bool = False,
                            max_workers: int | None = None, pi_bins=None) -> list:
    """Projected clustering of ``data`` in each pair's own transverse radius: DD, DR and (optionally) RR of the pairs with a
    line-of-sight separation ``|chi_a - chi_b| <= pi_max``, binned by ``r_p = (d_a + d_b) / 2 * theta`` -> ``[CorrFunc(dd, dr,
    None, rr)]``, one per scale of the configuration (no counterpart in the reference).

    ``cf.sample()`` is the Landy-Szalay estimate (Davis-Peebles without RR) of the correlation function averaged over the
    cylinder ``|pi| <= pi_max`` in each radius bin, ``xi_bar``, with jackknife samples over the patches; the projected
    correlation function is ``w_p(r_p) = 2 * pi_max * xi_bar``. This is the single-cylinder estimator: the pairs are not
    binned in ``pi``, and ``xi(r_p, pi)`` is not integrated bin by bin.

    ``pi_bins`` asks for that estimator instead: a number ``n >= 1`` of equal bins from 0 to ``pi_max``,
    or their edges (from 0, strictly ascending, ending at ``pi_max``). DD, DR and RR are then binned in
    ``pi = |chi_a - chi_b|`` besides -- bin 0 ``[0, pe[1]]``, bin j ``(pe[j], pe[j + 1]]`` -- and the result is
    ``[ProjectedCorrFunc]``, one per scale: ``sample_xi()`` gives ``xi(r_p, pi_j)`` per pi bin, ``sample()`` the summed
    ``w_p = 2 sum_j dpi_j xi_j`` with its jackknife samples, ``cylinder()`` the single-cylinder ``CorrFunc`` of
    ``pi_bins=None``. The number of pi bins times the fine radius bins of the configuration's resolution is capped by the
    device's LDS (104 pi bins at 12 fine bins); beyond the cap the call is a ``ValueError`` that states it.

    The scales are transverse radii in a physical (``kpc``, ``Mpc``: ``d = D_A(z)``) or comoving (``kpc/h``, ``Mpc/h``:
    ``d = D_A(z) (1 + z)``) unit; an angular unit is a ``ValueError``. ``pi_max`` is a comoving length in the Mpc the scales
    are converted with (``Scales`` reads the ``/h`` units as comoving lengths and applies no factor ``h``), finite and
    ``> 0``. Both catalogues need redshifts, finite and ``> 0``. An object so near that the largest radius spans more than
    5.73 degrees is a ``ValueError`` that names its redshift.

    Pairs are counted INSIDE a redshift bin of the configuration, as ``autocorrelate`` and ``autocorrelate_shear`` count
    them: a pair across a bin edge is not counted however close it is in ``pi``. A ``w_p`` measurement therefore takes one
    bin (or a few wide bins) over the whole sample. The counts run on one device of one process: several ranks raise
    ``NotImplementedError`` (``max_workers`` is accepted and has no effect)."""
    _require_distinct(data, random)
    if parallel.world()[1] > 1:
        raise NotImplementedError("projected counts run in one process on one device")
    pi_max = engine.check_pi_max(pi_max)
    pi_edges = None if pi_bins is None else engine.check_pi_edges(pi_bins, pi_max)
    unit = config.scales.scales.unit
    engine.radial_kind(unit)  # angular units have no radius: ValueError
    edges, closed = config.binning.edges, config.binning.closed
    _log_info("building data trees")
    data_layout = data.build_trees(edges, closed=closed, with_redshifts=True)
    _log_info("building random trees")
    random_layout = random.build_trees(edges, closed=closed, with_redshifts=True)
    for layout in (data_layout, random_layout):
        engine.check_proj_redshifts(layout)
    _log_info("computing projected auto-correlation from DD, DR" + (", RR" if count_rr else ""))
    links = PatchLinkage.from_catalogs(config, data, random, max_angle=radial_max_angle(config, data_layout, random_layout))
    kwargs = dict(pi_max=pi_max, progress=progress, max_workers=max_workers, pi_bins=pi_edges)
    DD = links.count_projected_pairs(data, count_type_info="DD", **kwargs)
    DR = links.count_projected_pairs(data, random, count_type_info="DR", **kwargs)
    RR = links.count_projected_pairs(random, count_type_info="RR", **kwargs) if count_rr else [None] * len(DD)
    if pi_edges is None:
        return [CorrFunc(dd, dr, None, rr) for dd, dr, rr in zip(DD, DR, RR)]
    return [ProjectedCorrFunc(pi_edges, [CorrFunc(dd_j, dr_j, None, None if rr is None else rr[j]) for j, (dd_j, dr_j) in enumerate(zip(dd, dr))])
            for dd, dr, rr in zip(DD, DR, RR)]


def autocorrelate_multipoles(config, data: Catalog, random: Catalog, *, mu_bins, count_rr: bool = True, progress: bool = False,
                             max_workers: int | None = None) -> list:
    """Redshift-space clustering of ``data``: DD, DR and (optionally) RR binned in the redshift-space separation
    ``s = sqrt(r_p^2 + pi^2)`` and in ``mu = pi / s``, with ``r_p = (d_a + d_b) / 2 * theta`` and ``pi = |chi_a - chi_b|`` as
    ``autocorrelate_projected`` has them and no line-of-sight cut -> ``[MultipoleCorrFunc]``, one per scale of the
    configuration (no counterpart in the reference). ``sample_xi()`` gives ``xi(s, mu_j)`` per mu bin,
    ``sample(ell)`` the multipole ``xi_ell(s) = (2 ell + 1) sum_j xi_j int_{mu_j}^{mu_{j+1}} P_ell(mu) dmu`` with its jackknife
    samples, ``sample_multipoles()`` the monopole, quadrupole and hexadecapole.

    ``mu_bins`` is a number ``n >= 1`` of equal bins of ``mu`` in [0, 1], or their edges (from 0 to 1, strictly ascending):
    bin 0 is ``[0, mu_1]``, bin j ``(mu_j, mu_{j+1}]``; ``mu`` is unsigned. The number of mu bins times the fine bins of the
    configuration's resolution is capped by the device's LDS (104 mu bins at 12 fine bins, 25 at 50); beyond the cap the
    call is a ``ValueError`` that states it.

    The scales of the configuration are read as ``s``: in ``kpc`` / ``Mpc`` with ``d = D_A(z)``, in ``kpc/h`` / ``Mpc/h``
    with the comoving ``d = D_A(z) (1 + z)``; an angular unit is a ``ValueError``. The line-of-sight coordinate is the
    comoving distance whatever the unit, as for ``w_p``, so the comoving units are the consistent choice for ``s``: with a
    physical unit the transverse part of ``s`` is physical and the line-of-sight part comoving. Both catalogues need
    redshifts, finite and ``> 0``. An object so near that the largest ``s`` spans more than 5.73 degrees is a
    ``ValueError`` that names its redshift.

    Pairs are counted INSIDE a redshift bin of the configuration, as ``autocorrelate_projected`` counts them, on one device
    of one process: several ranks raise ``NotImplementedError`` (``max_workers`` is accepted and has no effect)."""
    _require_distinct(data, random)
    if parallel.world()[1] > 1:
        raise NotImplementedError("projected counts run in one process on one device")
    mu_edges = engine.check_mu_edges(mu_bins)
    engine.radial_kind(config.scales.scales.unit)  # angular units have no radius: ValueError
    edges, closed = config.binning.edges, config.binning.closed
    _log_info("building data trees")
    data_layout = data.build_trees(edges, closed=closed, with_redshifts=True)
    _log_info("building random trees")
    random_layout = random.build_trees(edges, closed=closed, with_redshifts=True)
    for layout in (data_layout, random_layout):
        engine.check_proj_redshifts(layout)
    _log_info("computing redshift-space auto-correlation from DD, DR" + (", RR" if count_rr else ""))
    links = PatchLinkage.from_catalogs(config, data, random, max_angle=radial_max_angle(config, data_layout, random_layout))
    kwargs = dict(mu_bins=mu_edges, progress=progress, max_workers=max_workers)
    DD = links.count_smu_pairs(data, count_type_info="DD", **kwargs)
    DR = links.count_smu_pairs(data, random, count_type_info="DR", **kwargs)
    RR = links.count_smu_pairs(random, count_type_info="RR", **kwargs) if count_rr else [None] * len(DD)
    return [MultipoleCorrFunc(mu_edges, [CorrFunc(dd_j, dr_j, None, None if rr is None else rr[j]) for j, (dd_j, dr_j) in enumerate(zip(dd, dr))])
            for dd, dr, rr in zip(DD, DR, RR)]


def _crosscorrelate_radial(config, data1, data2, rand1, rand2, count_rr, what: str, count) -> list:
    """What the two cross-correlations in a radius share: the checks, the trees with redshifts of every catalogue given, ONE
    linkage that reaches as far as the nearest object of any of them sees the largest scale, and the four counts in the
    slots in which ``crosscorrelate`` puts them -- D1D2, D1R2 (``dr``) where ``rand2`` is given, R1D2 (``rd``) where ``rand1`` is,
    R1R2 where both are and ``count_rr``. ``count(links, first, second, info)`` is the linkage's count of two catalogues, a
    list over scales of lists over the bins of the second binning (or of ``NormalisedCounts``, where there is none).
    Returns ``(DD, DR, RD, RR)``, ``None`` for a count that was not asked for."""
    _require_distinct(data1, data2, rand1, rand2)
    if parallel.world()[1] > 1:
        raise NotImplementedError("projected counts run in one process on one device")
    count_dr, count_rd = rand2 is not None, rand1 is not None
    if not count_dr and not count_rd:
        raise ValueError("at least one random dataset must be provided")
    engine.radial_kind(config.scales.scales.unit)  # angular units have no radius: ValueError
    edges, closed = config.binning.edges, config.binning.closed
    catalogs = [cat for cat in (data1, data2, rand1, rand2) if cat is not None]
    _log_info("building trees")
    layouts = [cat.build_trees(edges, closed=closed, with_redshifts=True) for cat in catalogs]
    for layout in layouts:
        engine.check_proj_redshifts(layout)
    count_rr = count_rr and count_dr and count_rd
    _log_info(f"computing {what} cross-correlation from DD" + (", DR" if count_dr else "") + (", RD" if count_rd else "")
              + (", RR" if count_rr else ""))
    # (the linkage holds every catalogue's patch centres against those of the largest: check_patch_conistency)
    links = PatchLinkage.from_catalogs(config, *catalogs, max_angle=radial_max_angle(config, *layouts))
    return (count(links, data1, data2, "DD"), count(links, data1, rand2, "DR") if count_dr else None,
            count(links, rand1, data2, "RD") if count_rd else None, count(links, rand1, rand2, "RR") if count_rr else None)


def _binned_corrfuncs(result_type, edges, DD, DR, RD, RR) -> list:
    """One ``result_type(edges, [CorrFunc(dd_j, dr_j, rd_j, rr_j) per bin j])`` per scale from the four counts of
    ``_crosscorrelate_radial`` with a second binning."""
    num_scales = len(DD)
    DR, RD, RR = ([None] * num_scales if counts is None else counts for counts in (DR, RD, RR))
    return [result_type(edges, [CorrFunc(dd_j, *(None if counts is None else counts[j] for counts in (dr, rd, rr))) for j, dd_j in enumerate(dd)])
            for dd, dr, rd, rr in zip(DD, DR, RD, RR)]


def crosscorrelate_projected(config, data1: Catalog, data2: Catalog, rand1: Catalog | None = None, rand2: Catalog | None = None, *,
                             pi_max: float, pi_bins=None, signed: bool = False, count_rr: bool = True, progress: bool = False,
                             max_workers: int | None = None) -> list:
    """Projected cross-correlation of two samples in each pair's own transverse radius: ``autocorrelate_projected`` between
    ``data1`` and ``data2`` (no counterpart in the reference). D1D2 is always counted, D1R2 where
    ``rand2`` is given, R1D2 where ``rand1`` is, R1R2 where both are and ``count_rr``; at least one random catalogue is
    required. The four go into ``CorrFunc(dd, dr, rd, rr)`` as ``crosscorrelate`` fills it, and ``CorrFunc`` chooses the
    estimator: Landy-Szalay with RR, Davis-Peebles otherwise.

    ``signed=False`` bins ``pi = |chi_2 - chi_1|`` and returns, per scale, what ``autocorrelate_projected`` returns: a
    ``CorrFunc`` of the cylinder ``pi <= pi_max`` (``pi_bins=None``) or a ``ProjectedCorrFunc``.

    ``signed=True`` keeps the sign, ``pi = chi(object of data2 or rand2) - chi(object of data1 or rand1)``, positive where the
    second sample's object lies behind: for two different tracers ``xi(r_p, pi)`` is not symmetric in ``pi``. ``pi_bins`` is
    then required: a number ``n >= 1`` of equal bins from ``-pi_max`` to ``pi_max``, or their edges, strictly ascending
    between the two and symmetric inside or not. The result is ``[SignedProjectedCorrFunc]``, one per scale: ``sample_xi()``
    per signed bin, ``sample()`` the ``w_p = sum_j dpi_j xi_j`` over both signs, ``folded()`` the result of ``signed=False``
    over the mirrored edges. The cap on the number of bins is ``autocorrelate_projected``'s, the signed bins counted as
    they are.

    All catalogues carry redshifts and share their patch centres. Units, ``pi_max``, redshift bins (pairs are counted INSIDE
    a bin), reach and the one-process rule are ``autocorrelate_projected``'s."""
    pi_max = engine.check_pi_max(pi_max)
    if signed:
        if pi_bins is None:
            raise ValueError("a signed projected correlation needs pi_bins: the sign lives in the pi bins")
        pi_edges = engine.check_signed_pi_edges(pi_bins, pi_max)
    else:
        pi_edges = None if pi_bins is None else engine.check_pi_edges(pi_bins, pi_max)

    def count(links, first, second, info):
        return links.count_projected_pairs(first, second, pi_max=pi_max, pi_bins=pi_edges, signed=signed, progress=progress,
                                           max_workers=max_workers, count_type_info=info)

    DD, DR, RD, RR = _crosscorrelate_radial(config, data1, data2, rand1, rand2, count_rr, "projected", count)
    if pi_edges is None:
        DR, RD, RR = ([None] * len(DD) if counts is None else counts for counts in (DR, RD, RR))
        return [CorrFunc(dd, dr, rd, rr) for dd, dr, rd, rr in zip(DD, DR, RD, RR)]
    return _binned_corrfuncs(SignedProjectedCorrFunc if signed else ProjectedCorrFunc, pi_edges, DD, DR, RD, RR)


def crosscorrelate_multipoles(config, data1: Catalog, data2: Catalog, rand1: Catalog | None = None, rand2: Catalog | None = None, *,
                              mu_bins, signed: bool = False, count_rr: bool = True, progress: bool = False,
                              max_workers: int | None = None) -> list:
    """Redshift-space cross-correlation of two samples: ``autocorrelate_multipoles`` between ``data1`` and ``data2`` (no
    counterpart in the reference), with the counts, the randoms and the estimator of
    ``crosscorrelate_projected``.

    ``signed=False`` bins the unsigned ``mu`` over ``mu_bins`` in [0, 1] and returns ``[MultipoleCorrFunc]``. ``signed=True``
    keeps the sign of ``pi = chi(object of data2 or rand2) - chi(object of data1 or rand1)`` on ``mu = pi / s``: ``mu_bins`` is a
    number ``n >= 1`` of equal bins from -1 to 1, or their edges, and the result is ``[SignedMultipoleCorrFunc]``, whose
    ``sample(ell)`` measures the odd multipoles too (the dipole and octupole of two different tracers) and whose ``folded()``
    is the result of ``signed=False`` over the mirrored edges. The cap on the number of bins is
    ``autocorrelate_multipoles``', the signed bins counted as they are.

    All catalogues carry redshifts and share their patch centres. Units, redshift bins (pairs are counted INSIDE a bin),
    reach and the one-process rule are ``autocorrelate_multipoles``'."""
    mu_edges = engine.check_signed_mu_edges(mu_bins) if signed else engine.check_mu_edges(mu_bins)

    def count(links, first, second, info):
        return links.count_smu_pairs(first, second, mu_bins=mu_edges, signed=signed, progress=progress, max_workers=max_workers,
                                     count_type_info=info)

    DD, DR, RD, RR = _crosscorrelate_radial(config, data1, data2, rand1, rand2, count_rr, "redshift-space", count)
    return _binned_corrfuncs(SignedMultipoleCorrFunc if signed else MultipoleCorrFunc, mu_edges, DD, DR, RD, RR)


def crosscorrelate_alignment(config, shapes: Catalog, density: Catalog, density_rand: Catalog, *, pi_max: float, pi_bins=None,
                             shape_rand: Catalog | None = None, progress: bool = False, max_workers: int | None = None) -> list:
    """Projected position-shape correlation of the shape sample ``shapes`` with the density sample ``density``: the
    intrinsic-alignment measurement ``w_g+(r_p)`` and its null test ``w_gx(r_p)`` -> ``[AlignmentCorrFunc]``, one per scale
    of the configuration (no counterpart in the reference). ``cf.sample("plus")`` is ``w_g+``,
    positive for shapes that point at the density objects, ``cf.sample("cross")`` is ``w_gx``, both with jackknife samples
    over the patches; ``cf.sample_xi(component)`` gives the pi bins.

    Every pair of a shape and a density object is binned in its own radius ``r_p = (d_a + d_b) / 2 * theta`` and in
    ``pi = |chi_a - chi_b| <= pi_max``, and the shape's ellipticity is rotated to the great circle through the pair. Two
    library calls of the new count sum the planes of shapes x density (SD) and shapes x density randoms (SR); the estimator
    is ``(SD - SR) / N`` per pi bin with ``N`` the pair count W of SR, or of ``shape_rand`` x ``density_rand`` where shape
    randoms are given (one more call, of the count of ``autocorrelate_projected``). ``pi_bins`` is a number of equal bins
    from 0 to ``pi_max`` or their edges; ``None`` is one bin ``[0, pi_max]``. The number of pi bins is capped by the device's
    LDS at a third of ``autocorrelate_projected``'s (35 at 12 fine bins, 8 at 50); beyond the cap the call is a
    ``ValueError`` that states it.

    ``shapes`` carries ``g1`` / ``g2`` and redshifts, ``density``, ``density_rand`` and ``shape_rand`` redshifts. Units,
    ``pi_max``, redshift bins (pairs are counted INSIDE a bin), reach and the one-process rule are
    ``autocorrelate_projected``'s; all catalogues are separate ``Catalog`` instances."""
    _require_distinct(shapes, density, density_rand, shape_rand)
    if parallel.world()[1] > 1:
        raise NotImplementedError("projected counts run in one process on one device")
    pi_edges = engine.check_pi_edges(1 if pi_bins is None else pi_bins, pi_max)
    engine.radial_kind(config.scales.scales.unit)  # angular units have no radius: ValueError
    edges, closed = config.binning.edges, config.binning.closed
    if not shapes.has_shear:
        raise ValueError("the shape catalogue has no 'g1'/'g2' attached")
    _log_info("building trees")
    layouts = [shapes.build_trees(edges, closed=closed, with_shear=True, with_redshifts=True)]
    layouts += [cat.build_trees(edges, closed=closed, with_redshifts=True) for cat in (density, density_rand, shape_rand) if cat is not None]
    for layout in layouts:
        engine.check_proj_redshifts(layout)
    _log_info("computing position-shape correlation from SD, SR" + (", RR" if shape_rand is not None else ""))
    catalogs = [cat for cat in (shapes, density, density_rand, shape_rand) if cat is not None]
    links = PatchLinkage.from_catalogs(config, *catalogs, max_angle=radial_max_angle(config, *layouts))
    kwargs = dict(pi_max=pi_max, pi_bins=pi_edges, progress=progress, max_workers=max_workers)
    SD = links.count_alignment_pairs(shapes, density, count_type_info="SD", **kwargs)
    SR = links.count_alignment_pairs(shapes, density_rand, count_type_info="SR", **kwargs)
    RR = [None] * len(SD) if shape_rand is None else links.count_projected_pairs(density_rand, shape_rand, count_type_info="RR", **kwargs)
    result = []
    for sd, sr, rr in zip(SD, SR, RR):
        bins = [dict(t_sd=d[0], x_sd=d[1], w_sd=d[2], t_sr=r[0], x_sr=r[1], w_sr=r[2]) for d, r in zip(sd, sr)]
        if rr is not None:
            for planes, counts in zip(bins, rr):
                planes["rr"] = counts
        result.append(AlignmentCorrFunc(pi_edges, bins))
    return result


def autocorrelate_alignment(config, shapes: Catalog, shape_rand: Catalog | None = None, *, pi_max: float, pi_bins=None,
                            progress: bool = False, max_workers: int | None = None) -> list:
    """Projected shape-shape correlation of the shape sample ``shapes``: the intrinsic-alignment signals ``w_++(r_p)`` and
    ``w_xx(r_p)`` and the parity-odd null test ``w_+x(r_p)`` -> ``[ShapeShapeCorrFunc]``, one per scale of the configuration
    (no counterpart in the reference). ``cf.sample("plus")`` is ``w_++``, ``cf.sample("cross")`` is
    ``w_xx``, ``cf.sample("plus_cross")`` is ``w_+x``, each with jackknife samples over the patches;
    ``cf.sample_xi(component)`` gives the pi bins.

    Every unordered pair of two shapes is binned in its own radius ``r_p = (d_a + d_b) / 2 * theta`` and in
    ``pi = |chi_a - chi_b| <= pi_max``, and both ellipticities are rotated to the great circle through the pair. One
    library call sums the planes ``S+S+``, ``SxSx``, ``S+Sx`` and the pair weights. With ``shape_rand`` one more call, of
    the count of ``autocorrelate_projected``, gives ``R_S R_S`` and the estimator is ``S+S+ / R_S R_S`` per pi bin, each
    count over its own normalisation; without randoms it is ``S+S+ / W``, the pair-weighted mean product, as
    ``autocorrelate_shear`` reports ``xi_+``. The two differ by the factor ``1 + xi_gg`` of the sample's own clustering.
    ``pi_bins`` is a number of equal bins from 0 to ``pi_max`` or their edges; ``None`` is one bin ``[0, pi_max]``. The
    number of pi bins is capped by the device's LDS (21 at 12 fine bins, 5 at 50); beyond the cap the call is a
    ``ValueError`` that states it.

    ``shapes`` carries ``g1`` / ``g2`` and redshifts, ``shape_rand`` redshifts. Units, ``pi_max``, redshift bins (pairs are
    counted INSIDE a bin), reach and the one-process rule are ``autocorrelate_projected``'s; the catalogues are separate
    ``Catalog`` instances."""
    _require_distinct(shapes, shape_rand)
    if parallel.world()[1] > 1:
        raise NotImplementedError("projected counts run in one process on one device")
    pi_edges = engine.check_pi_edges(1 if pi_bins is None else pi_bins, pi_max)
    engine.radial_kind(config.scales.scales.unit)  # angular units have no radius: ValueError
    edges, closed = config.binning.edges, config.binning.closed
    if not shapes.has_shear:
        raise ValueError("the shape catalogue has no 'g1'/'g2' attached")
    _log_info("building trees")
    layouts = [shapes.build_trees(edges, closed=closed, with_shear=True, with_redshifts=True)]
    if shape_rand is not None:
        layouts.append(shape_rand.build_trees(edges, closed=closed, with_redshifts=True))
    for layout in layouts:
        engine.check_proj_redshifts(layout)
    _log_info("computing shape-shape correlation from SS" + (", RR" if shape_rand is not None else ""))
    catalogs = [cat for cat in (shapes, shape_rand) if cat is not None]
    links = PatchLinkage.from_catalogs(config, *catalogs, max_angle=radial_max_angle(config, *layouts))
    kwargs = dict(pi_max=pi_max, pi_bins=pi_edges, progress=progress, max_workers=max_workers)
    SS = links.count_shape_pairs(shapes, count_type_info="SS", **kwargs)
    RR = [None] * len(SS) if shape_rand is None else links.count_projected_pairs(shape_rand, count_type_info="RR", **kwargs)
    result = []
    for ss, rr in zip(SS, RR):
        bins = [dict(pp=pp, xx=xx, px=px, w=w) for pp, xx, px, w in ss]
        if rr is not None:
            for planes, counts in zip(bins, rr):
                planes["rr"] = counts
        result.append(ShapeShapeCorrFunc(pi_edges, bins))
    return result


def crosscorrelate(config, reference: Catalog, unknown: Catalog, *, ref_rand: Catalog | None = None,
                   unk_rand: Catalog | None = None, progress: bool = False, max_workers: int | None = None) -> list:
    """Angular cross-correlation between redshift slices of ``reference`` and the whole ``unknown``
    sample: DD always, DR / RD / RR depending on the randoms given -> ``[CorrFunc]``, one per scale
    (measurements.py:529-628)."""
    _require_distinct(reference, unknown, ref_rand, unk_rand)
    count_dr, count_rd = unk_rand is not None, ref_rand is not None
    if not count_dr and not count_rd:
        raise ValueError("at least one random dataset must be provided")
    edges, closed = config.binning.edges, config.binning.closed
    randoms = []
    _log_info("building reference data trees")
    reference.build_trees(edges, closed=closed)
    if count_rd:
        ref_rand.build_trees(edges, closed=closed)
        randoms.append(ref_rand)
    unknown.build_trees(None)
    if count_dr:
        unk_rand.build_trees(None)
        randoms.append(unk_rand)
    _log_info("computing cross-correlation from DD" + (", DR" if count_dr else "") + (", RD" if count_rd else "")
              + (", RR" if count_dr and count_rd else ""))
    links = PatchLinkage.from_catalogs(config, reference, unknown, *randoms)
    # the reference issues DD, DR, RD, RR one after the other (measurements.py:617-628); here they are ONE submission
    DD, DR, RD, RR = links.count_pairs_batch(
        [((reference, unknown), "DD"), ((reference, unk_rand), "DR"), ((ref_rand, unknown), "RD"), ((ref_rand, unk_rand), "RR")],
        progress=progress, max_workers=max_workers)
    return [CorrFunc(dd, dr, rd, rr) for dd, dr, rd, rr in zip(DD, DR, RD, RR)]


# ---------------------------------------------------------------------------------------------
# scalar-field (nk / kk) correlations (measurements.py:631-794)
def compute_scalar_normalisation(catalog: Catalog, binning) -> NormalisedScalarCounts:
    """The mean scalar field per patch and redshift bin as a pair-count container: ``[B, P, P]`` tensors whose diagonals
    hold the sum of ``kappa * w`` and the sum of ``w`` of every (patch, bin) tree, zero elsewhere
    (measurements.py:634-648). The sums are taken on the device from the two resident catalogues of the layout
    ``build_trees`` made (``yawhip_catalog_segment_sums``)."""
    num_bins, num_patches = len(binning), catalog.num_patches
    layout = _active_layout(catalog, num_bins)
    if layout.kappa is None:
        raise ValueError("catalog has no 'kappa' attached")
    sums_k, sums_w = engine.scalar_segment_sums(layout)  # [P, B_or_1]
    if layout.num_bins == 1 and num_bins != 1:  # an unbinned catalogue repeats its single tree (trees.py:600-601)
        sums_k, sums_w = np.repeat(sums_k, num_bins, axis=1), np.repeat(sums_w, num_bins, axis=1)
    sum_kappa = np.zeros((num_bins, num_patches, num_patches))
    sum_weights = np.zeros_like(sum_kappa)
    idx = np.arange(num_patches)
    sum_kappa[:, idx, idx] = sums_k.T
    sum_weights[:, idx, idx] = sums_w.T
    return NormalisedScalarCounts(PatchedCounts(binning, sum_kappa, auto=False), PatchedCounts(binning, sum_weights, auto=False))


def autocorrelate_scalar(config, data: Catalog, *, progress: bool = False, max_workers: int | None = None) -> list:
    """Angular autocorrelation amplitude of a scalar field in redshift slices: the "kk" count of ``data`` with itself over
    its "nn" count -> ``[ScalarCorrFunc]``, one per scale (measurements.py:651-705). ``data`` carries kappa and redshifts."""
    edges, closed = config.binning.edges, config.binning.closed
    _log_info("building data trees")
    data.build_trees(edges, closed=closed)
    _log_info("computing auto-correlation with DD")
    links = PatchLinkage.from_catalogs(config, data)
    DD = links.count_scalar_pairs(data, mode="kk", progress=progress, max_workers=max_workers, count_type_info="DD")
    return [ScalarCorrFunc(dd) for dd in DD]


def crosscorrelate_scalar(config, reference: Catalog, unknown: Catalog, *, unk_rand: Catalog | None = None,
                          progress: bool = False, max_workers: int | None = None) -> list:
    """Angular cross-correlation amplitude between the scalar field carried by ``reference`` (with redshifts) and the
    ``unknown`` sample: "kn" DD, minus the same count against ``unk_rand`` when it is given, else minus the mean field per
    patch (``compute_scalar_normalisation``) -> ``[ScalarCorrFunc]``, one per scale (measurements.py:708-794)."""
    return _crosscorrelate_scalar(config, reference, unknown, unk_rand, "kn", progress, max_workers)


def _crosscorrelate_scalar(config, reference, other, rand, mode: str, progress, max_workers) -> list:
    """The two scalar cross-correlation drivers: ``reference`` is binned in redshift, ``other`` is not. ``mode`` "kn": the
    field rides on the reference and ``rand`` stands in for ``other``; "nk": the field rides on ``other`` (a map) and ``rand``
    stands in for the reference. Without ``rand`` the mean field per patch of the side that carries it takes DR's place."""
    _require_distinct(reference, other, rand)
    count_dr, field_on_reference = rand is not None, mode == "kn"
    edges, closed = config.binning.edges, config.binning.closed
    randoms = []
    _log_info("building reference data trees")
    reference.build_trees(edges, closed=closed)
    other.build_trees(None)
    if count_dr:
        if field_on_reference:
            rand.build_trees(None)
        else:
            rand.build_trees(edges, closed=closed)
        randoms.append(rand)
    _log_info("computing cross-correlation with DD" + (", DR" if count_dr else ""))
    links = PatchLinkage.from_catalogs(config, reference, other, *randoms)
    kwargs = dict(progress=progress, max_workers=max_workers)
    if count_dr:  # the reference counts DD (kn), DD (nn), DR (kn), DR (nn) one after the other; here they are ONE submission
        dr = (reference, rand) if field_on_reference else (rand, other)
        DD, DR = links._count_scalar_batch([((reference, other), "DD"), (dr, "DR")], mode, **kwargs)
    else:
        DD = links.count_scalar_pairs(reference, other, mode=mode, count_type_info="DD", **kwargs)
        DR = [compute_scalar_normalisation(reference if field_on_reference else other, config.binning.binning)] * len(DD)
    return [ScalarCorrFunc(dd, dr) for dd, dr in zip(DD, DR)]


def crosscorrelate_scalar_map(config, reference: Catalog, scalar_map: Catalog, *, ref_rand: Catalog | None = None,
                              progress: bool = False, max_workers: int | None = None) -> list:
    """Angular cross-correlation amplitude between redshift slices of ``reference`` and a scalar field WITHOUT redshifts,
    typically a map (``Catalog.from_healpix_map``): the "nk" DD count of ``reference`` against ``scalar_map``, minus the same
    count of ``ref_rand`` against the map when it is given, else minus the map's mean field per patch
    (``compute_scalar_normalisation``) -> ``[ScalarCorrFunc]``, one per scale.

    This driver has no counterpart in the reference. The reference's ``crosscorrelate_scalar`` takes the scalar field from
    the catalogue that carries the redshifts ("kn": the field is binned with its own objects); a map has no redshifts, so
    it can only be the unbinned side of the count, and the count that fits, "nk", is one the reference's drivers never
    issue. The pieces are the reference's all the same: the "nk" mode of its pair counts, ``NormalisedScalarCounts`` and
    ``ScalarCorrFunc``."""
    return _crosscorrelate_scalar(config, reference, scalar_map, ref_rand, "nk", progress, max_workers)


def crosscorrelate_shear(config, reference: Catalog, sources: Catalog, *, ref_rand: Catalog | None = None,
                         radius: str = "slice", progress: bool = False, max_workers: int | None = None) -> list:
    """Tangential shear of ``sources`` (a catalogue with ``g1`` / ``g2``, no redshifts needed) around ``reference`` in its
    redshift slices, and the cross shear as its null test: per redshift bin and scale ``gamma_t = sum T / sum W`` over the
    pairs in range, minus the same ratio around the lenses of ``ref_rand`` when it is given (``gamma_x`` alike) ->
    ``[(ScalarCorrFunc(dd_t, dr_t), ScalarCorrFunc(dd_x, dr_x)), ...]``, one pair per scale, ``dr = None`` without randoms.
    A pair adds ``T = w_l w_s * -(g1 cos 2phi + g2 sin 2phi)`` and ``X = w_l w_s * (g1 sin 2phi - g2 cos 2phi)``, ``phi`` the
    position angle of the lens seen from the source, from east towards north (frame of ``g1, g2``: ``Catalog.from_arrays``).

    With physical or comoving scales, ``radius="slice"`` (the default) turns the limits into an angle once per redshift
    slice, at its middle; ``radius="lens"`` bins every pair by ``R = D(z_l) theta`` of its OWN lens (the references then need
    redshifts; angular scales are a ``ValueError``), as ``crosscorrelate_delta_sigma`` describes.

    This driver has no counterpart in the reference. Linkage, scales, patches and jackknife are ``crosscorrelate``'s; the
    count runs on one device of one process."""
    _require_distinct(reference, sources, ref_rand)
    if not sources.has_shear:
        raise ValueError("catalog has no 'g1'/'g2' attached")
    return _crosscorrelate_lensing(config, reference, sources, ref_rand, radius, progress, max_workers, delta_sigma=False)


def _crosscorrelate_lensing(config, reference, sources, ref_rand, radius, progress, max_workers, *, delta_sigma: bool):
    """What ``crosscorrelate_shear`` and ``crosscorrelate_delta_sigma`` (``delta_sigma``: every layout carries redshifts) share
    after their own argument checks: the layouts, the linkage -- as far as the nearest lens sees the largest radius for
    ``radius="lens"`` -- and DD with the optional DR. Returns the result list of ``crosscorrelate_shear``."""
    per_lens = _per_lens(config, radius)
    edges, closed = config.binning.edges, config.binning.closed
    lens_redshifts = delta_sigma or per_lens
    randoms = []
    _log_info("building reference data trees")
    lens_layouts = [reference.build_trees(edges, closed=closed, with_redshifts=lens_redshifts)]
    if ref_rand is not None:
        lens_layouts.append(ref_rand.build_trees(edges, closed=closed, with_redshifts=lens_redshifts))
        randoms.append(ref_rand)
    if delta_sigma:
        sources.build_trees(None, with_redshifts=True)
    else:
        sources.build_trees(None)
    _log_info(("computing excess surface density" if delta_sigma else "computing shear cross-correlation") + " with DD"
              + (", DR" if randoms else ""))
    kwargs = dict(progress=progress, max_workers=max_workers)
    if per_lens:
        links = PatchLinkage.from_catalogs(config, reference, sources, *randoms, max_angle=radial_max_angle(config, *lens_layouts))
        count = functools.partial(links.count_dsigma_radial_pairs, shear_only=not delta_sigma)
    else:
        links = PatchLinkage.from_catalogs(config, reference, sources, *randoms)
        count = links.count_dsigma_pairs if delta_sigma else links.count_shear_pairs
    DD = count(reference, sources, count_type_info="DD", **kwargs)
    DR = count(ref_rand, sources, count_type_info="DR", **kwargs) if randoms else [(None, None)] * len(DD)
    return [(ScalarCorrFunc(dd_t, dr_t), ScalarCorrFunc(dd_x, dr_x)) for (dd_t, dd_x), (dr_t, dr_x) in zip(DD, DR)]


def _per_lens(config, radius: str) -> bool:
    """``radius`` of the two lensing drivers: "slice" (False) or "lens" (True; the scales must not be angular)."""
    if radius not in ("slice", "lens"):
        raise ValueError(f"radius must be 'slice' or 'lens', not {radius!r}")
    if radius == "lens":
        engine.radial_kind(config.scales.scales.unit)
    return radius == "lens"


def crosscorrelate_delta_sigma(config, reference: Catalog, sources: Catalog, *, ref_rand: Catalog | None = None,
                               boost: bool = False, radius: str = "slice", progress: bool = False,
                               max_workers: int | None = None) -> list:
    """Excess surface density of the matter around ``reference`` in its redshift slices, from ``sources`` with ``g1`` / ``g2``
    and point redshifts: per redshift bin and scale

        Delta Sigma (R) = sum_ls w_l w_s Sigma_c^-1 gamma_t / sum_ls w_l w_s Sigma_c^-2      in M_sun / pc^2 (physical),

    ``Sigma_c^-1 (z_l, z_s) = (4 pi G / c^2) D_A(z_l) max(0, 1 - chi_l / chi_s)`` evaluated per PAIR from the two redshifts
    with the configuration's cosmology, which is assumed flat (a custom one is used as given): a source in front of its lens
    adds nothing. The cross component is the null test. Minus the same ratio around the lenses of ``ref_rand`` when it is
    given -> ``[(ScalarCorrFunc(dd_t, dr_t), ScalarCorrFunc(dd_x, dr_x)), ...]``, one tuple per scale, ``dr = None`` without
    randoms: the shape of ``crosscorrelate_shear``, whose frame and rotation these are. With physical or comoving scales
    (``unit="kpc"``) ``radius`` says how a pair finds its bin. ``"slice"`` (the default) turns the limits into an angle once per
    redshift slice, at its middle, as the clustering counts do: a lens at the near end of a wide slice is then counted at a
    radius other than the bin names. ``"lens"`` bins every pair by ``R = D(z_l) theta`` of its OWN lens -- ``D = D_A`` for
    ``kpc`` / ``Mpc``, ``D_A (1 + z_l)`` for ``kpc/h`` / ``Mpc/h`` --, the same radii in every slice; the linkage then reaches
    as far as the nearest lens (or random lens) sees the largest radius, at most 5.73 degrees (a ``ValueError`` that names
    the lens's redshift beyond that), and angular scales are a ``ValueError``.

    ``boost=True`` (needs ``ref_rand``) adds a third item per scale, a plain ``CorrFunc(dd, dr)`` whose counts are the
    denominators ``sum w_l w_s Sigma_c^-2`` of DD and DR, already counted, each normalised by the lens weight sums per
    (patch, bin) times the sources' patch totals as ``crosscorrelate`` normalises its counts: ``cf_boost.sample()`` is the
    boost factor minus one, ``B(R) - 1``, with its jackknife samples -- the excess of sources around real lenses over random
    ones, i.e. the dilution of the signal by sources that belong to the lens.

    This driver has no counterpart in the reference. Linkage, scales, patches and jackknife are ``crosscorrelate``'s; the
    count runs on one device of one process."""
    _require_distinct(reference, sources, ref_rand)
    if not sources.has_shear:
        raise ValueError("catalog has no 'g1'/'g2' attached")
    if not sources.has_redshifts:
        raise ValueError("excess surface density needs source redshifts: the sources have no 'redshifts' attached")
    if boost and ref_rand is None:
        raise ValueError("the boost factor needs random lenses: give 'ref_rand'")
    result = _crosscorrelate_lensing(config, reference, sources, ref_rand, radius, progress, max_workers, delta_sigma=True)
    if boost:  # the W planes of the two counts over the products of the weight sums: (DD - DR) / DR
        binning, num_bins = config.binning.binning, len(config.binning.binning)
        source_layout = _active_layout(sources, num_bins)  # (the layouts the counts ran on)
        norms = [PatchedSumWeights(binning, _active_layout(lenses, num_bins).sum_weights_for(num_bins),
                                   source_layout.sum_weights_for(num_bins), auto=False)
                 for lenses in (reference, ref_rand)]
        result = [(cf_t, cf_x, CorrFunc(NormalisedCounts(cf_t.dd.number_counts, norms[0]), NormalisedCounts(cf_t.dr.number_counts, norms[1])))
                  for cf_t, cf_x in result]
    return result


def autocorrelate_shear(config, sources: Catalog, *, linkage: PatchLinkage | None = None, progress: bool = False,
                        max_workers: int | None = None) -> list:
    """Shear-shear correlations of ``sources`` (a catalogue with ``g1`` / ``g2`` and redshifts) inside the redshift bins of
    the configuration: per bin and scale ``xi_plus = sum P / sum W``, ``xi_minus = sum M / sum W`` and the parity-odd
    ``xi_cross = sum C / sum W`` (a null test) over the pairs in range ->
    ``[(ScalarCorrFunc(dd_plus), ScalarCorrFunc(dd_minus), ScalarCorrFunc(dd_cross)), ...]``, one triple per scale. With
    ``(t, x)`` the shear of an object along and across the great circle that joins the pair -- each end rotated by its own
    position angle, since the east / north frames (``Catalog.from_arrays``) at the two ends are not parallel on the sphere --
    a pair adds ``P = w_a w_b (t_a t_b + x_a x_b)``, ``M = w_a w_b (t_a t_b - x_a x_b)``, ``C = w_a w_b (t_a x_b + x_a t_b)``
    and ``W = w_a w_b`` (include/yawhip.h has the arithmetic).

    This driver has no counterpart in the reference. Patches, scales and jackknife are ``autocorrelate``'s; ``linkage`` may
    pass a prepared ``PatchLinkage``; the count runs on one device of one process."""
    if not sources.has_shear:
        raise ValueError("catalog has no 'g1'/'g2' attached")
    _log_info("building source trees")
    sources.build_trees(config.binning.edges, closed=config.binning.closed, with_shear=True)
    _log_info("computing shear auto-correlation with DD")
    links = linkage if linkage is not None else PatchLinkage.from_catalogs(config, sources)
    DD = links.count_shear_auto_pairs(sources, count_type_info="DD", progress=progress, max_workers=max_workers)
    return [tuple(ScalarCorrFunc(dd) for dd in triple) for triple in DD]


def correlate_shear_tomographic(config, sources: Catalog, sources2: Catalog | None = None, *, bin_pairs=None,
                                linkage: PatchLinkage | None = None, progress: bool = False,
                                max_workers: int | None = None) -> list:
    """The tomographic matrix of shear-shear correlations: ``xi_plus^{ij}``, ``xi_minus^{ij}`` and the parity-odd
    ``xi_cross^{ij}`` between redshift bin ``i`` of ``sources`` and bin ``j`` of ``sources2`` -- another shape sample, another
    survey, the other half of a null test -- or, without ``sources2``, between the bins of ``sources`` itself. Both are
    catalogues with ``g1`` / ``g2`` and redshifts; the pair term is ``autocorrelate_shear``'s. Returns, per scale, a list of
    ``B`` rows; row ``i`` is ``(ScalarCorrFunc(dd_plus), ScalarCorrFunc(dd_minus), ScalarCorrFunc(dd_cross))`` on the
    configuration's binning, whose bins run over ``j``.

    ``bin_pairs=[(i, j), ...]`` restricts the pairs: the default is every ``i <= j`` of one catalogue (``i > j`` is refused:
    it is the same signal) and all ``B * B`` ordered pairs of two. Slots not asked for hold zero counts and sample to NaN. For
    one catalogue slot ``(i, i)`` holds exactly what ``autocorrelate_shear`` stores for bin ``i``, and slot ``j < i`` of row
    ``i`` mirrors slot ``i`` of row ``j`` with the patch axes transposed.

    Scales: the pairs of ``(i, j)`` are binned with the limits of bin ``min(i, j)``. For angular units every bin has the same
    limits; for physical units this is a convention -- the scale is turned into an angle at the middle of the nearer bin.

    This driver has no counterpart in the reference and needs no randoms. Patches, scales and jackknife are
    ``autocorrelate``'s (``crosscorrelate``'s checks for two catalogues: distinct objects, consistent patches); ``linkage``
    may pass a prepared ``PatchLinkage``; the count runs on one device of one process."""
    catalogs = (sources,) if sources2 is None else (sources, sources2)
    _require_distinct(*catalogs)
    if not all(cat.has_shear for cat in catalogs):
        raise ValueError("catalog has no 'g1'/'g2' attached")
    _log_info("building source trees")
    for cat in catalogs:
        cat.build_trees(config.binning.edges, closed=config.binning.closed, with_shear=True)
    _log_info("computing tomographic shear correlation with DD")
    links = linkage if linkage is not None else PatchLinkage.from_catalogs(config, *catalogs)
    DD = links.count_shear_tomographic_pairs(sources, sources2, bin_pairs=bin_pairs, count_type_info="DD", progress=progress,
                                             max_workers=max_workers)
    return [[tuple(ScalarCorrFunc(dd) for dd in triple) for triple in rows] for rows in DD]
