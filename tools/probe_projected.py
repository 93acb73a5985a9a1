#!/usr/bin/env python3
"""Timing probe (not a test): the projected pair count of one catalogue inside its redshift bins.

One input, that of tools/probe_shear_auto.py with radii in the place of angles: weighted objects with redshifts uniform in
0.1 < z < 0.9 in ``--bins`` slices, uniform in a box of ``--box`` degrees cut into ``--patches`` patches (a square grid of
centres); one scale ``--rmin`` .. ``--rmax`` kpc with ``--fine`` fine bins, and the line-of-sight cut ``--pi-max`` Mpc. The
default ``--rmax`` is what the nearest object of the catalogue (z = 0.1) sees under 10 arcmin, the reach of the 0.5' - 10'
run of tools/probe_shear_auto.py; the windows of the farther redshift bins are narrower than that.

* draws the scene and runs ``engine.count_projected_fine`` (``yawhip_proj_count``, kernel ``k_count_projected``) on the ``i <= j``
  job list of the linkage that reaches as far as the nearest object sees ``--rmax``, bin ``k`` with bin ``k``: once to warm up,
  then ``--repeat`` times (the median and the min - max spread of the device time between the call's two events,
  ``CountStats.kernel_ms``);
* checks ``--check`` of the cells -- the smallest diagonal and off-diagonal ones that hold pairs -- against the numpy brute force
  of tests/proj_oracle.py: ``|ours - oracle| <= 1e-10 A`` per fine bin, ``A`` the sum of ``|w_a w_b|`` of its pairs;
* prints one JSON line (device ms, candidates, evaluated, ps per evaluated separation) and appends it to ``--out``
  (profiles/projected_probe.jsonl holds the committed runs), with the word of ``--label`` if one is given.

``--pi-bins N`` times the pi-binned count instead (``engine.count_projected_pi_fine``, ``yawhip_proj_count_pi``, kernel
``k_count_projected_pi``) on the same input, with ``N`` equal bins from 0 to ``--pi-max``, checks the same
cells against tests/proj_pi_oracle.py in every pi bin, and adds to its line ``pi_bins``, the dynamic LDS of a workgroup
(the formula of include/yawhip.h) and the workgroups of 256 threads that this LDS lets one CU hold (160 KiB per CU). More
pi bins than that LDS formula admits at ``--fine`` is the library's refusal, passed on.

``--mu-bins N`` times the redshift-space count (``engine.count_smu_fine``, ``yawhip_proj_count_smu``, kernel ``k_count_smu``;
DESIGN.md section 23) on the same input with the radii read as ``s`` and ``N`` equal bins of mu in [0, 1] -- there is no
line-of-sight cut, ``--pi-max`` is not used -- checks the same cells against tests/smu_oracle.py in every mu bin, and adds
``mu_bins`` and the same LDS figures to its line.

The evaluated separations of a diagonal cell count one order of every pair (include/yawhip.h), where ``k_count_shear_auto``
also reports the other order inside a lane tile's own range: per diagonal tile of 256 lanes that is 32 640 separations which
this figure leaves out and that one has.

Usage:  python tools/probe_projected.py --objects 2e6 --patches 64
"""
from __future__ import annotations

import argparse
import json
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import yet_another_wizz_amd as yaw  # noqa: E402
from yet_another_wizz_amd import _lib, engine, measurements  # noqa: E402
from yet_another_wizz_amd.build import source_sha16  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--objects", default="2e6")
    ap.add_argument("--patches", type=int, default=64, help="a square number")
    ap.add_argument("--bins", type=int, default=4)
    ap.add_argument("--box", type=float, default=10.0)
    ap.add_argument("--rmin", type=float, default=50.0, help="kpc")
    ap.add_argument("--rmax", type=float, default=None, help="kpc (default: 10 arcmin at z = 0.1)")
    ap.add_argument("--pi-max", type=float, default=60.0, help="Mpc")
    ap.add_argument("--fine", type=int, default=50)
    ap.add_argument("--pi-bins", type=int, default=None, help="time yawhip_proj_count_pi with this many equal pi bins")
    ap.add_argument("--mu-bins", type=int, default=None, help="time yawhip_proj_count_smu with this many equal mu bins")
    ap.add_argument("--repeat", type=int, default=5)
    ap.add_argument("--check", type=int, default=4, help="cells compared with the oracle")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "projected_probe.jsonl"))
    ap.add_argument("--label", default=None, help="a word for the line's \"label\" key, e.g. which tree this run times")
    args = ap.parse_args()
    if _lib.device_count() < 1:
        raise SystemExit("no GPU: nothing to time")
    import proj_oracle

    n = int(float(args.objects))
    side = int(round(np.sqrt(args.patches)))
    if side * side != args.patches:
        raise SystemExit("--patches must be a square number")
    cosmology = yaw.Configuration.create(rmin=1.0, rmax=2.0, unit="kpc", zmin=0.1, zmax=0.9, num_bins=1).cosmology
    rmax = args.rmax if args.rmax is not None else round(1e3 * np.deg2rad(10.0 / 60.0) * float(cosmology.angular_diameter_distance(0.1)), 1)
    rng = np.random.default_rng(1)
    grid = (np.arange(side) + 0.5) * args.box / side
    centers = yaw.AngularCoordinates(np.deg2rad([[10.0 + a, -0.5 * args.box + b] for a in grid for b in grid]))
    catalog = yaw.Catalog.from_arrays(rng.uniform(10.0, 10.0 + args.box, n), rng.uniform(-0.5 * args.box, 0.5 * args.box, n),
                                      redshifts=rng.uniform(0.1, 0.9, n), weights=rng.uniform(0.5, 1.5, n), patch_centers=centers)
    config = yaw.Configuration.create(rmin=args.rmin, rmax=rmax, unit="kpc", rweight=0.0, resolution=args.fine,
                                      zmin=0.1, zmax=0.9, num_bins=args.bins)
    unit = config.scales.scales.unit
    layout = catalog.build_trees(config.binning.edges, closed=config.binning.closed, with_redshifts=True)
    max_angle = measurements.radial_max_angle(config, layout)
    links = yaw.PatchLinkage.from_catalogs(config, catalog, max_angle=max_angle)
    jobs = links.get_patch_pairs(catalog)
    r2 = measurements.threshold_table(measurements.radial_plans(config))
    nb = args.bins
    seg1 = (jobs[:, :1].astype(np.int64) * nb + np.arange(nb)).ravel()
    seg2 = (jobs[:, 1:].astype(np.int64) * nb + np.arange(nb)).ravel()
    cells = np.column_stack([seg1, seg2, np.tile(np.arange(nb), len(jobs)), seg1 == seg2]).astype(np.int32)

    if args.pi_bins is not None and args.mu_bins is not None:
        raise SystemExit("--pi-bins and --mu-bins are two counts: one at a time")
    pi_edges = None if args.pi_bins is None else engine.check_pi_edges(args.pi_bins, args.pi_max)
    mu_edges = None if args.mu_bins is None else engine.check_mu_edges(args.mu_bins)
    planes = pi_edges if pi_edges is not None else mu_edges  # the edges of a count with planes, else None

    def call():
        if mu_edges is not None:
            return engine.count_smu_fine(layout, layout, cells, r2, mu_edges=mu_edges, cosmology=config.cosmology, unit=unit,
                                         sort_axis=links.sort_axis)
        if pi_edges is not None:
            return engine.count_projected_pi_fine(layout, layout, cells, r2, pi_edges=pi_edges, cosmology=config.cosmology, unit=unit,
                                                  sort_axis=links.sort_axis)
        return engine.count_projected_fine(layout, layout, cells, r2, pi_max=args.pi_max, cosmology=config.cosmology, unit=unit,
                                           sort_axis=links.sort_axis)

    call()  # warm-up (uploads, code objects)
    wall, device = [], []
    for _ in range(args.repeat):
        t0 = time.perf_counter()
        W, stats = call()
        wall.append(1e3 * (time.perf_counter() - t0))
        device.append(stats.kernel_ms)

    # the smallest cells of each kind that hold pairs, against the brute force
    handle = proj_oracle.as_handle(layout, *engine.proj_columns(layout, config.cosmology, unit))
    sizes = np.diff(layout.offsets)
    cost = sizes[cells[:, 0]].astype(np.float64) * sizes[cells[:, 1]]
    holds = W.sum(axis=-1).sum(axis=0) > 0 if planes is not None else W.sum(axis=1) > 0
    checked, worst = [], 0.0
    for diagonal in (1, 0):
        of_kind = np.flatnonzero((cells[:, 3] == diagonal) & holds)
        checked += list(of_kind[np.argsort(cost[of_kind], kind="stable")][: (args.check + diagonal) // 2])
    if checked:
        if mu_edges is not None:
            import smu_oracle

            exp_w, exp_a, _ = smu_oracle.smu_cells(handle, handle, cells[checked], r2, mu_edges * mu_edges)
            differs = np.abs(W[:, checked] - exp_w)
        elif pi_edges is not None:
            import proj_pi_oracle

            exp_w, exp_a, _ = proj_pi_oracle.proj_pi_cells(handle, handle, cells[checked], r2, pi_edges)
            differs = np.abs(W[:, checked] - exp_w)
        else:
            exp_w, exp_a, _ = proj_oracle.proj_cells(handle, handle, cells[checked], r2, args.pi_max)
            differs = np.abs(W[checked] - exp_w)
        if not np.all(differs <= 1e-10 * exp_a):
            raise SystemExit(f"cells {checked} differ from the oracle by up to {np.max(differs / np.maximum(exp_a, 1e-300)):.3e} A")
        worst = float(np.max(differs[exp_a > 0] / exp_a[exp_a > 0]))
    median = statistics.median(device)
    line = dict(**({"label": args.label} if args.label else {}), objects=n, patches=args.patches, bins=nb, jobs=int(len(jobs)), cells=int(len(cells)), fine_bins=int(r2.shape[1] - 1),
                rmin_kpc=args.rmin, rmax_kpc=rmax, pi_max_mpc=args.pi_max, max_angle_arcmin=round(float(np.rad2deg(max_angle)) * 60.0, 3),
                sort_axis=int(links.sort_axis), candidate_pairs=int(stats.candidate_pairs), evaluated=int(stats.evaluated_pairs),
                kernel_ms=round(median, 3), kernel_ms_spread=[round(min(device), 3), round(max(device), 3)],
                wall_ms=round(statistics.median(wall), 3), ps_per_evaluated=round(1e9 * median / max(stats.evaluated_pairs, 1), 3),
                weight_in_range=float(W.sum()), cells_with_pairs=int(np.count_nonzero(holds)), cells_checked=[int(c) for c in checked],
                worst_difference_over_A=worst, repeat=args.repeat, source_sha16=source_sha16())
    if planes is not None:
        n_edges, n_pi = int(r2.shape[1]), len(planes) - 1
        lds = 2 * 256 * 48 + 8 * (((n_edges + 1) & ~1) + ((n_pi + 2) & ~1)) + 4 * n_pi * (n_edges - 1) * 8
        line.update(dict(pi_bins=n_pi, kernel="k_count_projected_pi") if pi_edges is not None else dict(mu_bins=n_pi, kernel="k_count_smu"),
                    lds_bytes_per_workgroup=lds, workgroups_per_cu_by_lds=(160 * 1024) // lds)
    if mu_edges is not None:
        del line["pi_max_mpc"]  # no cut
    text = json.dumps(line)
    print(text, flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "a") as f:
        f.write(text + "\n")


if __name__ == "__main__":
    main()
