#!/usr/bin/env python3
"""Timing probe (not a test): the shear count against the weighted pair count of the same catalogues and jobs.

One input: lenses with redshifts in ``--bins`` slices and weighted sources with a random shear, uniform in a box of
``--box`` degrees cut into ``--patches`` patches (a square grid of centres); one scale ``--rmin`` .. ``--rmax`` arcmin with
``--fine`` fine bins (50 is the default ``rweight`` resolution). On the linkage's job list:

* ``shear``  ``engine.count_shear_fine`` (``yawhip_shear_count``, kernel ``k_count_shear``);
* ``exact``  ``engine.count_fine(kernel="exact")`` of the same layouts and jobs: the plain float64 path the shear kernel is
             modelled on -- the same hot loop, without the per-tile key window (it streams every lens segment whole) and
             without the projection of the pairs in range.

Each is run once to warm up, then ``--repeat`` times; the medians of the device time (``CountStats.kernel_ms``) and of the host
wall time around the blocking call are reported with the pair separations each evaluated, so that the rate per evaluated
pair can be compared as well as the time. Prints one JSON line and appends it to ``--out`` (profiles/shear_probe.jsonl holds
the committed run, if there is one).

Usage:  python tools/probe_shear.py --lenses 4e5 --sources 2e6 --patches 64
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

import yet_another_wizz_amd as yaw  # noqa: E402
from yet_another_wizz_amd import _lib, engine  # noqa: E402
from yet_another_wizz_amd.build import source_sha16  # noqa: E402


def timed(call, repeat):
    call()  # warm-up (uploads, code objects)
    wall, device, stats = [], [], None
    for _ in range(repeat):
        t0 = time.perf_counter()
        *_, stats = call()
        wall.append(1e3 * (time.perf_counter() - t0))
        device.append(stats.kernel_ms)
    return statistics.median(wall), statistics.median(device), stats


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--lenses", default="4e5")
    ap.add_argument("--sources", default="2e6")
    ap.add_argument("--patches", type=int, default=64, help="a square number")
    ap.add_argument("--bins", type=int, default=4)
    ap.add_argument("--box", type=float, default=10.0)
    ap.add_argument("--rmin", type=float, default=0.5)
    ap.add_argument("--rmax", type=float, default=10.0)
    ap.add_argument("--fine", type=int, default=50)
    ap.add_argument("--repeat", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "shear_probe.jsonl"))
    args = ap.parse_args()
    if _lib.device_count() < 1:
        raise SystemExit("no GPU: nothing to time")
    n_lens, n_src = int(float(args.lenses)), int(float(args.sources))
    side = int(round(np.sqrt(args.patches)))
    if side * side != args.patches:
        raise SystemExit("--patches must be a square number")
    rng = np.random.default_rng(1)
    grid = (np.arange(side) + 0.5) * args.box / side
    centers = yaw.AngularCoordinates(np.deg2rad([[10.0 + a, -0.5 * args.box + b] for a in grid for b in grid]))

    def positions(n):
        return rng.uniform(10.0, 10.0 + args.box, n), rng.uniform(-0.5 * args.box, 0.5 * args.box, n)

    lenses = yaw.Catalog.from_arrays(*positions(n_lens), redshifts=rng.uniform(0.1, 0.9, n_lens), weights=rng.uniform(0.5, 1.5, n_lens),
                                     patch_centers=centers)
    sources = yaw.Catalog.from_arrays(*positions(n_src), weights=rng.uniform(0.5, 1.5, n_src), g1=rng.normal(0, 0.3, n_src),
                                      g2=rng.normal(0, 0.3, n_src), patch_centers=centers)
    config = yaw.Configuration.create(rmin=args.rmin, rmax=args.rmax, unit="arcmin", rweight=0.0, resolution=args.fine,
                                      zmin=0.1, zmax=0.9, num_bins=args.bins)
    lens_layout = lenses.build_trees(config.binning.edges, closed=config.binning.closed)
    source_layout = sources.build_trees(None)
    links = yaw.PatchLinkage.from_catalogs(config, lenses, sources)
    jobs = links.get_patch_pairs(lenses, sources)
    _, thresholds = links._angular_setup()
    axis = links.sort_axis
    shear_wall, shear_dev, shear_stats = timed(
        lambda: engine.count_shear_fine(lens_layout, source_layout, jobs, thresholds, sort_axis=axis), args.repeat)
    exact_wall, exact_dev, exact_stats = timed(
        lambda: engine.count_fine(lens_layout, source_layout, jobs, thresholds, kernel="exact", sort_axis=axis), args.repeat)
    T, X, W, _ = engine.count_shear_fine(lens_layout, source_layout, jobs, thresholds, sort_axis=axis)
    sums, _ = engine.count_fine(lens_layout, source_layout, jobs, thresholds, kernel="exact", sort_axis=axis)
    line = dict(lenses=n_lens, sources=n_src, patches=args.patches, bins=args.bins, jobs=int(len(jobs)), fine_bins=int(thresholds.shape[1] - 1),
                rmin_arcmin=args.rmin, rmax_arcmin=args.rmax, sort_axis=int(axis), candidate_pairs=int(shear_stats.candidate_pairs),
                shear_evaluated=int(shear_stats.evaluated_pairs), exact_evaluated=int(exact_stats.evaluated_pairs),
                shear_kernel_ms=round(shear_dev, 3), exact_kernel_ms=round(exact_dev, 3),
                shear_wall_ms=round(shear_wall, 3), exact_wall_ms=round(exact_wall, 3),
                kernel_ratio=round(shear_dev / exact_dev, 3),
                shear_ps_per_evaluated=round(1e9 * shear_dev / max(shear_stats.evaluated_pairs, 1), 3),
                exact_ps_per_evaluated=round(1e9 * exact_dev / max(exact_stats.evaluated_pairs, 1), 3),
                weight_in_range=float(W.sum()), w_max_rel_diff=float(np.max(np.abs(W - sums) / np.maximum(np.abs(sums), 1e-300))),
                exact_variant=sorted(exact_stats.variants), repeat=args.repeat, source_sha16=source_sha16())
    text = json.dumps(line)
    print(text, flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "a") as f:
        f.write(text + "\n")


if __name__ == "__main__":
    main()
