#!/usr/bin/env python3
"""Timing probe (not a test): the shear-shear count against the tangential-shear count on the same objects.

One input: weighted sources with a random shear and redshifts in ``--bins`` slices, uniform in a box of ``--box`` degrees cut
into ``--patches`` patches (a square grid of centres); one scale ``--rmin`` .. ``--rmax`` arcmin with ``--fine`` fine bins (50 is
the default ``rweight`` resolution).

* ``auto``   ``engine.count_shear_auto_fine`` (``yawhip_shear_auto_count``, kernel ``k_count_shear_auto``) on the binned layout with
             shear and the ``i <= j`` job list of the linkage;
* ``cross``  ``engine.count_shear_fine`` (``yawhip_shear_count``, kernel ``k_count_shear``) with the same objects as lenses (the
             binned layout) and as sources (the unbinned layout), on the linkage's ordered job list: the kernel the new one is
             modelled on -- the same streaming loop with a 32-byte instead of a 48-byte LDS object, one rotation instead of two.

Each is run once to warm up, then ``--repeat`` times; the medians of the device time (``CountStats.kernel_ms``, events around the
kernel) and of the host wall time around the blocking call are reported with the pair separations each evaluated, so that the
time per evaluated separation can be compared. Prints one JSON line and appends it to ``--out``
(profiles/shear_auto_probe.jsonl holds the committed runs).

Usage:  python tools/probe_shear_auto.py --sources 2e6 --patches 64 --rmax 10
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
    wall, device, out = [], [], None
    for _ in range(repeat):
        t0 = time.perf_counter()
        out = call()
        wall.append(1e3 * (time.perf_counter() - t0))
        device.append(out[-1].kernel_ms)
    return statistics.median(wall), statistics.median(device), out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sources", default="2e6")
    ap.add_argument("--patches", type=int, default=64, help="a square number")
    ap.add_argument("--bins", type=int, default=4)
    ap.add_argument("--box", type=float, default=10.0)
    ap.add_argument("--rmin", type=float, default=0.5)
    ap.add_argument("--rmax", type=float, default=10.0)
    ap.add_argument("--fine", type=int, default=50)
    ap.add_argument("--repeat", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "shear_auto_probe.jsonl"))
    args = ap.parse_args()
    if _lib.device_count() < 1:
        raise SystemExit("no GPU: nothing to time")
    n = int(float(args.sources))
    side = int(round(np.sqrt(args.patches)))
    if side * side != args.patches:
        raise SystemExit("--patches must be a square number")
    rng = np.random.default_rng(1)
    grid = (np.arange(side) + 0.5) * args.box / side
    centers = yaw.AngularCoordinates(np.deg2rad([[10.0 + a, -0.5 * args.box + b] for a in grid for b in grid]))
    sources = yaw.Catalog.from_arrays(rng.uniform(10.0, 10.0 + args.box, n), rng.uniform(-0.5 * args.box, 0.5 * args.box, n),
                                      redshifts=rng.uniform(0.1, 0.9, n), weights=rng.uniform(0.5, 1.5, n),
                                      g1=rng.normal(0, 0.3, n), g2=rng.normal(0, 0.3, n), patch_centers=centers)
    config = yaw.Configuration.create(rmin=args.rmin, rmax=args.rmax, unit="arcmin", rweight=0.0, resolution=args.fine,
                                      zmin=0.1, zmax=0.9, num_bins=args.bins)
    unbinned = sources.build_trees(None)
    binned = sources.build_trees(config.binning.edges, closed=config.binning.closed, with_shear=True)
    links = yaw.PatchLinkage.from_catalogs(config, sources)
    auto_jobs = links.get_patch_pairs(sources)
    cross_jobs = links.get_patch_pairs(sources, sources)
    _, thresholds = links._angular_setup()
    axis = links.sort_axis
    auto_wall, auto_dev, (P, M, C, W, auto_stats) = timed(
        lambda: engine.count_shear_auto_fine(binned, auto_jobs, thresholds, sort_axis=axis), args.repeat)
    cross_wall, cross_dev, (_, _, W_cross, cross_stats) = timed(
        lambda: engine.count_shear_fine(binned, unbinned, cross_jobs, thresholds, sort_axis=axis), args.repeat)
    auto_ps = 1e9 * auto_dev / max(auto_stats.evaluated_pairs, 1)
    cross_ps = 1e9 * cross_dev / max(cross_stats.evaluated_pairs, 1)
    line = dict(sources=n, patches=args.patches, bins=args.bins, fine_bins=int(thresholds.shape[1] - 1), rmin_arcmin=args.rmin,
                rmax_arcmin=args.rmax, sort_axis=int(axis), auto_jobs=int(len(auto_jobs)), cross_jobs=int(len(cross_jobs)),
                auto_candidates=int(auto_stats.candidate_pairs), cross_candidates=int(cross_stats.candidate_pairs),
                auto_evaluated=int(auto_stats.evaluated_pairs), cross_evaluated=int(cross_stats.evaluated_pairs),
                auto_kernel_ms=round(auto_dev, 3), cross_kernel_ms=round(cross_dev, 3),
                auto_wall_ms=round(auto_wall, 3), cross_wall_ms=round(cross_wall, 3),
                auto_ps_per_evaluated=round(auto_ps, 3), cross_ps_per_evaluated=round(cross_ps, 3),
                per_evaluated_ratio=round(auto_ps / cross_ps, 3),
                auto_weight_in_range=float(W.sum()), cross_weight_in_range=float(W_cross.sum()),
                xi_plus=float(P.sum() / W.sum()), xi_minus=float(M.sum() / W.sum()), xi_cross=float(C.sum() / W.sum()),
                repeat=args.repeat, source_sha16=source_sha16())
    text = json.dumps(line)
    print(text, flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "a") as f:
        f.write(text + "\n")


if __name__ == "__main__":
    main()
