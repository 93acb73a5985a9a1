#!/usr/bin/env python3
"""Timing probe (not a test): the shear-shear count over a cell list against the shear-shear count inside the bins.

The input of tools/probe_shear_auto.py: weighted sources with a random shear and redshifts in ``--bins`` slices, uniform in a
box of ``--box`` degrees cut into ``--patches`` patches (a square grid of centres); one scale ``--rmin`` .. ``--rmax`` arcmin
with ``--fine`` fine bins. On the binned layout with shear, in this order in one process:

* ``auto``   ``engine.count_shear_auto_fine`` (``yawhip_shear_auto_count``, kernel ``k_count_shear_auto``) on the ``p <= q`` job
             list of the linkage;
* ``same``   ``engine.count_shear_pair_fine`` (``yawhip_shear_pair_count``, kernel ``k_count_shear_pair``) on the cells
             ``(p, q, k, k, k)`` of the same jobs and bins: the same separations in the same order (the sums are compared bit
             for bit), so the time per evaluated separation should be the same;
* ``upper``  the same call on the cells of every bin pair ``i <= j`` as ``count_shear_tomographic_pairs`` builds them: the
             ``p <= q`` jobs inside a bin, every linked ``(p, q)`` between two bins (left out with ``--no-upper``).

Each is run once to warm up, then ``--repeat`` times; the medians of the device time (``CountStats.kernel_ms``, events around
the kernel) and of the host wall time around the blocking call are reported with the separations each evaluated. Prints one
JSON line and appends it to ``--out`` (profiles/shear_tomo_probe.jsonl holds the committed runs). Run it several times to see
the spread from one process to the next.

Usage:  python tools/probe_shear_tomo.py --sources 2e6 --patches 64 --rmax 10
"""
from __future__ import annotations

import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import yet_another_wizz_amd as yaw  # noqa: E402
from probe_shear_auto import timed  # noqa: E402
from yet_another_wizz_amd import _lib, engine  # noqa: E402
from yet_another_wizz_amd.build import source_sha16  # noqa: E402


def cells_of(jobs, i, j):
    return np.column_stack([jobs, np.full(len(jobs), i), np.full(len(jobs), j), np.full(len(jobs), min(i, j))]).astype(np.int32)


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
    ap.add_argument("--no-upper", action="store_true")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "shear_tomo_probe.jsonl"))
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
    binned = sources.build_trees(config.binning.edges, closed=config.binning.closed, with_shear=True)
    links = yaw.PatchLinkage.from_catalogs(config, sources)
    auto_jobs = links.get_patch_pairs(sources)
    cross_jobs = links.get_patch_pairs(sources, sources)
    _, thresholds = links._angular_setup()
    axis = links.sort_axis
    # (p, q, k, k, k) in the order of the auto count's [jobs, B] cells
    same_cells = np.array([(p, q, k, k, k) for p, q in auto_jobs for k in range(args.bins)], dtype=np.int32)
    upper_cells = np.concatenate([cells_of(auto_jobs if i == j else cross_jobs, i, j)
                                  for i in range(args.bins) for j in range(i, args.bins)])

    def per_evaluated(device_ms, stats):
        return 1e9 * device_ms / max(stats.evaluated_pairs, 1)

    auto_wall, auto_dev, (*auto_planes, auto_stats) = timed(
        lambda: engine.count_shear_auto_fine(binned, auto_jobs, thresholds, sort_axis=axis), args.repeat)
    same_wall, same_dev, (*same_planes, same_stats) = timed(
        lambda: engine.count_shear_pair_fine(binned, binned, same_cells, thresholds, sort_axis=axis), args.repeat)
    same_bits = all(np.array_equal(a.reshape(b.shape), b) for a, b in zip(same_planes, auto_planes))
    auto_ps, same_ps = per_evaluated(auto_dev, auto_stats), per_evaluated(same_dev, same_stats)
    line = dict(sources=n, patches=args.patches, bins=args.bins, fine_bins=int(thresholds.shape[1] - 1), rmin_arcmin=args.rmin,
                rmax_arcmin=args.rmax, sort_axis=int(axis), auto_jobs=int(len(auto_jobs)), cross_jobs=int(len(cross_jobs)),
                same_cells=int(len(same_cells)), auto_evaluated=int(auto_stats.evaluated_pairs),
                same_evaluated=int(same_stats.evaluated_pairs), auto_kernel_ms=round(auto_dev, 3), same_kernel_ms=round(same_dev, 3),
                auto_wall_ms=round(auto_wall, 3), same_wall_ms=round(same_wall, 3), auto_ps_per_evaluated=round(auto_ps, 3),
                same_ps_per_evaluated=round(same_ps, 3), same_over_auto=round(same_ps / auto_ps, 4), same_bits_as_auto=bool(same_bits))
    if not args.no_upper:
        upper_wall, upper_dev, (P, M, C, W, upper_stats) = timed(
            lambda: engine.count_shear_pair_fine(binned, binned, upper_cells, thresholds, sort_axis=axis), args.repeat)
        line.update(upper_cells=int(len(upper_cells)), upper_candidates=int(upper_stats.candidate_pairs),
                    upper_evaluated=int(upper_stats.evaluated_pairs), upper_kernel_ms=round(upper_dev, 3),
                    upper_wall_ms=round(upper_wall, 3), upper_ps_per_evaluated=round(per_evaluated(upper_dev, upper_stats), 3),
                    upper_weight_in_range=float(W.sum()), xi_plus=float(P.sum() / W.sum()), xi_minus=float(M.sum() / W.sum()),
                    xi_cross=float(C.sum() / W.sum()))
    line.update(repeat=args.repeat, source_sha16=source_sha16())
    text = json.dumps(line)
    print(text, flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "a") as f:
        f.write(text + "\n")


if __name__ == "__main__":
    main()
