#!/usr/bin/env python3
"""Timing probe (not a test): the projected position-shape count of a shape sample about a density sample, against the
pi-binned pair count on the same columns, cells and edges.

The scene is that of tools/probe_projected.py with ``g1``, ``g2`` added: weighted objects with redshifts uniform in
0.1 < z < 0.9 in ``--bins`` slices, uniform in a box of ``--box`` degrees cut into ``--patches`` patches; one scale ``--rmin`` ..
``--rmax`` kpc with ``--fine`` fine bins and ``--pi-bins`` equal bins from 0 to ``--pi-max`` Mpc. The objects serve as the density
sample and, with their shear, as the shape sample (two ``Catalog`` instances: an object meets itself at ``R2 == 0``, which is in
no bin). The cells are ALL linked patch pairs ``(p, q)``, bin ``k`` with bin ``k``, as ``crosscorrelate_alignment`` counts them.

* runs ``engine.count_projected_shear_fine`` (``yawhip_proj_count_shear``, kernel ``k_count_projected_shear``) and, in the same
  process, ``engine.count_projected_pi_fine`` (``yawhip_proj_count_pi``, kernel ``k_count_projected_pi``) on the same density
  handle, the shapes' ``(x, y, z, w, d, c)`` as a plain projected handle, the same cells and edges: each once to warm up, then
  ``--repeat`` times in turns (the median and the min - max spread of ``CountStats.kernel_ms``, the device time between the
  call's two events). The two walks are identical up to the pair term, so the RATIO of the medians is the cost of the
  rotation and of three planes per pi bin;
* asserts that over the whole call ``W`` equals the pair count's planes to 1e-10 and that both report the same candidate and
  evaluated pairs, and checks ``--check`` of the smallest cells that hold pairs against the numpy brute force of
  tests/proj_shear_oracle.py: ``|ours - oracle| <= 1e-10 A`` per pi bin and fine bin;
* prints one JSON line and appends it to ``--out`` (profiles/alignment_probe.jsonl holds the committed runs).

Usage:  python tools/probe_alignment.py --objects 2e6 --patches 64
"""
from __future__ import annotations

import argparse
import json
import os
import statistics
import sys

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
    ap.add_argument("--pi-bins", type=int, default=1)
    ap.add_argument("--repeat", type=int, default=5)
    ap.add_argument("--check", type=int, default=4, help="cells compared with the oracle")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "alignment_probe.jsonl"))
    args = ap.parse_args()
    if _lib.device_count() < 1:
        raise SystemExit("no GPU: nothing to time")
    import proj_oracle
    import proj_shear_oracle

    n = int(float(args.objects))
    side = int(round(np.sqrt(args.patches)))
    if side * side != args.patches:
        raise SystemExit("--patches must be a square number")
    cosmology = yaw.Configuration.create(rmin=1.0, rmax=2.0, unit="kpc", zmin=0.1, zmax=0.9, num_bins=1).cosmology
    rmax = args.rmax if args.rmax is not None else round(1e3 * np.deg2rad(10.0 / 60.0) * float(cosmology.angular_diameter_distance(0.1)), 1)
    rng = np.random.default_rng(1)
    grid = (np.arange(side) + 0.5) * args.box / side
    centers = yaw.AngularCoordinates(np.deg2rad([[10.0 + a, -0.5 * args.box + b] for a in grid for b in grid]))
    columns = dict(redshifts=rng.uniform(0.1, 0.9, n), weights=rng.uniform(0.5, 1.5, n), patch_centers=centers)
    ra, dec = rng.uniform(10.0, 10.0 + args.box, n), rng.uniform(-0.5 * args.box, 0.5 * args.box, n)
    density = yaw.Catalog.from_arrays(ra, dec, **columns)
    shapes = yaw.Catalog.from_arrays(ra, dec, g1=rng.normal(0.0, 0.2, n), g2=rng.normal(0.0, 0.2, n), **columns)
    config = yaw.Configuration.create(rmin=args.rmin, rmax=rmax, unit="kpc", rweight=0.0, resolution=args.fine,
                                      zmin=0.1, zmax=0.9, num_bins=args.bins)
    unit = config.scales.scales.unit
    dens_layout = density.build_trees(config.binning.edges, closed=config.binning.closed, with_redshifts=True)
    shape_layout = shapes.build_trees(config.binning.edges, closed=config.binning.closed, with_shear=True, with_redshifts=True)
    max_angle = measurements.radial_max_angle(config, dens_layout, shape_layout)
    links = yaw.PatchLinkage.from_catalogs(config, density, shapes, max_angle=max_angle)
    jobs = links.get_patch_pairs(density, shapes)
    r2 = measurements.threshold_table(measurements.radial_plans(config))
    nb = args.bins
    seg1 = (jobs[:, :1].astype(np.int64) * nb + np.arange(nb)).ravel()
    seg2 = (jobs[:, 1:].astype(np.int64) * nb + np.arange(nb)).ravel()
    cells = np.column_stack([seg1, seg2, np.tile(np.arange(nb), len(jobs)), np.zeros(len(seg1))]).astype(np.int32)
    pi_edges = engine.check_pi_edges(args.pi_bins, args.pi_max)
    kwargs = dict(pi_edges=pi_edges, cosmology=config.cosmology, unit=unit, sort_axis=links.sort_axis)

    def shear():
        return engine.count_projected_shear_fine(dens_layout, shape_layout, cells, r2, **kwargs)

    def pairs():
        return engine.count_projected_pi_fine(dens_layout, shape_layout, cells, r2, **kwargs)

    shear(), pairs()  # warm-up (uploads, code objects)
    ms = {"shear": [], "pairs": []}
    for _ in range(args.repeat):  # in turns: both see the same state of the device
        (T, X, W), stats = shear()
        W_pi, stats_pi = pairs()
        ms["shear"].append(stats.kernel_ms), ms["pairs"].append(stats_pi.kernel_ms)
    if (stats.candidate_pairs, stats.evaluated_pairs) != (stats_pi.candidate_pairs, stats_pi.evaluated_pairs):
        raise SystemExit("the two counts do not report the same walk")
    if not np.allclose(W, W_pi, rtol=1e-10, atol=0):
        raise SystemExit("W is not the pair count's")

    # the smallest cells that hold pairs, against the brute force
    dens = proj_oracle.as_handle(dens_layout, *engine.proj_columns(dens_layout, config.cosmology, unit))
    shp = proj_shear_oracle.as_shapes(shape_layout, *engine.proj_columns(shape_layout, config.cosmology, unit))
    sizes_d, sizes_s = np.diff(dens_layout.offsets), np.diff(shape_layout.offsets)
    cost = sizes_d[cells[:, 0]].astype(np.float64) * sizes_s[cells[:, 1]]
    holds = np.flatnonzero(W.sum(axis=(0, 2)) > 0)
    checked = list(holds[np.argsort(cost[holds], kind="stable")][: args.check])
    worst = 0.0
    if checked:
        exp = proj_shear_oracle.proj_shear_cells(dens, shp, cells[checked], r2, pi_edges)
        for ours, theirs in ((T, exp[0]), (X, exp[1])):
            differs = np.abs(ours[:, checked] - theirs)
            if not np.all(differs <= 1e-10 * exp[3]):
                raise SystemExit(f"cells {checked} differ from the oracle by up to {np.max(differs / np.maximum(exp[3], 1e-300)):.3e} A")
            worst = max(worst, float(np.max(differs[exp[3] > 0] / exp[3][exp[3] > 0])))
        if not np.allclose(W[:, checked], exp[2], rtol=1e-10, atol=0):
            raise SystemExit(f"W of the cells {checked} differs from the oracle")
    median = {name: statistics.median(values) for name, values in ms.items()}
    n_edges, n_pi = int(r2.shape[1]), len(pi_edges) - 1
    lds = 2 * 256 * 48 + 8 * (((n_edges + 1) & ~1) + ((n_pi + 2) & ~1)) + 4 * 3 * n_pi * (n_edges - 1) * 8
    line = dict(objects=n, patches=args.patches, bins=nb, jobs=int(len(jobs)), cells=int(len(cells)), fine_bins=n_edges - 1, pi_bins=n_pi,
                rmin_kpc=args.rmin, rmax_kpc=rmax, pi_max_mpc=args.pi_max, max_angle_arcmin=round(float(np.rad2deg(max_angle)) * 60.0, 3),
                sort_axis=int(links.sort_axis), candidate_pairs=int(stats.candidate_pairs), evaluated=int(stats.evaluated_pairs),
                kernel="k_count_projected_shear", kernel_ms=round(median["shear"], 3),
                kernel_ms_spread=[round(min(ms["shear"]), 3), round(max(ms["shear"]), 3)],
                pairs_kernel="k_count_projected_pi", pairs_kernel_ms=round(median["pairs"], 3),
                pairs_kernel_ms_spread=[round(min(ms["pairs"]), 3), round(max(ms["pairs"]), 3)],
                ratio=round(median["shear"] / median["pairs"], 3), ps_per_evaluated=round(1e9 * median["shear"] / max(stats.evaluated_pairs, 1), 3),
                weight_in_range=float(W.sum()), member_share_of_evaluated=round(float(W_pi.sum() / np.mean(columns["weights"]) ** 2) / max(stats.evaluated_pairs, 1), 5),
                lds_bytes_per_workgroup=lds, workgroups_per_cu_by_lds=(160 * 1024) // lds, cells_checked=[int(c) for c in checked],
                worst_difference_over_A=worst, repeat=args.repeat, source_sha16=source_sha16())
    text = json.dumps(line)
    print(text, flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "a") as f:
        f.write(text + "\n")


if __name__ == "__main__":
    main()
