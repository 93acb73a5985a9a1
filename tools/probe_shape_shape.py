#!/usr/bin/env python3
"""Timing probe (not a test): the projected shape-shape count of a shape sample, against the pi-binned pair count and the
position-shape count on the same columns, cells and edges.

The scene is that of tools/probe_alignment.py: weighted objects with ``g1``, ``g2`` and redshifts uniform in 0.1 < z < 0.9 in
``--bins`` slices, uniform in a box of ``--box`` degrees cut into ``--patches`` patches; one scale ``--rmin`` .. ``--rmax`` kpc.
The objects are two ``Catalog`` instances, so that ONE cell list serves all three counts: ALL linked patch pairs ``(p, q)``,
bin ``k`` with bin ``k``, no diagonal cells (the position-shape count has none; an object meets itself at ``R2 == 0``, which is
in no bin). Every ``--cases`` entry ``FINExPI`` is one measurement with ``FINE`` fine radius bins and ``PI`` equal pi bins from 0
to ``--pi-max`` Mpc, all in one process on the same resident handles.

* runs ``engine.count_projected_shapes_fine`` (``yawhip_proj_count_shapes``, kernel ``k_count_projected_shapes``) and, in the
  same process, ``engine.count_projected_pi_fine`` (``k_count_projected_pi``) and ``engine.count_projected_shear_fine``
  (``k_count_projected_shear``) on the same columns, cells and edges: each once to warm up, then ``--repeat`` times in turns
  (the median and the min - max spread of ``CountStats.kernel_ms``, the device time between the call's two events). The three
  walks are identical up to the streamed object's size and the pair term, so the RATIOS of the medians are the cost of the
  64-byte stages, the second rotation and four planes per pi bin;
* asserts that over the whole call ``W`` equals the pair count's planes to 1e-10 and that all report the same candidate and
  evaluated pairs, and checks ``--check`` of the smallest cells that hold pairs against the numpy brute force of
  tests/proj_shape_oracle.py: ``|ours - oracle| <= 1e-10 A`` per pi bin and fine bin;
* prints one JSON line per case and appends it to ``--out`` (profiles/shape_shape_probe.jsonl holds the committed runs), with
  ``wall_ms``, the median wall time of the shape-shape call around its ``kernel_ms``, and the word of ``--label`` if one is given.

Usage:  python tools/probe_shape_shape.py --objects 2e6 --patches 64 --cases 50x1 50x5 12x1 12x21
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
    ap.add_argument("--cases", nargs="+", default=["50x1"], help="FINExPI: fine radius bins x pi bins")
    ap.add_argument("--repeat", type=int, default=5)
    ap.add_argument("--check", type=int, default=4, help="cells compared with the oracle")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "shape_shape_probe.jsonl"))
    ap.add_argument("--label", default=None, help="a word for the line's \"label\" key, e.g. which tree this run times")
    args = ap.parse_args()
    if _lib.device_count() < 1:
        raise SystemExit("no GPU: nothing to time")
    import proj_shape_oracle

    n = int(float(args.objects))
    side = int(round(np.sqrt(args.patches)))
    if side * side != args.patches:
        raise SystemExit("--patches must be a square number")
    cosmology = yaw.Configuration.create(rmin=1.0, rmax=2.0, unit="kpc", zmin=0.1, zmax=0.9, num_bins=1).cosmology
    rmax = args.rmax if args.rmax is not None else round(1e3 * np.deg2rad(10.0 / 60.0) * float(cosmology.angular_diameter_distance(0.1)), 1)
    rng = np.random.default_rng(1)
    grid = (np.arange(side) + 0.5) * args.box / side
    centers = yaw.AngularCoordinates(np.deg2rad([[10.0 + a, -0.5 * args.box + b] for a in grid for b in grid]))
    columns = dict(redshifts=rng.uniform(0.1, 0.9, n), weights=rng.uniform(0.5, 1.5, n), g1=rng.normal(0.0, 0.2, n), g2=rng.normal(0.0, 0.2, n),
                   patch_centers=centers)
    ra, dec = rng.uniform(10.0, 10.0 + args.box, n), rng.uniform(-0.5 * args.box, 0.5 * args.box, n)
    first, second = yaw.Catalog.from_arrays(ra, dec, **columns), yaw.Catalog.from_arrays(ra, dec, **columns)
    nb = args.bins
    for case in args.cases:
        fine, n_pi = (int(v) for v in case.split("x"))
        config = yaw.Configuration.create(rmin=args.rmin, rmax=rmax, unit="kpc", rweight=0.0, resolution=fine, zmin=0.1, zmax=0.9, num_bins=nb)
        unit = config.scales.scales.unit
        layout_a, layout_b = (cat.build_trees(config.binning.edges, closed=config.binning.closed, with_shear=True, with_redshifts=True)
                              for cat in (first, second))
        max_angle = measurements.radial_max_angle(config, layout_a, layout_b)
        links = yaw.PatchLinkage.from_catalogs(config, first, second, max_angle=max_angle)
        jobs = links.get_patch_pairs(first, second)
        r2 = measurements.threshold_table(measurements.radial_plans(config))
        seg1 = (jobs[:, :1].astype(np.int64) * nb + np.arange(nb)).ravel()
        seg2 = (jobs[:, 1:].astype(np.int64) * nb + np.arange(nb)).ravel()
        cells = np.column_stack([seg1, seg2, np.tile(np.arange(nb), len(jobs)), np.zeros(len(seg1))]).astype(np.int32)
        pi_edges = engine.check_pi_edges(n_pi, args.pi_max)
        kwargs = dict(pi_edges=pi_edges, cosmology=config.cosmology, unit=unit, sort_axis=links.sort_axis)
        counts = dict(shapes=lambda: engine.count_projected_shapes_fine(layout_a, layout_b, cells, r2, **kwargs),
                      pairs=lambda: engine.count_projected_pi_fine(layout_a, layout_b, cells, r2, **kwargs),
                      shear=lambda: engine.count_projected_shear_fine(layout_a, layout_b, cells, r2, **kwargs))
        for count in counts.values():
            count()  # warm-up (uploads, code objects)
        ms, wall, last = {name: [] for name in counts}, [], {}
        for _ in range(args.repeat):  # in turns: all see the same state of the device
            for name, count in counts.items():
                t0 = time.perf_counter()
                last[name] = count()
                if name == "shapes":
                    wall.append(1e3 * (time.perf_counter() - t0))
                ms[name].append(last[name][1].kernel_ms)
        (PP, XX, PX, W), stats = last["shapes"]
        W_pi = last["pairs"][0]
        walks = {(s.candidate_pairs, s.evaluated_pairs) for _, s in last.values()}
        if len(walks) != 1:
            raise SystemExit(f"the three counts do not report the same walk: {walks}")
        if not np.allclose(W, W_pi, rtol=1e-10, atol=0) or not np.allclose(W, last["shear"][0][2], rtol=1e-10, atol=0):
            raise SystemExit("W is not the pair count's")

        # the smallest cells that hold pairs, against the brute force
        a, b = (proj_shape_oracle.as_shapes(layout, *engine.proj_columns(layout, config.cosmology, unit)) for layout in (layout_a, layout_b))
        sizes_a, sizes_b = np.diff(layout_a.offsets), np.diff(layout_b.offsets)
        cost = sizes_a[cells[:, 0]].astype(np.float64) * sizes_b[cells[:, 1]]
        holds = np.flatnonzero(W.sum(axis=(0, 2)) > 0)
        checked = list(holds[np.argsort(cost[holds], kind="stable")][: args.check])
        worst = 0.0
        if checked:
            exp = proj_shape_oracle.proj_shape_cells(a, b, cells[checked], r2, pi_edges)
            for ours, theirs in zip((PP, XX, PX), exp):
                differs = np.abs(ours[:, checked] - theirs)
                if not np.all(differs <= 1e-10 * exp[4]):
                    raise SystemExit(f"cells {checked} differ from the oracle by up to {np.max(differs / np.maximum(exp[4], 1e-300)):.3e} A")
                worst = max(worst, float(np.max(differs[exp[4] > 0] / exp[4][exp[4] > 0])))
            if not np.allclose(W[:, checked], exp[3], rtol=1e-10, atol=0):
                raise SystemExit(f"W of the cells {checked} differs from the oracle")
        median = {name: statistics.median(values) for name, values in ms.items()}
        spread = {name: [round(min(values), 3), round(max(values), 3)] for name, values in ms.items()}
        n_edges = int(r2.shape[1])
        edges_bytes = 8 * (((n_edges + 1) & ~1) + ((n_pi + 2) & ~1))
        lds = {name: 2 * 256 * size + edges_bytes + 4 * planes * n_pi * (n_edges - 1) * 8 for name, (size, planes) in
               dict(shapes=(64, 4), pairs=(48, 1), shear=(48, 3)).items()}
        line = dict(**({"label": args.label} if args.label else {}), objects=n, patches=args.patches, bins=nb, jobs=int(len(jobs)), cells=int(len(cells)), fine_bins=n_edges - 1, pi_bins=n_pi,
                    rmin_kpc=args.rmin, rmax_kpc=rmax, pi_max_mpc=args.pi_max, max_angle_arcmin=round(float(np.rad2deg(max_angle)) * 60.0, 3),
                    sort_axis=int(links.sort_axis), candidate_pairs=int(stats.candidate_pairs), evaluated=int(stats.evaluated_pairs),
                    kernel="k_count_projected_shapes", kernel_ms=round(median["shapes"], 3), kernel_ms_spread=spread["shapes"],
                    wall_ms=round(statistics.median(wall), 3),
                    pairs_kernel="k_count_projected_pi", pairs_kernel_ms=round(median["pairs"], 3), pairs_kernel_ms_spread=spread["pairs"],
                    shear_kernel="k_count_projected_shear", shear_kernel_ms=round(median["shear"], 3), shear_kernel_ms_spread=spread["shear"],
                    ratio_to_pairs=round(median["shapes"] / median["pairs"], 3), ratio_to_shear=round(median["shapes"] / median["shear"], 3),
                    ps_per_evaluated=round(1e9 * median["shapes"] / max(stats.evaluated_pairs, 1), 3), weight_in_range=float(W.sum()),
                    lds_bytes_per_workgroup=lds["shapes"], workgroups_per_cu_by_lds={name: (160 * 1024) // size for name, size in lds.items()},
                    cells_checked=[int(c) for c in checked], worst_difference_over_A=worst, repeat=args.repeat, source_sha16=source_sha16())
        text = json.dumps(line)
        print(text, flush=True)
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "a") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
