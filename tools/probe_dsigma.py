#!/usr/bin/env python3
"""Timing probe (not a test): the excess-surface-density count against the shear count of the same layouts and jobs.

The input of tools/probe_shear.py with redshifts on the sources as well: lenses with redshifts in ``--bins`` slices and
weighted sources with a random shear and redshifts from the same range (about half of all pairs have the source in front),
uniform in a box of ``--box`` degrees cut into ``--patches`` patches; one scale ``--rmin`` .. ``--rmax`` arcmin with ``--fine``
fine bins. On the linkage's job list:

* ``dsigma``  ``engine.count_dsigma_fine`` (``yawhip_dsigma_count``, kernel ``k_count_dsigma``);
* ``shear``   ``engine.count_shear_fine`` (``yawhip_shear_count``, kernel ``k_count_shear``) on the same layouts, once with
              the package of this tree and, with ``--parent-tree``, once with the package and the built library of another
              checkout (the parent commit's): the existing kernel has to sit inside that one's spread.

Both evaluate the same separations (the key window knows nothing of redshifts), so ``dsigma / shear`` is the cost of the wider
streamed object (48 bytes against 32) and of the longer term of the pairs in range. Each call is run once to warm up, then
``--repeat`` times: the median and the min - max spread of the device time between the call's two events
(``CountStats.kernel_ms``), and the median host wall time around the blocking call.

Every measurement runs in a process of its own, one after the other (a process imports one package and loads one
library); this process only starts them and never opens the device. Prints one JSON line and appends it to ``--out``
(profiles/dsigma_probe.jsonl holds the committed runs).

Usage:  python tools/probe_dsigma.py --rmax 10 [--parent-tree /path/to/a/built/checkout/of/the/parent]
"""
from __future__ import annotations

import argparse
import json
import os
import statistics
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def arguments():
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
    ap.add_argument("--parent-tree", default=None, help="another checkout, its library built, to time the shear count with")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "dsigma_probe.jsonl"))
    ap.add_argument("--call", choices=["dsigma", "shear"], default=None, help="(internal) time this call in this process")
    ap.add_argument("--tree", default=ROOT, help="(internal) the checkout whose package the measuring process imports")
    return ap.parse_args()


def measure(args):
    """One call, timed in this process; prints its JSON fragment."""
    import numpy as np

    sys.path.insert(0, os.path.abspath(args.tree))
    import yet_another_wizz_amd as yaw
    from yet_another_wizz_amd import _lib, engine

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
    sources = yaw.Catalog.from_arrays(*positions(n_src), redshifts=rng.uniform(0.1, 0.9, n_src), weights=rng.uniform(0.5, 1.5, n_src),
                                      g1=rng.normal(0, 0.3, n_src), g2=rng.normal(0, 0.3, n_src), patch_centers=centers)
    config = yaw.Configuration.create(rmin=args.rmin, rmax=args.rmax, unit="arcmin", rweight=0.0, resolution=args.fine,
                                      zmin=0.1, zmax=0.9, num_bins=args.bins)
    # (the layouts of the two calls differ by the column of redshifts only: the same objects, segments and order)
    with_z = dict(with_redshifts=True) if args.call == "dsigma" else {}
    lens_layout = lenses.build_trees(config.binning.edges, closed=config.binning.closed, **with_z)
    source_layout = sources.build_trees(None, **with_z)
    links = yaw.PatchLinkage.from_catalogs(config, lenses, sources)
    jobs = links.get_patch_pairs(lenses, sources)
    _, thresholds = links._angular_setup()
    axis = links.sort_axis
    if args.call == "dsigma":
        def call():
            return engine.count_dsigma_fine(lens_layout, source_layout, jobs, thresholds, cosmology=config.cosmology, sort_axis=axis)
    else:
        def call():
            return engine.count_shear_fine(lens_layout, source_layout, jobs, thresholds, sort_axis=axis)
    call()  # warm-up (uploads, code objects)
    wall, device = [], []
    for _ in range(args.repeat):
        t0 = time.perf_counter()
        *planes, stats = call()
        wall.append(1e3 * (time.perf_counter() - t0))
        device.append(stats.kernel_ms)
    print(json.dumps(dict(jobs=int(len(jobs)), fine_bins=int(thresholds.shape[1] - 1), sort_axis=int(axis),
                          candidate_pairs=int(stats.candidate_pairs), evaluated=int(stats.evaluated_pairs),
                          kernel_ms=round(statistics.median(device), 3), kernel_ms_min=round(min(device), 3),
                          kernel_ms_max=round(max(device), 3), wall_ms=round(statistics.median(wall), 3),
                          cells_with_pairs=int(np.count_nonzero(planes[2])), library=_lib.LIB_PATH)), flush=True)


def main():
    args = arguments()
    if args.call:
        return measure(args)
    sys.path.insert(0, ROOT)
    from yet_another_wizz_amd.build import source_sha16

    def child(call, tree=ROOT):
        env = dict(os.environ)
        env.pop("YAW_AMD_LIB", None)  # every tree loads its own library
        argv = [sys.executable, os.path.abspath(__file__), "--call", call, "--tree", os.path.abspath(tree)]
        for name in ("lenses", "sources", "patches", "bins", "box", "rmin", "rmax", "fine", "repeat"):
            argv += [f"--{name}", str(getattr(args, name))]
        done = subprocess.run(argv, env=env, stdout=subprocess.PIPE, text=True, timeout=900)
        if done.returncode != 0:
            raise SystemExit(f"the {call} measurement failed (exit status {done.returncode}): nothing more is started")
        return json.loads(done.stdout.strip().splitlines()[-1])

    dsigma = child("dsigma")
    shear = child("shear")
    parent = child("shear", args.parent_tree) if args.parent_tree else None
    assert dsigma["evaluated"] == shear["evaluated"] and dsigma["jobs"] == shear["jobs"]
    line = dict(lenses=int(float(args.lenses)), sources=int(float(args.sources)), patches=args.patches, bins=args.bins, jobs=shear["jobs"],
                fine_bins=shear["fine_bins"], rmin_arcmin=args.rmin, rmax_arcmin=args.rmax, sort_axis=shear["sort_axis"],
                candidate_pairs=shear["candidate_pairs"], evaluated=shear["evaluated"])
    for name, got in (("dsigma", dsigma), ("shear", shear), ("shear_parent", parent)):
        if got is not None:
            line.update({f"{name}_kernel_ms": got["kernel_ms"], f"{name}_kernel_ms_spread": [got["kernel_ms_min"], got["kernel_ms_max"]],
                         f"{name}_wall_ms": got["wall_ms"]})
    against = parent or shear
    line.update(kernel_ratio=round(dsigma["kernel_ms"] / against["kernel_ms"], 3), ratio_against="shear_parent" if parent else "shear",
                dsigma_ps_per_evaluated=round(1e9 * dsigma["kernel_ms"] / max(dsigma["evaluated"], 1), 3),
                shear_ps_per_evaluated=round(1e9 * against["kernel_ms"] / max(against["evaluated"], 1), 3),
                dsigma_cells_with_pairs=dsigma["cells_with_pairs"], shear_cells_with_pairs=shear["cells_with_pairs"],
                repeat=args.repeat, source_sha16=source_sha16())
    if parent:
        line["shear_inside_parent_spread"] = bool(parent["kernel_ms_min"] <= shear["kernel_ms"] <= parent["kernel_ms_max"])
    text = json.dumps(line)
    print(text, flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "a") as f:
        f.write(text + "\n")


if __name__ == "__main__":
    main()
