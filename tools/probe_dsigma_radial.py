#!/usr/bin/env python3
"""Timing probe (not a test): the excess-surface-density count binned per lens against the count binned per slice.

The input of tools/probe_dsigma.py with scales in kpc: lenses with redshifts in ``--bins`` slices over 0.1 < z < 0.9 and
weighted sources with a random shear and redshifts from the same range, uniform in a box of ``--box`` degrees cut into
``--patches`` patches; one scale ``--rmin`` .. ``--rmax`` kpc with ``--fine`` fine bins. On one job list (the linkage that
reaches as far as the nearest lens sees ``--rmax``):

* ``radial``  ``engine.count_dsigma_radial_fine`` (``yawhip_dsigma_count_radial``, kernel ``k_count_dsigma_radial``) with the
              squared radii of the configuration's radial plan;
* ``slice``   ``engine.count_dsigma_fine`` (``yawhip_dsigma_count``, kernel ``k_count_dsigma``) on the same layouts and jobs
              with the chord thresholds at the slice middles -- with ``--parent-tree`` through the package and the built
              library of another checkout (the parent commit's), else through this tree's.

The two do NOT evaluate the same separations: the key window of the per-lens count follows the nearest lens of a redshift
bin, that of the per-slice count the slice's middle. The comparison is therefore the device time per evaluated separation.
Each call is run once to warm up, then ``--repeat`` times: the median and the min - max spread of the device time between
the call's two events (``CountStats.kernel_ms``), and of the host's wall time around the blocking call.

Every measurement runs in a process of its own, one after the other; this process only starts them and never opens the
device. Prints one JSON line and appends it to ``--out`` (profiles/dsigma_radial_probe.jsonl holds the committed runs).

Usage:  python tools/probe_dsigma_radial.py [--parent-tree /path/to/a/built/checkout/of/the/parent]
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
    ap.add_argument("--rmin", type=float, default=100.0, help="kpc")
    ap.add_argument("--rmax", type=float, default=2000.0, help="kpc")
    ap.add_argument("--fine", type=int, default=50)
    ap.add_argument("--repeat", type=int, default=5)
    ap.add_argument("--parent-tree", default=None, help="another checkout, its library built, to time the per-slice count with")
    ap.add_argument("--label", default=None, help="a word for the line's \"label\" key, e.g. which tree this run times")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "dsigma_radial_probe.jsonl"))
    ap.add_argument("--call", choices=["radial", "slice"], default=None, help="(internal) time this call in this process")
    ap.add_argument("--tree", default=ROOT, help="(internal) the checkout whose package the measuring process imports")
    return ap.parse_args()


def measure(args):
    """One call, timed in this process; prints its JSON fragment. Only what the parent commit's package has as well is used
    for the per-slice call: the job list and the edges come from plain arithmetic on the configuration."""
    import numpy as np

    sys.path.insert(0, os.path.abspath(args.tree))
    import yet_another_wizz_amd as yaw
    from yet_another_wizz_amd import _lib, engine, measurements

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

    lens_z = rng.uniform(0.1, 0.9, n_lens)
    lenses = yaw.Catalog.from_arrays(*positions(n_lens), redshifts=lens_z, weights=rng.uniform(0.5, 1.5, n_lens), patch_centers=centers)
    sources = yaw.Catalog.from_arrays(*positions(n_src), redshifts=rng.uniform(0.1, 0.9, n_src), weights=rng.uniform(0.5, 1.5, n_src),
                                      g1=rng.normal(0, 0.3, n_src), g2=rng.normal(0, 0.3, n_src), patch_centers=centers)
    config = yaw.Configuration.create(rmin=args.rmin, rmax=args.rmax, unit="kpc", rweight=0.0, resolution=args.fine,
                                      zmin=0.1, zmax=0.9, num_bins=args.bins)
    lens_layout = lenses.build_trees(config.binning.edges, closed=config.binning.closed, with_redshifts=True)
    source_layout = sources.build_trees(None, with_redshifts=True)
    # one job list for both calls: every patch pair within reach of the nearest lens of the catalogue
    d_near = float(config.cosmology.angular_diameter_distance(float(lens_z.min())))
    reach = 1e-3 * args.rmax / d_near * (1.0 + 1e-6)
    links = yaw.PatchLinkage.from_catalogs(config, lenses, sources)
    xyz, radii = sources.get_centers().to_3d(), sources.get_radii().data  # (the larger catalogue, as the linkage takes it)
    chord = np.sqrt(((xyz[:, None, :] - xyz[None, :, :]) ** 2).sum(axis=2))
    linked = 2.0 * np.arcsin(chord / 2.0) < radii[None, :] + radii[:, None] + reach
    jobs = np.ascontiguousarray(np.argwhere(linked), dtype=np.int32)
    axis = links.sort_axis
    if args.call == "radial":
        edges = measurements.threshold_table(measurements.radial_plans(config))

        def call():
            return engine.count_dsigma_radial_fine(lens_layout, source_layout, jobs, edges, cosmology=config.cosmology,
                                                   unit=config.scales.scales.unit, sort_axis=axis)
    else:
        _, edges = links._angular_setup()

        def call():
            return engine.count_dsigma_fine(lens_layout, source_layout, jobs, edges, cosmology=config.cosmology, sort_axis=axis)
    call()  # warm-up (uploads, code objects)
    wall, device = [], []
    for _ in range(args.repeat):
        t0 = time.perf_counter()
        *planes, stats = call()
        wall.append(1e3 * (time.perf_counter() - t0))
        device.append(stats.kernel_ms)
    print(json.dumps(dict(jobs=int(len(jobs)), fine_bins=int(edges.shape[1] - 1), sort_axis=int(axis),
                          candidate_pairs=int(stats.candidate_pairs), evaluated=int(stats.evaluated_pairs),
                          kernel_ms=round(statistics.median(device), 3), kernel_ms_min=round(min(device), 3),
                          kernel_ms_max=round(max(device), 3), wall_ms=round(statistics.median(wall), 3),
                          wall_ms_min=round(min(wall), 3), wall_ms_max=round(max(wall), 3),
                          cells_with_pairs=int(np.count_nonzero(planes[2])), sum_w=float(planes[2].sum()), library=_lib.LIB_PATH)), flush=True)


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

    radial = child("radial")
    per_slice = child("slice", args.parent_tree or ROOT)
    assert radial["jobs"] == per_slice["jobs"] and radial["candidate_pairs"] == per_slice["candidate_pairs"]
    line = dict(probe="tools/probe_dsigma_radial.py", **({"label": args.label} if args.label else {}), lenses=int(float(args.lenses)), sources=int(float(args.sources)), patches=args.patches, bins=args.bins, jobs=radial["jobs"],
                fine_bins=radial["fine_bins"], rmin_kpc=args.rmin, rmax_kpc=args.rmax, sort_axis=radial["sort_axis"],
                candidate_pairs=radial["candidate_pairs"], slice_library="parent" if args.parent_tree else "this tree")
    for name, got in (("radial", radial), ("slice", per_slice)):
        line.update({f"{name}_kernel_ms": got["kernel_ms"], f"{name}_kernel_ms_spread": [got["kernel_ms_min"], got["kernel_ms_max"]],
                     f"{name}_wall_ms": got["wall_ms"], f"{name}_wall_ms_spread": [got["wall_ms_min"], got["wall_ms_max"]],
                     f"{name}_evaluated": got["evaluated"],
                     f"{name}_ps_per_evaluated": round(1e9 * got["kernel_ms"] / max(got["evaluated"], 1), 3),
                     f"{name}_cells_with_pairs": got["cells_with_pairs"], f"{name}_sum_w": got["sum_w"]})
    line.update(per_evaluated_ratio=round(line["radial_ps_per_evaluated"] / line["slice_ps_per_evaluated"], 3),
                evaluated_ratio=round(radial["evaluated"] / max(per_slice["evaluated"], 1), 3),
                kernel_ratio=round(radial["kernel_ms"] / per_slice["kernel_ms"], 3), repeat=args.repeat, source_sha16=source_sha16())
    text = json.dumps(line)
    print(text, flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "a") as f:
        f.write(text + "\n")


if __name__ == "__main__":
    main()
