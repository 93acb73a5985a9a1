#!/usr/bin/env python3
"""Timing probe (not a test): the two counts with a signed line of sight against their unsigned siblings, between two catalogues.

The input of tools/probe_projected.py, twice: two catalogues of ``--objects`` weighted objects each (seeds 1 and 2) with
redshifts uniform in 0.1 < z < 0.9 in ``--bins`` slices, in a box of ``--box`` degrees cut into ``--patches`` patches; one scale
``--rmin`` .. ``--rmax`` kpc with ``--fine`` fine bins. The cells are those of a cross count: ALL linked patch pairs ``(p, q)``,
bin ``k`` with bin ``k``, none diagonal. On ONE pair of resident handles, one cell list and one table of radius edges, for every
``n`` of ``--planes`` and for pi (``yawhip_proj_count_pi`` / ``_pi_signed``, edges to ``+-pi_max``) and mu
(``yawhip_proj_count_smu`` / ``_smu_signed``, the radii read as ``s``):

* the unsigned sibling at ``n`` equal bins, the signed kernel at ``n`` equal bins (the same number of planes) and at ``2 n``
  (the mirrored set) where the LDS cap admits it: a warm-up, then ``--repeat`` calls each, the median and the min - max spread
  of the device time between the call's two events (``CountStats.kernel_ms``);
* ``--check`` of the smallest cells that hold pairs against tests/proj_signed_oracle.py / tests/smu_signed_oracle.py,
  ``|ours - oracle| <= 1e-10 A`` per signed bin and fine bin, and the fold of the mirrored planes against the sibling's to the
  same bound;
* one JSON line per ``n`` and kind (device ms of the three, the two ratios, evaluated separations) printed and appended to
  ``--out`` (profiles/signed_probe.jsonl holds the committed runs), with the word of ``--label`` if one is given.

Usage:  python tools/probe_signed.py --fine 50 --planes 1,12
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


def lds_bytes(n_edges, n):
    """The carve-up of include/yawhip.h for the four kernels timed here."""
    return 2 * 256 * 48 + 8 * (((n_edges + 1) & ~1) + ((n + 2) & ~1)) + 4 * n * (n_edges - 1) * 8


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--objects", default="2e6", help="per catalogue")
    ap.add_argument("--patches", type=int, default=64, help="a square number")
    ap.add_argument("--bins", type=int, default=4)
    ap.add_argument("--box", type=float, default=10.0)
    ap.add_argument("--rmin", type=float, default=50.0, help="kpc")
    ap.add_argument("--rmax", type=float, default=None, help="kpc (default: 10 arcmin at z = 0.1)")
    ap.add_argument("--pi-max", type=float, default=60.0, help="Mpc")
    ap.add_argument("--fine", type=int, default=50)
    ap.add_argument("--planes", default="1,12", help="the numbers n of bins, comma separated")
    ap.add_argument("--repeat", type=int, default=5)
    ap.add_argument("--check", type=int, default=2, help="cells compared with the oracle")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "signed_probe.jsonl"))
    ap.add_argument("--label", default=None, help="a word for the line's \"label\" key")
    args = ap.parse_args()
    if _lib.device_count() < 1:
        raise SystemExit("no GPU: nothing to time")
    import proj_oracle
    import proj_signed_oracle
    import smu_signed_oracle

    n_obj = int(float(args.objects))
    side = int(round(np.sqrt(args.patches)))
    if side * side != args.patches:
        raise SystemExit("--patches must be a square number")
    cosmology = yaw.Configuration.create(rmin=1.0, rmax=2.0, unit="kpc", zmin=0.1, zmax=0.9, num_bins=1).cosmology
    rmax = args.rmax if args.rmax is not None else round(1e3 * np.deg2rad(10.0 / 60.0) * float(cosmology.angular_diameter_distance(0.1)), 1)
    grid = (np.arange(side) + 0.5) * args.box / side
    centers = yaw.AngularCoordinates(np.deg2rad([[10.0 + a, -0.5 * args.box + b] for a in grid for b in grid]))
    catalogs = []
    for seed in (1, 2):
        rng = np.random.default_rng(seed)
        catalogs.append(yaw.Catalog.from_arrays(rng.uniform(10.0, 10.0 + args.box, n_obj), rng.uniform(-0.5 * args.box, 0.5 * args.box, n_obj),
                                                redshifts=rng.uniform(0.1, 0.9, n_obj), weights=rng.uniform(0.5, 1.5, n_obj), patch_centers=centers))
    config = yaw.Configuration.create(rmin=args.rmin, rmax=rmax, unit="kpc", rweight=0.0, resolution=args.fine, zmin=0.1, zmax=0.9,
                                      num_bins=args.bins)
    unit = config.scales.scales.unit
    layouts = [cat.build_trees(config.binning.edges, closed=config.binning.closed, with_redshifts=True) for cat in catalogs]
    max_angle = measurements.radial_max_angle(config, *layouts)
    links = yaw.PatchLinkage.from_catalogs(config, *catalogs, max_angle=max_angle)
    jobs = links.get_patch_pairs(*catalogs)
    table = measurements.threshold_table(measurements.radial_plans(config))
    nb, n_edges = args.bins, int(table.shape[1])
    seg1 = (jobs[:, :1].astype(np.int64) * nb + np.arange(nb)).ravel()
    seg2 = (jobs[:, 1:].astype(np.int64) * nb + np.arange(nb)).ravel()
    cells = np.column_stack([seg1, seg2, np.tile(np.arange(nb), len(jobs)), np.zeros(len(seg1))]).astype(np.int32)
    kwargs = dict(cosmology=config.cosmology, unit=unit, sort_axis=links.sort_axis)
    handles = [proj_oracle.as_handle(layout, *engine.proj_columns(layout, config.cosmology, unit)) for layout in layouts]
    sizes = [np.diff(layout.offsets) for layout in layouts]
    cost = sizes[0][cells[:, 0]].astype(np.float64) * sizes[1][cells[:, 1]]

    def timed(count, **edges):
        count(*layouts, cells, table, **edges, **kwargs)  # warm-up (uploads, code objects)
        device = []
        for _ in range(args.repeat):
            W, stats = count(*layouts, cells, table, **edges, **kwargs)
            device.append(stats.kernel_ms)
        return W, stats, dict(ms=round(statistics.median(device), 3), spread=[round(min(device), 3), round(max(device), 3)])

    def against_oracle(W, oracle, edges):
        holds = W.sum(axis=(0, 2)) > 0
        of_kind = np.flatnonzero(holds)
        checked = list(of_kind[np.argsort(cost[of_kind], kind="stable")][: args.check])
        if not checked:
            return [], 0.0
        exp_w, exp_a, _ = oracle(*handles, cells[checked], table, edges)
        differs = np.abs(W[:, checked] - exp_w)
        if not np.all(differs <= 1e-10 * exp_a):
            raise SystemExit(f"cells {checked} differ from the oracle by up to {np.max(differs / np.maximum(exp_a, 1e-300)):.3e} A")
        return [int(c) for c in checked], float(np.max(differs[exp_a > 0] / exp_a[exp_a > 0])) if np.any(exp_a > 0) else 0.0

    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    for n in (int(v) for v in args.planes.split(",")):
        for kind in ("pi", "mu"):
            if kind == "pi":
                sibling, signed, key, top = engine.count_projected_pi_fine, engine.count_projected_pi_signed_fine, "pi_edges", args.pi_max
                oracle = proj_signed_oracle.proj_pi_signed_cells
                to_library = lambda edges: edges
            else:
                sibling, signed, key, top = engine.count_smu_fine, engine.count_smu_signed_fine, "mu_edges", 1.0
                oracle = smu_signed_oracle.smu_signed_cells
                to_library = smu_signed_oracle.signed_squares
            half = np.linspace(0.0, top, n + 1)
            if lds_bytes(n_edges, n) > 65536:
                print(f"{n} {kind} bins do not fit at {n_edges} edges: skipped", flush=True)
                continue
            W_u, stats_u, t_u = timed(sibling, **{key: half})
            W_s, stats_s, t_s = timed(signed, **{key: np.linspace(-top, top, n + 1)})
            checked, worst = against_oracle(W_s, oracle, to_library(np.linspace(-top, top, n + 1)))
            line = dict(**({"label": args.label} if args.label else {}), kind=kind, n=n, objects_per_catalogue=n_obj, patches=args.patches, bins=nb,
                        jobs=int(len(jobs)), cells=int(len(cells)), fine_bins=n_edges - 1, rmin_kpc=args.rmin, rmax_kpc=rmax,
                        sort_axis=int(links.sort_axis), candidate_pairs=int(stats_s.candidate_pairs), evaluated=int(stats_s.evaluated_pairs),
                        evaluated_sibling=int(stats_u.evaluated_pairs), unsigned_n=t_u, signed_n=t_s,
                        ratio_equal_planes=round(t_s["ms"] / t_u["ms"], 4), weight_unsigned=float(W_u.sum()), weight_signed_n=float(W_s.sum()),
                        lds_bytes_n=lds_bytes(n_edges, n), cells_checked=checked, worst_difference_over_A=worst, repeat=args.repeat,
                        source_sha16=source_sha16())
            if kind == "pi":
                line["pi_max_mpc"] = args.pi_max
            if lds_bytes(n_edges, 2 * n) <= 65536:  # the mirrored set: 2 n signed bins against n unsigned
                both = proj_signed_oracle.mirrored(half)
                W_m, _, t_m = timed(signed, **{key: both})
                folded = proj_signed_oracle.fold(W_m)
                bound = 1e-10 * np.maximum(np.abs(W_u), np.abs(folded))
                if not np.all(np.abs(folded - W_u) <= bound):
                    raise SystemExit(f"{kind}, {2 * n} signed bins: the folded planes differ from the sibling's")
                line.update(signed_2n=t_m, ratio_mirrored=round(t_m["ms"] / t_u["ms"], 4), lds_bytes_2n=lds_bytes(n_edges, 2 * n),
                            weight_signed_2n=float(W_m.sum()))
            text = json.dumps(line)
            print(text, flush=True)
            with open(args.out, "a") as f:
                f.write(text + "\n")


if __name__ == "__main__":
    main()
