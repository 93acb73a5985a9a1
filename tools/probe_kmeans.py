#!/usr/bin/env python3
"""Timing probe (not a test): patch centres for ``patch_num=`` by the three ways the package has.

Per (n, patches) setting, on points uniform in a cap of 60 degrees (weights ~ U(0.5, 1.5) with ``--weights``):

* ``full``   ``patches.centers_from_xyz`` on the device route: upload, seeding and Lloyd rounds apart (``open_s``, ``seed_s``,
             ``lloyd_s`` of its info), medians of ``--repeat`` runs after a warm-up run;
* ``numpy``  the same function on the numpy route, once, where a cost estimate from the device run's rounds says it ends
             within a minute (else null);
* ``probe``  today's default: ``catalog.kmeans_centers`` on the probe slice ``Catalog.from_arrays`` takes
             (``100 000 sqrt(patches)`` objects), median of ``--repeat`` runs when the first takes under five seconds, else
             that one run.

Also the smallest and largest patch (objects nearest to each centre) of the ``full`` and the ``probe`` centres, and whether
the two routes of ``full`` returned the same centres. Prints one JSON line per setting and appends it to ``--out``
(profiles/kmeans_probe.jsonl holds the committed run, if there is one).

Usage:  python tools/probe_kmeans.py --n 1e6,1e7,1e8 --patches 64,1024 --repeat 5 [--weights]
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

from yet_another_wizz_amd import _lib, catalog, patches  # noqa: E402
from yet_another_wizz_amd.build import source_sha16  # noqa: E402


def spread(xyz, centers):
    sizes = np.bincount(catalog.nearest_center(xyz, centers.to_3d()), minlength=len(centers))
    return int(sizes.min()), int(sizes.max())


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", default="1e6", help="comma-separated object counts")
    ap.add_argument("--patches", default="64", help="comma-separated")
    ap.add_argument("--repeat", type=int, default=5)
    ap.add_argument("--weights", action="store_true")
    ap.add_argument("--max-iterations", type=int, default=100)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "kmeans_probe.jsonl"))
    args = ap.parse_args()
    if _lib.device_count() < 1:
        raise SystemExit("no GPU: nothing to compare")
    rng = np.random.default_rng(1)
    for n in (int(float(s)) for s in args.n.split(",")):
        ra = rng.uniform(0.0, 2.0 * np.pi, n)
        dec = np.arcsin(rng.uniform(0.5, 1.0, n))
        weights = rng.uniform(0.5, 1.5, n) if args.weights else None
        xyz = catalog.radec_to_xyz(ra, dec)
        for k in (int(s) for s in args.patches.split(",")):
            def full():
                return patches.centers_from_xyz(xyz, weights, k, max_iterations=args.max_iterations, return_info=True)

            saved, patches.DEVICE_KMEANS_MIN = patches.DEVICE_KMEANS_MIN, 0
            try:
                dev, info = full()  # warm-up (context, code objects)
                runs = []
                for _ in range(args.repeat):
                    t0 = time.perf_counter()
                    _, timed = full()
                    runs.append((time.perf_counter() - t0, timed["open_s"], timed["seed_s"], timed["lloyd_s"]))
            finally:
                patches.DEVICE_KMEANS_MIN = saved
            if info["route"] != "device":
                raise SystemExit(f"{k} patches did not take the device route")
            total_s, open_s, seed_s, lloyd_s = (statistics.median(col) for col in zip(*runs))
            # numpy: a pass over n objects per seed, n k distances per round (5 ns and 1 ns each with the host pool's 16 threads)
            estimate = 5e-9 * n * k + 1e-9 * n * k * info["iterations"]
            numpy_s = numpy_seed_s = numpy_lloyd_s = agree = None
            if estimate < 60.0:
                patches.DEVICE_KMEANS_MIN = 1 << 62
                try:
                    t0 = time.perf_counter()
                    host, host_info = full()
                    numpy_s = time.perf_counter() - t0
                finally:
                    patches.DEVICE_KMEANS_MIN = saved
                numpy_seed_s, numpy_lloyd_s = host_info["seed_s"], host_info["lloyd_s"]
                agree = bool(np.array_equal(host.data, dev.data) and host_info["inertia"] == info["inertia"])
            probe_size = int(100_000 * np.sqrt(k))
            step = max(1, n // probe_size)
            probe_xyz = np.column_stack([c[::step] for c in xyz])
            probe_w = None if weights is None else weights[::step]
            t0 = time.perf_counter()
            probe = catalog.kmeans_centers(probe_xyz, probe_w, k)
            probe_s = time.perf_counter() - t0
            if probe_s < 5.0:
                more = []
                for _ in range(args.repeat - 1):
                    t0 = time.perf_counter()
                    catalog.kmeans_centers(probe_xyz, probe_w, k)
                    more.append(time.perf_counter() - t0)
                probe_s = statistics.median([probe_s] + more)
            line = dict(n=n, patches=k, weighted=weights is not None, iterations=info["iterations"], converged=info["converged"],
                        step_path=info["step_path"], full_s=round(total_s, 4), open_s=round(open_s, 4), seed_s=round(seed_s, 4),
                        lloyd_s=round(lloyd_s, 4), lloyd_round_ms=round(1e3 * lloyd_s / max(info["iterations"], 1), 3),
                        numpy_s=None if numpy_s is None else round(numpy_s, 3),
                        numpy_seed_s=None if numpy_seed_s is None else round(numpy_seed_s, 3),
                        numpy_lloyd_s=None if numpy_lloyd_s is None else round(numpy_lloyd_s, 3), routes_agree=agree,
                        probe_objects=len(probe_xyz), probe_s=round(probe_s, 3), full_sizes=spread(xyz, dev),
                        probe_sizes=spread(xyz, probe), repeat=args.repeat, source_sha16=source_sha16())
            text = json.dumps(line)
            print(text, flush=True)
            os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
            with open(args.out, "a") as f:
                f.write(text + "\n")


if __name__ == "__main__":
    main()
