#!/usr/bin/env python3
"""Timing probe (not a test): scalar-field correlations at the headline size.

The headline workload's columns (full sky, 64 patches, 30 redshift bins; seeds 101 / 202) with kappa ~ N(0, 1) on the
reference sample. Prints JSON lines with the hash of the kernel sources they ran:

  upload   the binned reference layout through ``yawhip_catalog_upload_scalar`` (one call, two catalogues) against two
           plain ``yawhip_catalog_upload_axis`` calls of the same columns (weights w, weights kappa * w formed by numpy
           beforehand, not timed), per repeat on a fresh context-resident state (catalogues freed in between); and one plain
           upload alone. Best of ``--repeat``. ``saving_ms`` = two plain uploads - the scalar upload. ``coord_copy_ms`` is a
           bare host-to-device copy of the three coordinate columns from the same (pageable) numpy memory, for scale: the
           call saves that copy and one segmented sort (the sort's own time: ``rocprofv3 --kernel-trace --stats -- python
           tools/probe_scalar.py --upload-only``).
  measure  ``crosscorrelate_scalar(config, ref, unk)`` cold (first call: build_trees, uploads, counts, normalisation) and
           warm (further calls on the resident catalogues), the count kernels' own times of a warm scalar count
           (``last_batch_stats``), and for comparison the warm wall time of the two-request scalar count and of the plain
           "nn" ``count_pairs`` alone.

Usage:  python tools/probe_scalar.py [--n-ref 1e7] [--n-unk 1e7] [--repeat 3] [--weights] [--upload-only]
"""
from __future__ import annotations

import argparse
import json
import os
import sys
import time

import numpy as np
import torch  # (device copy timing only)

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import yet_another_wizz_amd as yaw  # noqa: E402
from yet_another_wizz_amd import _lib, engine  # noqa: E402
from yet_another_wizz_amd.build import source_sha16  # noqa: E402


def fibonacci_centers(num):
    i = np.arange(num) + 0.5
    return np.column_stack([(np.pi * (1.0 + 5.0**0.5) * i) % (2.0 * np.pi), np.arcsin(1.0 - 2.0 * i / num)])


def uniform_sky(seed, n):
    rng = np.random.default_rng(seed)
    return rng.uniform(0.0, 2.0 * np.pi, n), np.arcsin(rng.uniform(-1.0, 1.0, n)), rng


def timed(fn):
    t0 = time.perf_counter()
    out = fn()
    return out, (time.perf_counter() - t0) * 1e3


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n-ref", type=float, default=1e7)
    ap.add_argument("--n-unk", type=float, default=1e7)
    ap.add_argument("--patches", type=int, default=64)
    ap.add_argument("--zbins", type=int, default=30)
    ap.add_argument("--repeat", type=int, default=3)
    ap.add_argument("--weights", action="store_true", help="w ~ U(0.5, 1.5) on both catalogues (the twin is weighted either way)")
    ap.add_argument("--upload-only", action="store_true", help="stop after the upload comparison (for a kernel trace)")
    args = ap.parse_args()
    common = dict(n_ref=int(args.n_ref), n_unk=int(args.n_unk), patches=args.patches, zbins=args.zbins, weights=args.weights,
                  source_sha16=source_sha16())
    centers = yaw.AngularCoordinates(fibonacci_centers(args.patches))
    ra, dec, rng = uniform_sky(101, int(args.n_ref))
    z, w = rng.uniform(0.1, 1.0, len(ra)), (rng.uniform(0.5, 1.5, len(ra)) if args.weights else None)
    kappa = rng.normal(0.0, 1.0, len(ra))
    ref = yaw.Catalog.from_arrays(ra, dec, redshifts=z, weights=w, kappa=kappa, patch_centers=centers, degrees=False)
    ra, dec, rng = uniform_sky(202, int(args.n_unk))
    unk = yaw.Catalog.from_arrays(ra, dec, weights=rng.uniform(0.5, 1.5, len(ra)) if args.weights else None,
                                  patch_centers=centers, degrees=False)
    config = yaw.Configuration.create(rmin=1.0, rmax=10.0, unit="arcmin", zmin=0.1, zmax=1.0, num_bins=args.zbins)

    # ---- upload: one scalar upload against two plain ones, the same layout, the same context and strip grid
    layout = ref.build_trees(config.binning.edges, closed=config.binning.closed)
    ctx = engine.get_context()
    common["devices"] = len(ctx.devices)  # (a context of several devices replicates every upload)
    product = layout.kappa * layout.w if layout.w is not None else layout.kappa.copy()
    shape = (layout.num_patches, layout.num_bins, layout.offsets)

    def plain(weights):
        return _lib.DeviceCatalog(ctx, layout.x, layout.y, layout.z, weights, *shape)

    def scalar():
        return _lib.DeviceCatalog.upload_scalar(ctx, layout.x, layout.y, layout.z, layout.w, layout.kappa, *shape)

    dev = torch.device("cuda", ctx.devices[0])
    bufs = [torch.empty(len(layout.x), dtype=torch.float64, device=dev) for _ in range(3)]

    def coord_copy():
        for buf, column in zip(bufs, (layout.x, layout.y, layout.z)):
            buf.copy_(torch.from_numpy(column))
        torch.cuda.synchronize(dev)

    for cat in scalar():  # warm-up: code objects, sort workspace
        cat.free()
    coord_copy()
    t_scalar, t_two, t_one, t_copy = [], [], [], []
    for _ in range(args.repeat):
        cats, ms = timed(scalar)
        t_scalar.append(ms)
        bytes_scalar = sum(c.device_bytes for c in cats)
        for cat in cats:
            cat.free()
        cats, ms = timed(lambda: (plain(layout.w), plain(product)))
        t_two.append(ms)
        bytes_two = sum(c.device_bytes for c in cats)
        for cat in cats:
            cat.free()
        cat, ms = timed(lambda: plain(layout.w))
        t_one.append(ms)
        cat.free()
        t_copy.append(timed(coord_copy)[1])
    del bufs
    print(json.dumps(dict(what="upload", objects_kept=int(layout.num_records), scalar_upload_ms=round(min(t_scalar), 2),
                          two_plain_uploads_ms=round(min(t_two), 2), one_plain_upload_ms=round(min(t_one), 2),
                          saving_ms=round(min(t_two) - min(t_scalar), 2), coord_copy_ms=round(min(t_copy), 2),
                          all_one_plain_ms=[round(t, 2) for t in t_one], all_scalar_ms=[round(t, 2) for t in t_scalar],
                          all_two_plain_ms=[round(t, 2) for t in t_two], device_bytes_scalar=bytes_scalar,
                          device_bytes_two_plain=bytes_two, **common)), flush=True)

    if args.upload_only:
        return

    # ---- the measurement: cold, then warm
    ref.drop_layouts()
    cfs, cold = timed(lambda: yaw.crosscorrelate_scalar(config, ref, unk))
    warm = []
    for _ in range(args.repeat):
        cfs, ms = timed(lambda: yaw.crosscorrelate_scalar(config, ref, unk))
        warm.append(ms)
    links = yaw.PatchLinkage.from_catalogs(config, ref, unk)
    links.count_scalar_pairs(ref, unk, mode="kn", count_type_info="DD")
    stats = {name: dict(count_ms=round(st.count_ms, 4), kernel_ms=round(st.kernel_ms, 4), variants=sorted(st.variants))
             for name, st in links.last_batch_stats.items()}
    links.count_pairs(ref, unk)
    nn_alone = min(timed(lambda: links.count_pairs(ref, unk))[1] for _ in range(max(args.repeat, 3)))
    pair = min(timed(lambda: links.count_scalar_pairs(ref, unk, mode="kn"))[1] for _ in range(max(args.repeat, 3)))
    print(json.dumps(dict(what="measure", cold_ms=round(cold, 1), warm_ms=round(min(warm), 3), all_warm_ms=[round(t, 3) for t in warm],
                          warm_scalar_pair_counts_ms=round(pair, 3), warm_nn_count_alone_ms=round(nn_alone, 3), batch_stats=stats,
                          finite=bool(np.all(np.isfinite(cfs[0].sample().data))), **common)), flush=True)


if __name__ == "__main__":
    main()
