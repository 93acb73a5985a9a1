#!/usr/bin/env python3
"""Timing probe (not a test): HistData.from_catalog's device histogram against the reference-style numpy loop.

Per size (weighted, 64 patches, 30 bins): the wall time of ``engine.redshift_histogram`` (the call HistData.from_catalog
makes, after a warm-up call), split into the host-to-device copy of the columns and the rest (kernels, partial
copy-back, host sum) by a run with the same columns that only copies them; and the reference's loop (one np.histogram
per patch, redshifts.py:44-57) on the same host, one thread. Prints one JSON line per size, with the copy rate in GB/s and
the hash of the kernel sources it ran (profiles/histdata_probe.jsonl holds the committed run).

Usage:  python tools/probe_histdata.py [--sizes 1e6,1e7,1e8] [--repeat 3]
"""
from __future__ import annotations

import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402  (device copy timing only)

from yet_another_wizz_amd import engine  # noqa: E402
from yet_another_wizz_amd.build import source_sha16  # noqa: E402


def numpy_loop(z, w, offsets, edges):
    out = np.empty((len(offsets) - 1, len(edges) - 1))
    for p, (lo, hi) in enumerate(zip(offsets[:-1], offsets[1:])):
        zp, wp = z[lo:hi], w[lo:hi]
        mask = zp > edges[0]
        out[p] = np.histogram(zp[mask], edges, weights=wp[mask])[0]
    return out


def best(fn, repeat):
    times = []
    for _ in range(repeat):
        t0 = time.perf_counter()
        fn()
        times.append(time.perf_counter() - t0)
    return min(times)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", default="1e6,1e7,1e8")
    ap.add_argument("--repeat", type=int, default=3)
    args = ap.parse_args()
    rng = np.random.default_rng(1)
    edges = np.linspace(0.07, 1.43, 31)
    for n in (int(float(s)) for s in args.sizes.split(",")):
        z = rng.uniform(0.0, 1.5, n)
        w = rng.uniform(0.5, 1.5, n)
        offsets = np.linspace(0, n, 65).astype(np.int64)
        call = lambda: engine.redshift_histogram(z, w, offsets, edges, True)  # noqa: E731
        got = call()  # warm-up (context, code objects)
        t_gpu = best(call, args.repeat)
        dev = torch.device("cuda", engine.default_devices()[0])
        bufs = [torch.empty(min(n, 1 << 23), dtype=torch.float64, device=dev) for _ in range(2)]

        def copy_only():
            for lo in range(0, n, 1 << 23):
                hi = min(n, lo + (1 << 23))
                for col, buf in zip((z, w), bufs):
                    buf[: hi - lo].copy_(torch.from_numpy(col[lo:hi]))
            torch.cuda.synchronize(dev)

        copy_only()
        t_copy = best(copy_only, args.repeat)
        t_np = best(lambda: numpy_loop(z, w, offsets, edges), 1 if n >= 10**8 else args.repeat)
        ok = bool(np.allclose(got, numpy_loop(z, w, offsets, edges), rtol=1e-10, atol=1e-12 * w.sum())) if n <= 10**7 else None
        copy_bytes = 2 * 8 * n  # z and w, float64
        print(json.dumps(dict(n=n, patches=64, bins=30, weighted=True, gpu_s=round(t_gpu, 5), copy_s=round(t_copy, 5),
                              copy_bytes=copy_bytes, copy_gbps=round(copy_bytes / t_copy / 1e9, 1),
                              call_gbps=round(copy_bytes / t_gpu / 1e9, 1),
                              kernels_and_rest_s=round(max(t_gpu - t_copy, 0.0), 5), numpy_s=round(t_np, 4),
                              speedup=round(t_np / t_gpu, 1), agrees_with_numpy=ok, device=torch.cuda.get_device_name(dev),
                              source_sha16=source_sha16())), flush=True)
        del bufs


if __name__ == "__main__":
    main()
