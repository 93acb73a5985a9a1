#!/usr/bin/env python3
"""Timing probe (not a test): the HEALPix map of n points on the device route against the numpy route on the same host.

Per size: the wall time of ``engine.healpix_map`` (the call ``healpix.healpix_map`` makes; median of ``--repeat`` after a
warm-up call), the time of a run that only moves the same bytes (the columns to the device in the library's passes, the map
back) and its share of the call, and the numpy route (``ang2pix`` + ``np.bincount``) on the same inputs -- once from 1e8
points on, else the median of ``--repeat``. With ``--pixels`` the call returns the pixels instead of the map
(``healpix.ang2pix``). Prints one JSON line per size, with whether the two routes returned the same array and the hash of the
kernel sources (profiles/healpix_map_probe.jsonl holds the committed run).

Usage:  python tools/probe_healpix_map.py --nside 1024 --n 1e7,1e8 --repeat 5 [--weights] [--pixels] [--ring]
"""
from __future__ import annotations

import argparse
import json
import os
import statistics
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402  (device copy timing only)

from yet_another_wizz_amd import engine, healpix  # noqa: E402
from yet_another_wizz_amd.build import source_sha16  # noqa: E402

PASS = 1 << 24  # the library's default pass


def median(fn, repeat):
    times = []
    for _ in range(repeat):
        t0 = time.perf_counter()
        fn()
        times.append(time.perf_counter() - t0)
    return statistics.median(times)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--nside", type=int, default=1024)
    ap.add_argument("--n", default="1e7")
    ap.add_argument("--repeat", type=int, default=5)
    ap.add_argument("--weights", action="store_true")
    ap.add_argument("--pixels", action="store_true", help="time ang2pix (pixels out) instead of the map")
    ap.add_argument("--ring", action="store_true")
    args = ap.parse_args()
    order = healpix.nside2order(args.nside)
    npix = 12 << (2 * order)
    nested = not args.ring
    rng = np.random.default_rng(1)
    for n in (int(float(s)) for s in args.n.split(",")):
        phi = rng.uniform(0.0, 2.0 * np.pi, n)
        z = rng.uniform(-1.0, 1.0, n)
        w = rng.uniform(0.5, 1.5, n) if args.weights and not args.pixels else None
        cols = [c for c in (phi, z, w) if c is not None]

        def device_route():
            return engine.healpix_map(phi, z, w, order, nested, want_pixels=args.pixels, want_map=not args.pixels)[0 if args.pixels else 1]

        def host_route():
            pix = healpix._host_pixels(order, phi, z, nested)
            return pix if args.pixels else np.bincount(pix, w, minlength=npix).astype(np.float64, copy=False)

        got = device_route()  # warm-up (context, code objects)
        t_dev = median(device_route, args.repeat)
        dev = torch.device("cuda", engine.default_devices()[0])
        bufs = [torch.empty(min(n, PASS), dtype=torch.float64, device=dev) for _ in cols]
        out_dev = torch.zeros(n if args.pixels else npix, dtype=torch.int64 if args.pixels else torch.float64, device=dev)

        def copy_only():
            for lo in range(0, n, PASS):
                hi = min(n, lo + PASS)
                for col, buf in zip(cols, bufs):
                    buf[: hi - lo].copy_(torch.from_numpy(col[lo:hi]))
            out_dev.cpu()
            torch.cuda.synchronize(dev)

        copy_only()
        t_copy = median(copy_only, args.repeat)
        t0 = time.perf_counter()
        expect = host_route()
        t_host = time.perf_counter() - t0
        if n < 10**8:
            t_host = statistics.median([t_host] + [median(host_route, 1) for _ in range(args.repeat - 1)])
        copy_bytes = 8 * n * len(cols) + out_dev.numel() * 8
        print(json.dumps(dict(n=n, nside=args.nside, nested=nested, weighted=w is not None, out="pixels" if args.pixels else "map",
                              device_s=round(t_dev, 5), host_s=round(t_host, 4), speedup=round(t_host / t_dev, 1),
                              copy_s=round(t_copy, 5), copy_share=round(min(t_copy / t_dev, 1.0), 3), copy_bytes=copy_bytes,
                              routes_agree=bool(np.array_equal(got, expect)), repeat=args.repeat,
                              device=torch.cuda.get_device_name(dev), source_sha16=source_sha16())), flush=True)
        del bufs, out_dev, got, expect


if __name__ == "__main__":
    main()
