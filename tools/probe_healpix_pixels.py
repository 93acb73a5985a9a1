#!/usr/bin/env python3
"""Timing probe (not a test): the unmasked pixels of a HEALPix scalar map on the device route against the numpy route on the
same host.

Per setting: the wall time of ``engine.healpix_pixels`` (the call ``healpix.map_pixels`` makes: the host's count of the
selected pixels, the upload of the maps, the passes and the copies back; median of ``--repeat`` after a warm-up call), the
part of it that is the host's count, the time of a run that only moves the same bytes (the maps to the device, the selected
columns back) and its share of the call, and the numpy route (``healpix._host_map_pixels``) on the same maps -- once from
order 11 on, else the median of ``--repeat``. Prints one JSON line per setting, with whether the two routes returned the same
columns and the hash of the kernel sources (profiles/healpix_pixels_probe.jsonl holds the committed run). It is also
the only place where maps of order 12 and 13 (1.6 and 6.4 GB) run.

Usage:  python tools/probe_healpix_pixels.py --nside 256,1024,4096 --masked-fraction 0.5 --repeat 5 [--weights] [--ring]
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


def median(fn, repeat):
    times = []
    for _ in range(repeat):
        t0 = time.perf_counter()
        fn()
        times.append(time.perf_counter() - t0)
    return statistics.median(times)


def make_map(npix, masked_fraction, rng, step=1 << 24):
    """A map of normal values with ``masked_fraction`` of the pixels UNSEEN, filled in blocks."""
    values = np.empty(npix)
    for lo in range(0, npix, step):
        part = rng.normal(size=min(step, npix - lo))
        part[rng.random(len(part)) < masked_fraction] = healpix.UNSEEN
        values[lo : lo + step] = part
    return values


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--nside", default="1024", help="comma-separated")
    ap.add_argument("--masked-fraction", type=float, default=0.5)
    ap.add_argument("--weights", action="store_true", help="with a weight map (a tenth of its pixels empty)")
    ap.add_argument("--ring", action="store_true")
    ap.add_argument("--repeat", type=int, default=5)
    args = ap.parse_args()
    nested = not args.ring
    rng = np.random.default_rng(1)
    for nside in (int(s) for s in args.nside.split(",")):
        order = healpix.nside2order(nside)
        npix = 12 << (2 * order)
        values = make_map(npix, args.masked_fraction, rng)
        weights = None
        if args.weights:
            weights = rng.uniform(0.5, 1.5, npix)
            weights[:: 10] = 0.0
        maps = [m for m in (values, weights) if m is not None]

        def device_route():
            return engine.healpix_pixels(values, weights, order, nested)

        def host_route():
            return healpix._host_map_pixels(order, values, weights, nested)

        got = device_route()  # warm-up (context, code objects)
        if got is None:
            raise SystemExit("no GPU: nothing to compare")
        n_sel = len(got[0])
        t_dev = median(device_route, args.repeat)
        t_count = median(lambda: healpix.count_selected(values, weights), args.repeat)
        dev = torch.device("cuda", engine.default_devices()[0])
        bufs = [torch.empty(npix, dtype=torch.float64, device=dev) for _ in maps]
        outs = [torch.zeros(n_sel, dtype=torch.float64, device=dev) for _ in range(4 + len(maps) - 1)]  # int64 ipix: as many bytes

        def copy_only():
            for m, buf in zip(maps, bufs):
                buf.copy_(torch.from_numpy(m))
            for out in outs:
                out.cpu()
            torch.cuda.synchronize(dev)

        copy_only()
        t_copy = median(copy_only, args.repeat)
        del bufs, outs
        t0 = time.perf_counter()
        expect = host_route()
        t_host = time.perf_counter() - t0
        if order < 11:
            t_host = statistics.median([t_host] + [median(host_route, 1) for _ in range(args.repeat - 1)])
        agree = all((a is None and b is None) or np.array_equal(a, b) for a, b in zip(got, expect))
        agree = agree and np.array_equal(got[1].view(np.int64), expect[1].view(np.int64)) and \
            np.array_equal(got[2].view(np.int64), expect[2].view(np.int64))
        copy_bytes = 8 * npix * len(maps) + 8 * n_sel * (4 + len(maps) - 1)
        print(json.dumps(dict(nside=nside, npix=npix, selected=n_sel, masked_fraction=args.masked_fraction, nested=nested,
                              weighted=weights is not None, device_s=round(t_dev, 5), host_count_s=round(t_count, 5),
                              host_s=round(t_host, 4), speedup=round(t_host / t_dev, 1), copy_s=round(t_copy, 5),
                              copy_share=round(min(t_copy / t_dev, 1.0), 3), copy_bytes=copy_bytes, routes_agree=bool(agree),
                              repeat=args.repeat, device=torch.cuda.get_device_name(dev), source_sha16=source_sha16())), flush=True)
        del got, expect, values, weights, maps


if __name__ == "__main__":
    main()
