"""Timing of BoxRandoms catalogues, device route against host route: the draw stage (``engine.draw_box_randoms`` against
the generator called chunk by chunk) and the whole ``Catalog.from_random``, with weights and redshifts drawn from attached
values. Every time is a host clock around work that ends in a device synchronise (the library waits for its stream
before it returns). Prints one JSON line; also checks that both routes drew the same columns.

    python tools/probe_randoms.py --n 1e7 1e8 --data 1e7

``--healpix NSIDE`` times HealPixRandoms instead (``engine.draw_healpix_randoms``), on a mask of the box's footprint at that
nside (5 % of the sky); ``--repeat R`` takes the median of R timings of the device-route stages after one untimed call (the host route, seconds
long, is timed once).

    python tools/probe_randoms.py --healpix 1024 --n 1e7 1e8 --repeat 5
"""
import argparse
import gc
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import yet_another_wizz_amd as yaw  # noqa: E402
from yet_another_wizz_amd import _lib, engine  # noqa: E402
from yet_another_wizz_amd.catalog import RANDOM_CHUNKSIZE  # noqa: E402
from yet_another_wizz_amd.randoms import BoxRandoms, HealPixRandoms, pix2loc_nest  # noqa: E402


def host_draw(gen, num, chunksize):
    chunks = [gen(min(chunksize, num - lo)) for lo in range(0, num, chunksize)]
    return [np.concatenate([c[k] for c in chunks]) for k in ("ra", "dec", "weights", "redshifts")]


def clock(fn, repeat=1):
    """Median of ``repeat`` timings of ``fn()`` (one untimed call first if repeat > 1) and the last result."""
    times = []
    for i in range(repeat + (repeat > 1)):
        out = None
        gc.collect()
        t0 = time.perf_counter()
        out = fn()
        if i > 0 or repeat == 1:
            times.append(time.perf_counter() - t0)
    return float(np.median(times)), out


def footprint_mask(nside):
    """Nested mask of the probe's box (ra 0 .. 90, dec -30 .. 30 degrees cut to 5 % of the sky: dec -11.5 .. 11.5)."""
    order = nside.bit_length() - 1
    mask = np.empty(12 * nside * nside)
    step = 1 << 22
    for lo in range(0, len(mask), step):
        phi, z = pix2loc_nest(order, np.arange(lo, min(lo + step, len(mask))))
        mask[lo : lo + step] = (phi < np.pi / 2) & (np.abs(z) < 0.2)
    return mask


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--n", type=float, nargs="+", default=[1e7, 1e8], help="randoms per catalogue")
    ap.add_argument("--data", type=float, default=1e7, help="attached weights / redshifts to draw from")
    ap.add_argument("--patches", type=int, default=64)
    ap.add_argument("--healpix", type=int, default=0, metavar="NSIDE", help="time HealPixRandoms on a mask of this nside")
    ap.add_argument("--repeat", type=int, default=1, help="timings per device-route stage (median; one untimed call first if > 1); the host route is timed once")
    args = ap.parse_args()
    if _lib.device_count() < 1:
        raise SystemExit("probe_randoms: no GPU")
    rng = np.random.default_rng(1)
    n_data = int(args.data)
    attached = dict(weights=rng.uniform(0.5, 1.5, n_data), redshifts=rng.uniform(0.05, 1.5, n_data), seed=12345)
    if args.healpix:
        gen = HealPixRandoms(footprint_mask(args.healpix), nested=True, is_mask=True, **attached)
        draw_name = "draw_healpix_randoms"
    else:
        gen = BoxRandoms(0.0, 90.0, -30.0, 30.0, **attached)
        draw_name = "draw_box_randoms"
    device_draw = getattr(engine, draw_name)
    side = int(np.sqrt(args.patches))
    ra, dec = np.meshgrid(np.linspace(5.0, 85.0, side), np.linspace(-25.0, 25.0, args.patches // side))
    centres = yaw.AngularCoordinates(np.deg2rad(np.column_stack([ra.ravel(), dec.ravel()])))
    gen.reseed()
    device_draw(gen, 1000, RANDOM_CHUNKSIZE)  # context, code objects
    result = dict(probe="randoms", generator=type(gen).__name__, data=n_data, chunksize=RANDOM_CHUNKSIZE, patches=len(centres),
                  repeat=args.repeat, runs=[])
    if args.healpix:
        result.update(nside=args.healpix, unmasked=len(gen._ipix_unmasked))

    def reseeded(fn):
        def call():
            gen.reseed()
            return fn()
        return call

    for num in (int(v) for v in args.n):
        run = dict(n=num)
        t, ((x, y, w, z), _) = clock(reseeded(lambda: device_draw(gen, num, RANDOM_CHUNKSIZE)), args.repeat)
        run["device_draw_s"] = t
        run["device_bytes_to_host"] = sum(c.nbytes for c in (x, y, w, z))
        t, (hra, hdec, hw, hz) = clock(reseeded(lambda: host_draw(gen, num, RANDOM_CHUNKSIZE)))
        run["host_draw_s"] = t
        run["draws_identical"] = bool(np.array_equal(x, hra) and np.array_equal(w, hw) and np.array_equal(z, hz)
                                      and np.array_equal(np.arcsin(y), hdec))
        del x, y, w, z, hra, hdec, hw, hz
        t, cat = clock(lambda: yaw.Catalog.from_random(None, gen, num, patch_centers=centres), args.repeat)
        assert cat._random_route == "device"
        run["device_from_random_s"] = t
        del cat
        setattr(engine, draw_name, lambda *a, **k: None)
        try:
            t, cat = clock(lambda: yaw.Catalog.from_random(None, gen, num, patch_centers=centres))
        finally:
            setattr(engine, draw_name, device_draw)
        assert cat._random_route == "host"
        run["host_from_random_s"] = t
        del cat
        run["draw_speedup"] = run["host_draw_s"] / run["device_draw_s"]
        run["device_draw_effective_GBps"] = run["device_bytes_to_host"] / run["device_draw_s"] / 1e9
        result["runs"].append(run)
    print(json.dumps(result))


if __name__ == "__main__":
    main()
