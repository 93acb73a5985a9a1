"""Timing of BoxRandoms catalogues, device route against host route: the draw stage (``engine.draw_box_randoms`` against
the generator called chunk by chunk) and the whole ``Catalog.from_random``, with weights and redshifts drawn from attached
values. Every time is a host clock around work that ends in a device synchronise (the library waits for its stream
before it returns). Prints one JSON line; also checks that both routes drew the same columns.

    python tools/probe_randoms.py --n 1e7 1e8 --data 1e7
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
from yet_another_wizz_amd.randoms import BoxRandoms  # noqa: E402


def host_draw(gen, num, chunksize):
    chunks = [gen(min(chunksize, num - lo)) for lo in range(0, num, chunksize)]
    return [np.concatenate([c[k] for c in chunks]) for k in ("ra", "dec", "weights", "redshifts")]


def clock(fn):
    gc.collect()
    t0 = time.perf_counter()
    out = fn()
    return time.perf_counter() - t0, out


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--n", type=float, nargs="+", default=[1e7, 1e8], help="randoms per catalogue")
    ap.add_argument("--data", type=float, default=1e7, help="attached weights / redshifts to draw from")
    ap.add_argument("--patches", type=int, default=64)
    args = ap.parse_args()
    if _lib.device_count() < 1:
        raise SystemExit("probe_randoms: no GPU")
    rng = np.random.default_rng(1)
    n_data = int(args.data)
    gen = BoxRandoms(0.0, 90.0, -30.0, 30.0, weights=rng.uniform(0.5, 1.5, n_data), redshifts=rng.uniform(0.05, 1.5, n_data),
                     seed=12345)
    side = int(np.sqrt(args.patches))
    ra, dec = np.meshgrid(np.linspace(5.0, 85.0, side), np.linspace(-25.0, 25.0, args.patches // side))
    centres = yaw.AngularCoordinates(np.deg2rad(np.column_stack([ra.ravel(), dec.ravel()])))
    gen.reseed()
    engine.draw_box_randoms(gen, 1000, RANDOM_CHUNKSIZE)  # context, code objects
    result = dict(probe="randoms", data=n_data, chunksize=RANDOM_CHUNKSIZE, patches=len(centres), runs=[])
    for num in (int(v) for v in args.n):
        run = dict(n=num)
        gen.reseed()
        t, ((x, y, w, z), _) = clock(lambda: engine.draw_box_randoms(gen, num, RANDOM_CHUNKSIZE))
        run["device_draw_s"] = t
        run["device_bytes_to_host"] = sum(c.nbytes for c in (x, y, w, z))
        gen.reseed()
        t, (hra, hdec, hw, hz) = clock(lambda: host_draw(gen, num, RANDOM_CHUNKSIZE))
        run["host_draw_s"] = t
        run["draws_identical"] = bool(np.array_equal(x, hra) and np.array_equal(w, hw) and np.array_equal(z, hz)
                                      and np.array_equal(np.arcsin(y), hdec))
        del x, y, w, z, hra, hdec, hw, hz
        t, cat = clock(lambda: yaw.Catalog.from_random(None, gen, num, patch_centers=centres))
        assert cat._random_route == "device"
        run["device_from_random_s"] = t
        del cat
        drawn, engine.draw_box_randoms = engine.draw_box_randoms, lambda *a, **k: None
        try:
            t, cat = clock(lambda: yaw.Catalog.from_random(None, gen, num, patch_centers=centres))
        finally:
            engine.draw_box_randoms = drawn
        assert cat._random_route == "host"
        run["host_from_random_s"] = t
        del cat
        run["draw_speedup"] = run["host_draw_s"] / run["device_draw_s"]
        run["device_draw_effective_GBps"] = run["device_bytes_to_host"] / run["device_draw_s"] / 1e9
        result["runs"].append(run)
    print(json.dumps(result))


if __name__ == "__main__":
    main()
