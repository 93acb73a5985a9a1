"""The per-item path of the float32 band kernels (csrc/yawhip_band32.inc, csrc/yawhip_kernel_fine.hip) -- lane records, cap
bounds, band search, statistics -- on two small scenes.

* the scene of tests/test_gpu_band_walk_trips.py: bands of 0-3 entries, shared-out tiles, the 75-object tile with one object
  in the last occupied lane, windows of 319 / 511 / 700 entries, tied keys;
* a scene of STATIONS, a little over 2 000 objects. A station is a handful of lane objects and their partners within an
  arcminute, alone in a strip of its own (four grid cells from the next station): its lane objects are one strip run -- lane
  tiles of exactly that many objects -- and its partners are the whole merged window of those tiles. Stations have 1, 2, 3,
  127, 128 and 129 lane objects (a second tile of one object at two objects per lane) and windows of 1, 2, 3, 4, 5, 63, 64,
  65, 255, 256 and 257 entries: around every power of two, where the halving search of the bands changes its number of steps.
  The lane objects of a station take the bins 0, 1, 2, 0, ... in the order of their keys, so every lane that holds two or four
  objects holds objects of different bins, all three with four. Two more stations sit on the poles of the sort axis: lane
  keys within 2e-7 of -1 and +1 (and so of -/+ cos theta of every grid here), the clip branches of the float32 cap bounds.
  These cases run with `auto_orient` off, on the layouts of the catalogues' own sort axis z -- with it the polar patches
  would be counted on another axis and the keys would be nowhere near 1.

Every case runs one object per lane (pairs of entries per trip, half bands on a self count), two and four, unweighted and
weighted (one call returns counts and sums: both launches), one threshold row and a row per bin, in the one-chunk, the
three-chunk and the fine-grid kernel. Against the oracle: counts bit for bit, weighted sums to 1e-10 relative. And against
tests/golden/lane_image.npz (tools/make_golden_lane_image.py, recorded from the build before the per-item path was changed):
`evaluated_pairs` and `exact_reevaluations` -- the bands are culling bounds, so the same entries must be walked and the same
evaluations settled exactly.
"""
from __future__ import annotations

import functools

import numpy as np
import pytest

import test_gpu_band_walk_trips as walk
import test_gpu_count_variants as table
from conftest import ARCMIN, load_golden
from oracle import oracle

pytestmark = pytest.mark.gpu
RTOL_W = 1e-10

B, P = table.B, table.P
JOBS, PAIRS = table.JOBS, table.PAIRS
GRIDS = {**walk.GRIDS, "fine": np.geomspace(0.1, 1.0, 8)}  # edges in arcmin; eight edges: the fine-grid kernel
R_MAX = walk.R_MAX
CELL = 2e-3                      # strip grid of the table (STRIP_MICRO)
STATION_LANES = (1, 2, 3, 127, 128, 129, 5, 7, 9, 11, 13)
STATION_WINDOW = (257, 256, 255, 1, 2, 3, 4, 5, 63, 64, 65)
POLE_LANES, POLE_WINDOW = 6, 40


def angles(grid: str) -> np.ndarray:
    name, _, per_bin = grid.partition("/")
    row = GRIDS[name] * ARCMIN
    return np.stack([row * (walk.BIN_SCALE[k] if per_bin else 1.0) for k in range(B)])


def thresholds(grid: str) -> np.ndarray:
    return np.stack([oracle.thresholds_for(a) for a in angles(grid)])


def station_y(j: int) -> float:
    """The middle of a cell of the latitude grid about the strip axis y, four cells from the next station's."""
    return float(np.sin((250 + 4 * j + 0.5) * CELL))


@functools.lru_cache(maxsize=1)
def _stations():
    rng = np.random.default_rng(20261022)
    lane_xyz, lane_p, lane_rank = [], [], []
    part_xyz, part_p = [], []
    for j, (n_lane, n_win) in enumerate(zip(STATION_LANES, STATION_WINDOW)):
        patch = 0 if j < 6 else 1
        u = np.sort(rng.uniform(-0.2, 0.2, n_lane)) * R_MAX
        v = station_y(j) + rng.uniform(-0.2, 0.2, n_lane) * R_MAX
        lane_xyz += list(walk._unit(u, v)); lane_p += [patch] * n_lane; lane_rank += list(range(n_lane))
        # one partner on the inner edge of the station's first lane object (0.2': it stays in the cell), the others anywhere
        # within reach of some lane object
        first = walk._unit(u[:1], v[:1])[0]
        part_xyz.append(walk._around(first, 0.2 * ARCMIN, 0.5 * np.pi, walk.DELTAS[j % len(walk.DELTAS)]))
        pu = rng.uniform(-0.4, 0.4, n_win - 1) * R_MAX
        pv = station_y(j) + rng.uniform(-0.4, 0.4, n_win - 1) * R_MAX
        part_xyz += list(walk._unit(pu, pv)); part_p += [patch] * n_win
    for patch, pole in ((2, 1.0), (3, -1.0)):  # within 2' of a pole of the sort axis: 1 - |u| < 2e-7
        rho, phi = rng.uniform(0.1, 2.0, POLE_LANES) * ARCMIN, rng.uniform(0.0, 2.0 * np.pi, POLE_LANES)
        xyz = np.column_stack([np.sin(rho) * np.cos(phi), np.sin(rho) * np.sin(phi), pole * np.cos(rho)])
        assert np.all(1.0 - np.abs(xyz[:, 2]) < 2e-7)
        order = np.argsort(xyz[:, 2])
        lane_xyz += list(xyz[order]); lane_p += [patch] * POLE_LANES; lane_rank += list(range(POLE_LANES))
        part_xyz.append(walk._around(xyz[order][0], 0.2 * ARCMIN, 0.5 * np.pi, 1e-12))
        rho, phi = rng.uniform(0.0, 2.6, POLE_WINDOW - 1) * ARCMIN, rng.uniform(0.0, 2.0 * np.pi, POLE_WINDOW - 1)
        part_xyz += list(np.column_stack([np.sin(rho) * np.cos(phi), np.sin(rho) * np.sin(phi), pole * np.cos(rho)]))
        part_p += [patch] * POLE_WINDOW
    lane_xyz, part_xyz = np.array(lane_xyz), np.array(part_xyz)
    lane_p, part_p, lane_rank = np.array(lane_p), np.array(part_p), np.array(lane_rank)
    zedges = np.linspace(0.1, 0.9, B + 1)
    n1, n2 = len(lane_p), len(part_p)
    k1 = lane_rank % B                                    # bins 0, 1, 2, 0, ... along the keys of a station
    z1 = 0.5 * (zedges[k1] + zedges[k1 + 1])
    k2 = np.arange(n2) % B
    z2 = 0.5 * (zedges[k2] + zedges[k2 + 1])
    w1, w2 = 10.0 ** rng.uniform(-2.0, 2.0, n1), 10.0 ** rng.uniform(-2.0, 2.0, n2)
    ra1, dec1 = walk._sky(lane_xyz)
    ra2, dec2 = walk._sky(part_xyz)
    return {
        "c1": oracle.sort_catalog(ra1, dec1, z1, w1, lane_p, P, zedges, "right"),
        "c2b": oracle.sort_catalog(ra2, dec2, z2, w2, part_p, P, zedges, "right"),
        "c2u": oracle.sort_catalog(ra2, dec2, None, w2, part_p, P, None, "right"),
    }


SCENES = {"walk": walk._scene, "stations": _stations}
S32 = {1: 320, 2: 512, 4: 512}   # (objects per lane -> stage) of the cases: k_count_band32 / _one
S64 = {1: 192, 2: 288, 4: 288}   # ... k_count_band32_fine


def _cases():
    """(id, scene, pair, grid, options, (unweighted, weighted) variant)."""
    out = []

    def add(scene, fam, r, pair, grid, triple_runs):
        merged = pair == "cross"
        uni = not (merged and "/bins" in grid)
        cap = (S64 if fam.endswith("_fine") else S32)[r]
        opts = {"kernel": "band", "band_fp32": 1, "triple_runs": triple_runs, "tile_r": r}
        if r == 2:
            opts["band_cap"] = cap
        args = (r, cap, merged, uni) if fam.endswith("_fine") else (r, cap, len(GRIDS[grid.partition("/")[0]]), merged, uni)
        out.append((f"{scene}-{fam}-R{r}-{pair}-{grid}", scene, pair, grid, opts, table._pair_reach(fam, *args)))

    for scene in SCENES:
        for r in (1, 2, 4):
            for per_bin in (False, True):
                grid = "e2" + ("/bins" if per_bin else "")
                add(scene, "k_count_band32_one", r, "cross", grid, 2)
                add(scene, "k_count_band32", r, "cross", grid, 0)
                add(scene, "k_count_band32_fine", r, "cross", "fine" + ("/bins" if per_bin else ""), 2 * (r % 2))
        add(scene, "k_count_band32_one", 1, "self", "e2", 2)     # half bands
        add(scene, "k_count_band32_one", 2, "binned", "e2", 2)   # per-bin items: the kernel ignores the record's bin
        add(scene, "k_count_band32", 1, "binned", "e2", 0)
        add(scene, "k_count_band32_one", 2, "cross", "e3", 2)    # cumulative counters
        add(scene, "k_count_band32", 4, "cross", "e4", 0)
    return out


CASES = _cases()


@pytest.fixture(scope="module")
def devices():
    made = {}

    def get(scene):
        if scene not in made:
            made[scene] = table._Device(0, SCENES[scene]())
        return made[scene]

    yield get
    for d in made.values():
        d.close()


@pytest.fixture(scope="module")
def expected():
    memo = {}

    def get(scene, pair, grid):
        if (scene, pair, grid) not in memo:
            cats = SCENES[scene]()
            a, b = PAIRS[pair]
            memo[(scene, pair, grid)] = oracle.count_jobs(cats[a], cats[b], JOBS, thresholds(grid))
        return memo[(scene, pair, grid)]

    return get


def run_case(d, case):
    """(counts, sums, stats) of a case on the device, the options restored afterwards."""
    from yet_another_wizz_amd import _lib

    _, _, pair, grid, options, _ = case
    a, b = PAIRS[pair]
    try:
        table._apply(d.ctx, {"seg_strips_min_run": 1, "auto_orient": 0, **options})
        return _lib.count_pairs(d.ctx, d.dev[a], d.dev[b], JOBS, thresholds(grid), want_counts=True, want_sums=True)
    finally:
        table._restore(d.ctx)
        d.ctx.set_option("auto_orient", 1)


def test_the_stations_are_what_the_cases_need():
    cats = _stations()
    c1, c2 = cats["c1"], cats["c2u"]
    assert len(c1["x"]) + len(c2["x"]) < 2500
    assert sorted(STATION_LANES)[:6] == [1, 2, 3, 5, 7, 9] and {127, 128, 129} <= set(STATION_LANES)
    assert sorted(STATION_WINDOW) == [1, 2, 3, 4, 5, 63, 64, 65, 255, 256, 257]
    n1 = [c1["off"][(p + 1) * B] - c1["off"][p * B] for p in range(P)]
    assert n1 == [sum(STATION_LANES[:6]), sum(STATION_LANES[6:]), POLE_LANES, POLE_LANES]
    assert list(np.diff(c2["off"])) == [sum(STATION_WINDOW[:6]), sum(STATION_WINDOW[6:]), POLE_WINDOW, POLE_WINDOW]
    # stations four cells apart, every object of a station well inside its cell; the polar keys
    lat = np.arcsin(np.concatenate([c1["y"][: n1[0] + n1[1]], c2["y"][: c2["off"][2]]])) / CELL
    cell = np.floor(lat)
    assert set(cell) == {250 + 4 * j for j in range(len(STATION_LANES))} and np.all(np.abs(lat - cell - 0.5) < 0.2)
    polar = np.abs(c1["z"][n1[0] + n1[1]:])
    assert len(polar) == 2 * POLE_LANES and np.all(1.0 - polar < 2e-7) and np.all(1.0 - np.cos(angles("e2/bins")[:, -1]) < 2e-7)


@pytest.mark.parametrize("case", CASES, ids=[c[0] for c in CASES])
def test_item_path_against_oracle_and_recorded_work(devices, expected, case):
    cid, scene, pair, grid, _, reach = case
    counts, sums, st = run_case(devices(scene), case)
    assert st.variants == set(reach), (cid, st.variants)
    exp_c, exp_s = expected(scene, pair, grid)
    assert exp_c.sum() > 1000, cid
    assert np.array_equal(counts, exp_c), cid
    np.testing.assert_allclose(sums, exp_s, rtol=RTOL_W, atol=0, err_msg=cid)
    recorded = load_golden("lane_image.npz")
    ids = [s.decode() for s in recorded["case"]]
    assert cid in ids, f"{cid}: not in tests/golden/lane_image.npz (tools/make_golden_lane_image.py)"
    i = ids.index(cid)
    print(cid, "evaluated_pairs", st.evaluated_pairs, "exact_reevaluations", st.exact_reevaluations)
    assert st.evaluated_pairs == int(recorded["evaluated_pairs"][i]), cid
    assert st.exact_reevaluations == int(recorded["exact_reevaluations"][i]), cid


def test_lane_records_equal_the_columns():
    """q4[i] == (qx[i], qy[i], qz[i], bin[i]) word for word, and zero records behind the last object: every strip layout of
    a binned and of an unbinned catalogue of 5 000 objects -- three orientations, patch-level and (binned) per-segment.
    The library compares on the host what it reads back from the device (yawhip_debug_lane_image, a test hook)."""
    import ctypes

    from yet_another_wizz_amd import _lib

    lib = _lib.load_library()
    hook = lib.yawhip_debug_lane_image
    hook.restype = ctypes.c_int
    hook.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int32, ctypes.c_int32, ctypes.POINTER(ctypes.c_int64),
                     ctypes.POINTER(ctypes.c_int64)]
    rng = np.random.default_rng(7)
    n = 5000
    ra, dec = np.deg2rad(rng.uniform(30.0, 31.5, n)), np.deg2rad(rng.uniform(-0.75, 0.75, n))
    patch = (ra > np.deg2rad(30.75)).astype(np.int64) + 2 * (dec > 0.0)
    zedges = np.linspace(0.1, 0.9, B + 1)
    cats = {"binned": oracle.sort_catalog(ra, dec, rng.uniform(0.11, 0.89, n), rng.uniform(0.5, 1.5, n), patch, P, zedges, "right"),
            "unbinned": oracle.sort_catalog(ra, dec, None, None, patch, P, None, "right")}
    d = table._Device(0, cats)
    try:
        for name, cat in d.dev.items():
            for seg in ((0, 1) if name == "binned" else (0,)):
                for o in (0, 1, 2):
                    checked, differing = ctypes.c_int64(-1), ctypes.c_int64(-1)
                    rc = hook(d.ctx._h, cat._h, o, seg, ctypes.byref(checked), ctypes.byref(differing))
                    assert rc == 0, (name, seg, o, lib.yawhip_last_error())
                    assert (checked.value, differing.value) == (n, 0), (name, seg, o)
    finally:
        d.close()
