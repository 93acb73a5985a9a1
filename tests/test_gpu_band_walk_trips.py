"""The walk loop of the float32 band kernels (csrc/yawhip_band32.inc) on the smallest shapes where it can go wrong.

A scene of a few thousand objects, built so that the loop meets, in known places:

* patch 0, the LINE: lane objects in close pairs (the two objects of a lane when two are counted per lane) along the sort
  axis, the pairs further apart than two windows, so that every lane has a band of its own made of the partners placed
  around it -- bands of 0, 1, 2 and 3 entries in turn, the longest band of a wave odd. The partners lie ON an edge of the
  lane object's annulus (within 1e-9 relative, the float32 classes leave three parts in 10^4 undecided at an arcminute):
  below the first object (the first entry of the band: the first trip), above the second (the last trip), on the
  bisector of the pair (both objects of the lane undecided in the same trip) and two of them next to each other along the
  sort axis (two consecutive trips). Then three lane tiles whose bands lie in 6, 14 and 28 neighbouring lanes only (bands
  shared out over 8, 4 and 2 lanes), nine entries each, one of them on the edge; and a last tile of 75 objects (one
  object in lane 37, none beyond). The first partner of the patch is the first entry of its window and of lane 1's band
  (a band that starts at entry 0 of its chunk: the downward walk steps from it onto the sentinels in front of the chunk),
  and the three partners of a tile's last lane are the last entries of the tile's window (a band that ends at the chunk's
  last entry, where the downward walk begins).
* patches 1-3, the CLUMPS: 319, 511 and 700 streamed objects within half an arcminute, around a hundred lane objects: a
  window of one entry less than each stage holds, and windows longer than both stages (they go through the stage in
  pieces). Lanes whose bands have ended walk the sentinel while the longest band of the wave goes on.
* a twin of every eighth lane object with the SAME sort key (self counts on the diagonal jobs: half bands with tied keys).

Every case runs both inclusions' kernels it names against the brute-force oracle: integer counts bit for bit, weighted sums
to 1e-10 relative, as tests/test_gpu_kernel_parity.py. `evaluated_pairs` and `exact_reevaluations` must equal what the
kernels gave before the loop was rewritten (tests/golden/band_walk_trips.npz, recorded by
tools/make_golden_band_walk_trips.py): the same evaluations are settled by the exact predicate, no more and no fewer.
"""
from __future__ import annotations

import functools

import numpy as np
import pytest

import test_gpu_count_variants as table
from conftest import ARCMIN, load_golden
from oracle import oracle

pytestmark = pytest.mark.gpu
RTOL_W = 1e-10

B, P = table.B, table.P          # three redshift bins, four patches
BIN_SCALE = (1.0, 0.85, 0.7)     # per-bin threshold rows ("/bins")
GRIDS = {                        # edges in arcmin; the largest separation is 1' in every grid
    "e2": np.array([0.2, 1.0]),
    "e3": np.array([0.2, 0.5, 1.0]),
    "e4": np.array([0.2, 0.4, 0.7, 1.0]),
}
R_MAX = 1.0 * ARCMIN
PAIR_GAP = 0.3 * ARCMIN          # between the two objects of a lane
LANE_GAP = 4.5 * ARCMIN          # between lanes: more than two windows plus every margin
Y0 = 0.501                       # the line's coordinate across the strips (strip grid 2e-3: the middle of a cell)
DELTAS = (0.0, 1e-16, -1e-16, 4e-16, -4e-16, 1e-12, -1e-12, 1e-9, -1e-9)


def angles(grid: str) -> np.ndarray:
    name, _, per_bin = grid.partition("/")
    row = GRIDS[name] * ARCMIN
    return np.stack([row * (BIN_SCALE[k] if per_bin else 1.0) for k in range(B)])


def thresholds(grid: str) -> np.ndarray:
    return np.stack([oracle.thresholds_for(a) for a in angles(grid)])


def _unit(u, v):
    """Unit vectors with sort-axis coordinate z = u and y = v (the footprint lies around x = 0.865, y = 0.5)."""
    u, v = np.asarray(u, dtype=np.float64), np.asarray(v, dtype=np.float64)
    return np.column_stack([np.sqrt(1.0 - u * u - v * v), v, u])


def _sky(xyz):
    ra, dec = oracle.from_3d(xyz[:, 0], xyz[:, 1], xyz[:, 2])
    return ra, dec


def _around(a, radius, phi, delta=0.0):
    """The unit vector at angle `radius` (1 + delta) from the unit vector a, in the direction phi from the one in which the
    sort key z grows fastest (phi = pi: the partner with the lowest key at that distance)."""
    north = np.array([0.0, 0.0, 1.0]) - a[2] * a
    north /= np.linalg.norm(north)
    east = np.cross(north, a)
    r = radius * (1.0 + delta)
    return a * np.cos(r) + (np.cos(phi) * north + np.sin(phi) * east) * np.sin(r)


@functools.lru_cache(maxsize=1)
def _scene():
    rng = np.random.default_rng(20261021)
    lane_u, lane_v, lane_p = [], [], []      # lane side (c1), as (z, y)
    part_xyz, part_p = [], []                # streamed side (c2)

    def partner(a, radius, phi, delta, patch=0):
        part_xyz.append(_around(a, radius, phi, delta))
        part_p.append(patch)

    # ---- patch 0: the line. Lane j = objects 2 j and 2 j + 1 of the run, tiles of 128 objects.
    n_lanes = 5 * 64 + 38
    u = -0.24
    for j in range(n_lanes):
        tile, lane = divmod(j, 64)
        n_obj = 1 if j == n_lanes - 1 else 2  # the last tile: 75 objects
        us = [u, u + PAIR_GAP][:n_obj]
        for q in us:
            lane_u.append(q)
            lane_v.append(Y0)
            lane_p.append(0)
        a0, a1 = _unit(us[0], Y0)[0], _unit(us[-1], Y0)[0]
        scale = BIN_SCALE[(2 * j) % B] if j % 2 else 1.0  # every other lane on the edge of its own bin's row
        edge = R_MAX * scale
        d = DELTAS[j % len(DELTAS)]
        if tile in (2, 3, 4):  # bands in a few neighbouring lanes only: shared out over 8, 4, 2 lanes
            first, count = {2: (0, 6), 3: (10, 14), 4: (3, 28)}[tile]
            if first <= lane < first + count:
                partner(a0, edge, np.pi, d)  # the undecided evaluation inside a shared band
                for _ in range(8):
                    partner(a0, rng.uniform(0.05, 0.95) * R_MAX, rng.uniform(0.0, 2.0 * np.pi), 0.0)
        else:
            kind = j % 4  # bands of 0, 1, 2, 3 entries
            if kind == 1:
                partner(a0, edge, np.pi, d)                       # first entry of the band, first trip
            elif kind == 2 and n_obj == 2:
                mid = (a0 + a1) / np.linalg.norm(a0 + a1)           # on the bisector: both objects in the same trip
                half = 0.5 * np.arccos(np.clip(a0 @ a1, -1.0, 1.0))
                partner(mid, np.arccos(np.cos(edge) / np.cos(half)), 0.5 * np.pi, d)
                inner = GRIDS[("e2", "e3", "e4")[j % 3]][j % 2 if j % 3 else 0] * ARCMIN
                partner(a1, inner if j % 8 >= 4 else edge, 0.0, d)  # last entry of the band, last trip (or an inner edge)
            elif kind == 3:
                partner(a0, edge, np.pi, d)
                partner(a0, edge, np.pi - 0.05, -d)                 # two entries next to each other: consecutive trips
                partner(a0, edge, np.pi + 0.06, d)
        u += LANE_GAP * (1.0 + 0.1 * rng.random())
    assert u < 0.26
    # ---- patches 1-3: the clumps
    for patch, n_stream in ((1, 319), (2, 511), (3, 700)):
        uc = 0.28 + 0.02 * patch
        n_lane = 100
        lu = uc + rng.uniform(-0.25, 0.25, n_lane) * ARCMIN
        lv = Y0 + rng.uniform(-0.25, 0.25, n_lane) * ARCMIN
        lane_u += list(lu); lane_v += list(lv); lane_p += [patch] * n_lane
        n_edge = 24
        part_xyz += list(_unit(uc + rng.uniform(-0.25, 0.25, n_stream - n_edge) * ARCMIN, Y0 + rng.uniform(-0.25, 0.25, n_stream - n_edge) * ARCMIN))
        part_p += [patch] * (n_stream - n_edge)
        for i in range(n_edge):  # on the 0.2' edge (the clump is narrower than the outer one) of a lane object
            partner(_unit(lu[i], lv[i])[0], 0.2 * ARCMIN, rng.uniform(0.0, 2.0 * np.pi), DELTAS[i % len(DELTAS)], patch)
    lane_u, lane_v, lane_p = np.array(lane_u), np.array(lane_v), np.array(lane_p)
    part_xyz, part_p = np.array(part_xyz), np.array(part_p)
    # twins with the same sort key (z) a little across the strip: tied keys in the self counts
    twin = np.arange(0, len(lane_u), 8)
    lane_u = np.concatenate([lane_u, lane_u[twin]])
    lane_v = np.concatenate([lane_v, lane_v[twin] + 0.5 * ARCMIN])
    lane_p = np.concatenate([lane_p, lane_p[twin]])

    zedges = np.linspace(0.1, 0.9, B + 1)
    n1, n2 = len(lane_u), len(part_p)
    k1 = np.arange(n1) % B                                  # objects 2 j, 2 j + 1 of lane j: bins (2 j) % B, (2 j + 1) % B
    z1 = 0.5 * (zedges[k1] + zedges[k1 + 1])
    z2 = 0.5 * (zedges[np.arange(n2) % B] + zedges[np.arange(n2) % B + 1])
    w1, w2 = 10.0 ** rng.uniform(-2.0, 2.0, n1), 10.0 ** rng.uniform(-2.0, 2.0, n2)
    ra1, dec1 = _sky(_unit(lane_u, lane_v))
    ra2, dec2 = _sky(part_xyz)
    return {
        "c1": oracle.sort_catalog(ra1, dec1, z1, w1, lane_p, P, zedges, "right"),
        "c2b": oracle.sort_catalog(ra2, dec2, z2, w2, part_p, P, zedges, "right"),
        "c2u": oracle.sort_catalog(ra2, dec2, None, w2, part_p, P, None, "right"),
    }


JOBS = table.JOBS
PAIRS = table.PAIRS  # "cross": c1 x c2u, "binned": c1 x c2b, "self": c1 x c1


def _cases():
    """(id, pair, grid, options, (unweighted, weighted) variant). tile_r and band_cap as tests/test_gpu_count_variants.py
    sets them; triple_runs = 2 merges the three strip runs into one window (k_count_band32_one), 0 keeps three windows."""
    out = []

    def add(one, r, cap, ne, pair, per_bin=False, **extra):
        fam = "k_count_band32_one" if one else "k_count_band32"
        merged = pair == "cross"
        uni = not (merged and per_bin)
        grid = f"e{ne}" + ("/bins" if per_bin else "")
        opts = {"kernel": "band", "band_fp32": 1, "triple_runs": 2 if one else 0, "tile_r": r, **extra}
        if r == 2:
            opts["band_cap"] = cap
        tag = ",".join(f"{k}={v}" for k, v in extra.items())
        out.append((f"{fam}-R{r}-CAP{cap}-E{ne}-{pair}-{grid}" + (f"-{tag}" if tag else ""), pair, grid, opts,
                    table._pair_reach(fam, r, cap, ne, merged, uni)))

    for one in (True, False):          # both inclusions, both stages, the plain one-annulus count (the headline's variants)
        for cap in (512, 320):
            add(one, 2, cap, 2, "cross")
    add(True, 2, 512, 2, "cross", flush_stages_log2=0)  # a flush of the lane counters after every stage
    add(True, 2, 512, 3, "cross")      # three and four edges
    add(False, 2, 512, 4, "cross")
    add(True, 2, 320, 2, "cross", per_bin=True)   # a threshold row per lane object
    add(False, 2, 512, 2, "cross", per_bin=True)
    add(True, 2, 512, 2, "binned")     # per-bin items
    add(True, 1, 320, 2, "cross")      # one object per lane: two entries per trip
    add(True, 1, 320, 2, "self")       # half bands on the diagonal jobs, tied keys
    add(False, 1, 320, 2, "binned")
    add(True, 4, 512, 2, "cross")      # four objects per lane
    return out


CASES = _cases()


@pytest.fixture(scope="module")
def cats():
    return _scene()


@pytest.fixture(scope="module")
def device(cats):
    d = table._Device(0, cats)
    yield d
    d.close()


@pytest.fixture(scope="module")
def expected(cats):
    memo = {}

    def get(pair, grid):
        if (pair, grid) not in memo:
            a, b = PAIRS[pair]
            memo[(pair, grid)] = oracle.count_jobs(cats[a], cats[b], JOBS, thresholds(grid))
        return memo[(pair, grid)]

    return get


def run_case(d, case):
    """(counts, sums, stats) of a case on the device, the options restored afterwards."""
    from yet_another_wizz_amd import _lib

    _, pair, grid, options, _ = case
    a, b = PAIRS[pair]
    try:
        table._apply(d.ctx, {"seg_strips_min_run": 1, **options})
        return _lib.count_pairs(d.ctx, d.dev[a], d.dev[b], JOBS, thresholds(grid), want_counts=True, want_sums=True)
    finally:
        table._restore(d.ctx)


def test_the_scene_is_what_the_cases_need(cats):
    c1, c2 = cats["c1"], cats["c2u"]
    n1 = np.array([c1["off"][(p + 1) * B] - c1["off"][p * B] for p in range(P)])
    n2 = np.diff(c2["off"])
    assert n1[0] > 5 * 128 and list(n2[1:]) == [319, 511, 700]  # CAP - 1 entries for both stages, and longer than both
    assert len(c1["x"]) < 2000 and len(c2["x"]) < 3000


@pytest.mark.parametrize("case", CASES, ids=[c[0] for c in CASES])
def test_walk_against_oracle_and_recorded_work(device, expected, case):
    cid, pair, grid, _, reach = case
    counts, sums, st = run_case(device, case)
    assert st.variants == set(reach), (cid, st.variants)
    exp_c, exp_s = expected(pair, grid)
    assert exp_c.sum() > 1000, cid
    assert np.array_equal(counts, exp_c), cid
    np.testing.assert_allclose(sums, exp_s, rtol=RTOL_W, atol=0, err_msg=cid)
    assert st.exact_reevaluations > 0, cid
    recorded = load_golden("band_walk_trips.npz")
    ids = [str(s) for s in recorded["case"]]
    assert cid in ids, f"{cid}: not in tests/golden/band_walk_trips.npz (tools/make_golden_band_walk_trips.py)"
    i = ids.index(cid)
    print(cid, "evaluated_pairs", st.evaluated_pairs, "exact_reevaluations", st.exact_reevaluations)
    assert st.evaluated_pairs == int(recorded["evaluated_pairs"][i]), cid
    assert st.exact_reevaluations == int(recorded["exact_reevaluations"][i]), cid
