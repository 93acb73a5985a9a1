"""GPU: the device route of the full-catalogue k-means (yawhip_kmeans_*, csrc/yawhip_kmeans.hip) against the numpy route of
patches.py, bit for bit: seed totals and picks at segment boundaries and across a segment whose q are all zero, the integer
sums, counts, inertia and ids of one Lloyd round on both accumulation paths (LDS partials, global atomics) with and without
weights, exact ties, whole runs, the error paths, and ``Catalog.from_arrays(patch_method="full")``."""
import functools

import numpy as np
import pytest

import yet_another_wizz_amd as yaw
from yet_another_wizz_amd import _lib, engine, patches
from yet_another_wizz_amd.catalog import radec_to_xyz

pytestmark = pytest.mark.gpu
SHIPPED_MIN = patches.DEVICE_KMEANS_MIN


@pytest.fixture(autouse=True)
def device_route(monkeypatch):
    monkeypatch.setattr(patches, "DEVICE_KMEANS_MIN", 0)


def on_host(fn, *args, **kwargs):
    """``fn`` on the numpy route."""
    saved, patches.DEVICE_KMEANS_MIN = patches.DEVICE_KMEANS_MIN, 1 << 62
    try:
        return fn(*args, **kwargs)
    finally:
        patches.DEVICE_KMEANS_MIN = saved


@functools.lru_cache(maxsize=None)
def points(n):
    """n unit vectors, uniform on the sphere, and weights spanning 2^-20 .. 2^20 with zeros and one negative. Read-only."""
    rng = np.random.default_rng(n)
    ra = rng.uniform(0.0, 2.0 * np.pi, n)
    dec = np.arcsin(rng.uniform(-1.0, 1.0, n))
    x, y, z = radec_to_xyz(ra, dec)
    w = np.ldexp(rng.uniform(0.5, 1.0, n), rng.integers(-19, 21, n))
    w[::13] = 0.0
    w[7] = -w[7]
    w[1], w[2] = 2.0 ** -20, 2.0 ** 20 * (1.0 - 2.0 ** -53)
    for a in (ra, dec, x, y, z, w):
        a.setflags(write=False)
    return ra, dec, x, y, z, w


@functools.lru_cache(maxsize=None)
def host_round(n, k, weighted):
    _, _, x, y, z, w = points(n)
    centres = np.column_stack([x[:k], y[:k], z[:k]]) * 0.999  # (off the points: no zero distances)
    return centres, patches.numpy_round(x, y, z, centres, w if weighted else None)


def test_seed_totals_and_picks_at_segment_boundaries():
    n = 70_001
    _, _, x, y, z, _ = points(n)
    x, y, z = x.copy(), y.copy(), z.copy()
    with engine.kmeans_open(x[:1], y[:1], z[:1]) as probe:
        seg = probe.segment
    n_seg = -(-n // seg)
    assert n % seg != 0 and n_seg >= 6  # a ragged last segment
    first = 2 * seg + 5
    for c in (x, y, z):  # segment 2 is a slab of duplicates of the first centre: all of its q are zero
        c[2 * seg : 3 * seg] = c[first]
    host = patches._HostRoute(x, y, z, None, None)
    with engine.kmeans_open(x, y, z) as km:
        for i, is_first in ((first, True), (11, False)):
            centre = (x[i], y[i], z[i])
            total = host.seed(centre, is_first)
            assert km.seed(centre, is_first) == total > 0
        q = host.q.astype(np.uint64)
        assert not q[2 * seg : 3 * seg].any() and q[first] == 0 and q[11] == 0
        prefix = np.cumsum(q, dtype=np.uint64)
        assert int(prefix[-1]) == total
        ends = [int(prefix[s * seg - 1]) for s in (1, 2, 3, n_seg // 2, n_seg - 1)]  # (2, 3: before and after the zero slab)
        assert ends[1] == ends[2]
        for r in [0, total - 1] + ends + [e - 1 for e in ends]:
            expect = int(np.searchsorted(prefix, np.uint64(r), side="right"))
            assert km.pick(r) == expect == host.pick(r), r
        assert km.pick(ends[1]) == 3 * seg  # the zero segment is skipped
        with pytest.raises(_lib.YawhipError, match="not below the total"):
            km.pick(total)


@pytest.mark.parametrize("weighted", [False, True])
@pytest.mark.parametrize("n, k, path", [(70_001, 7, "lds"), (200_003, 64, "lds"), (50_000, 4096, "global")])
def test_one_step_matches_numpy(n, k, path, weighted):
    _, _, x, y, z, w = points(n)
    centres, (sums, counts, inertia, ids) = host_round(n, k, weighted)
    wts = w if weighted else None
    with engine.kmeans_open(x, y, z, wts, patches.weight_scale(w) if weighted else 0.0) as km:
        assert km.max_centres_lds < 4096 <= km.max_centres
        got = km.step(centres, want_ids=True)
        assert km.last_path == path  # 7 and 64 keep their partials in LDS, 4096 adds to global memory
        again = km.step(centres)
    assert got[0].dtype == np.int64 and got[3].dtype == np.int32
    assert np.array_equal(got[3], ids)
    assert np.array_equal(got[1], counts) and int(counts.sum()) == n
    assert np.array_equal(got[0], sums)
    assert got[2] == inertia
    assert again[3] is None and np.array_equal(again[0], sums) and np.array_equal(again[1], counts) and again[2] == inertia


def test_exact_ties_go_to_the_lower_index():
    rng = np.random.default_rng(5)
    n = 3000
    angle = rng.uniform(0.0, 2.0 * np.pi, n)
    x, y, z = np.zeros(n), np.cos(angle), np.sin(angle)  # on the plane x = 0
    x[2000:] = rng.choice([-0.25, 0.25], 1000)           # and off it
    centres = np.array([[0.5, 0.25, 0.0], [-0.5, 0.25, 0.0], [0.5, 0.25, 0.0]])  # 0 and 1 mirror images, 2 a copy of 0
    with engine.kmeans_open(x, y, z) as km:
        sums, counts, inertia, ids = km.step(centres, want_ids=True)
        assert np.all(ids[:2000] == 0) and np.array_equal(ids[2000:], np.where(x[2000:] > 0, 0, 1)) and counts[2] == 0
        swapped = km.step(centres[[1, 0, 2]], want_ids=True)[3]
        assert np.all(swapped[:2000] == 0) and np.array_equal(swapped[2000:], np.where(x[2000:] > 0, 1, 0))
    expect = patches.numpy_round(x, y, z, centres)
    assert np.array_equal(ids, expect[3]) and np.array_equal(sums, expect[0]) and np.array_equal(counts, expect[1])
    assert inertia == expect[2]


@pytest.mark.parametrize("weighted", [False, True])
def test_whole_run_equals_the_numpy_route(weighted):
    n, k = 200_003, 16
    ra, dec, _, _, _, w = points(n)
    kwargs = dict(weights=w if weighted else None, degrees=False, max_iterations=10, return_info=True)
    host, host_info = on_host(patches.create_patch_centers, ra, dec, k, **kwargs)
    dev, dev_info = patches.create_patch_centers(ra, dec, k, **kwargs)
    dev2, dev2_info = patches.create_patch_centers(ra, dec, k, **kwargs)
    assert host_info["route"] == "numpy" and dev_info["route"] == "device" and dev_info["step_path"] == "lds"
    assert np.array_equal(dev.data, host.data) and np.array_equal(dev2.data, dev.data)
    for info in (dev_info, dev2_info):
        assert info["inertia"] == host_info["inertia"] and info["iterations"] == host_info["iterations"] == 10
        assert info["seeds"].tolist() == host_info["seeds"].tolist() and info["converged"] == host_info["converged"]
        assert np.array_equal(info["sums"], host_info["sums"]) and np.array_equal(info["counts"], host_info["counts"])


def test_too_many_centres_and_double_close():
    n = 7000
    ra, dec, x, y, z, _ = points(n)
    km = engine.kmeans_open(x, y, z)
    k = km.max_centres + 1
    assert k <= n
    with pytest.raises(_lib.YawhipError, match="too many centres"):
        km.step(np.column_stack([x[:k], y[:k], z[:k]]))
    sums, counts, _, _ = km.step(np.column_stack([x[: k - 1], y[: k - 1], z[: k - 1]]))  # the largest table that fits
    assert int(counts.sum()) == n and km.last_path == "global"
    km.close()
    km.close()  # harmless
    with pytest.raises(_lib.YawhipError):
        km.step(np.zeros((1, 3)))
    assert engine.kmeans_open(x, y, z).close() is None
    # the Python layer takes the numpy route for such a k: the same centres
    kwargs = dict(degrees=False, max_iterations=1, return_info=True)
    got, info = patches.create_patch_centers(ra, dec, k, **kwargs)
    expect, expect_info = on_host(patches.create_patch_centers, ra, dec, k, **kwargs)
    assert info["route"] == "numpy" and np.array_equal(got.data, expect.data) and info["inertia"] == expect_info["inertia"]


def test_catalog_with_full_patch_method(monkeypatch):
    """300 000 points in sixteen separated groups (the run converges in a few rounds): sixteen non-empty patches around the
    numpy route's centres."""
    monkeypatch.setattr(patches, "DEVICE_KMEANS_MIN", SHIPPED_MIN)  # as shipped: this size takes the device route
    assert SHIPPED_MIN <= 300_000
    n = 300_000
    rng = np.random.default_rng(16)
    group = rng.integers(0, 16, n)
    ra = np.deg2rad(20.0 + 25.0 * (group % 8) + rng.normal(0.0, 1.0, n))
    dec = np.deg2rad(-20.0 + 40.0 * (group // 8) + rng.normal(0.0, 1.0, n))
    w = rng.uniform(0.5, 2.0, n)
    cat = yaw.Catalog.from_arrays(ra, dec, weights=w, patch_num=16, degrees=False, patch_method="full")
    dev, info = patches.create_patch_centers(ra, dec, 16, weights=w, degrees=False, return_info=True)
    host = on_host(patches.create_patch_centers, ra, dec, 16, weights=w, degrees=False)
    assert info["route"] == "device" and info["converged"]
    assert cat.num_patches == 16 and min(cat.get_num_records()) > 0 and sum(cat.get_num_records()) == n
    assert np.array_equal(cat.get_centers().data, host.data) and np.array_equal(dev.data, host.data)
