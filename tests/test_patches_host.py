"""The numpy route of patches.py (the oracle of the device route, tests/test_gpu_kmeans.py) against its own arithmetic
restated with Python integers: the pick rule of the seeding, the integer sums of one Lloyd round, the blocked passes, the
inertia, the stop rule, the errors and the edge shapes -- then ``patch_method`` of the Catalog constructors. No GPU: the
device route is switched off."""
import bisect
import itertools

import numpy as np
import pytest

import yet_another_wizz_amd as yaw
from yet_another_wizz_amd import catalog, patches
from yet_another_wizz_amd.catalog import radec_to_xyz


@pytest.fixture(autouse=True)
def numpy_route(monkeypatch):
    monkeypatch.setattr(patches, "DEVICE_KMEANS_MIN", 1 << 62)


def sky(n, seed, cap=False):
    """(ra, dec) in radian: uniform on the sphere, or on a cap of 10 degrees."""
    rng = np.random.default_rng(seed)
    ra = rng.uniform(0.0, 2.0 * np.pi, n)
    dec = np.arcsin(rng.uniform(np.cos(np.deg2rad(10.0)) if cap else -1.0, 1.0, n))
    return ra, dec


def d2(px, py, pz, c):
    return ((px - c[0]) ** 2 + (py - c[1]) ** 2) + (pz - c[2]) ** 2


@pytest.mark.parametrize("seed", [1, 12345, 987654321])
def test_pick_rule_in_python_integers(seed):
    n, k = 1000, 9
    ra, dec = sky(n, 7)
    x, y, z = radec_to_xyz(ra, dec)
    _, info = patches.create_patch_centers(ra, dec, k, degrees=False, seed=seed, max_iterations=0, return_info=True)
    rng = np.random.default_rng(seed)
    chosen = [int(rng.integers(n))]
    m = None
    while len(chosen) < k:
        c = (x[chosen[-1]], y[chosen[-1]], z[chosen[-1]])
        d = d2(x, y, z, c)
        m = d if m is None else np.minimum(m, d)
        q = [int(np.floor(v * 2.0 ** 29)) for v in m]
        prefix = list(itertools.accumulate(q))  # Python integers
        r = int(rng.integers(prefix[-1]))
        chosen.append(bisect.bisect_right(prefix, r))  # the smallest index whose inclusive prefix exceeds r
        assert q[chosen[-1]] > 0
    assert info["seeds"].tolist() == chosen and len(set(chosen)) == k
    assert info["iterations"] == 0 and info["inertia"] == [] and not info["converged"]


@pytest.mark.parametrize("weighted", [False, True])
def test_one_round_in_python_integers(weighted):
    n, k = 2000, 11
    rng = np.random.default_rng(3)
    ra, dec = sky(n, 11)
    x, y, z = radec_to_xyz(ra, dec)
    w = None
    if weighted:
        w = np.ldexp(rng.uniform(0.5, 1.0, n), rng.integers(-20, 21, n))
        w[::17] = 0.0
        w[5] = -w[5]
    centres = np.column_stack([x[:k], y[:k], z[:k]])
    sums, counts, inertia, ids = patches.numpy_round(x, y, z, centres, w)
    scale = None
    if weighted:
        _, e = np.frexp(np.abs(w).max())
        scale = float(2.0 ** (30 - int(e)))
        assert scale == patches.weight_scale(w)
    exp_s, exp_n, exp_j = [[0, 0, 0] for _ in range(k)], [0] * k, 0
    for i in range(n):
        d = [float(d2(x[i], y[i], z[i], centres[c])) for c in range(k)]
        best = d.index(min(d))  # first minimum
        assert ids[i] == best
        exp_n[best] += 1
        exp_j += int(np.floor(d[best] * 2.0 ** 29))
        for axis, col in enumerate((x, y, z)):
            a = np.rint(col[i] * 2.0 ** 30) if w is None else np.rint((w[i] * col[i]) * scale)
            assert abs(a) <= 2 ** 30
            exp_s[best][axis] += int(a)
    assert sums.dtype == np.int64 and counts.dtype == np.int64
    assert sums.tolist() == exp_s and counts.tolist() == exp_n and inertia == exp_j


def test_blocked_passes_and_repeat_runs_agree(monkeypatch):
    n, k = 600, 5
    ra, dec = sky(n, 21, cap=True)
    w = np.random.default_rng(5).uniform(0.1, 3.0, n)
    base, base_info = patches.create_patch_centers(ra, dec, k, weights=w, degrees=False, return_info=True)
    again = patches.create_patch_centers(ra, dec, k, weights=w, degrees=False)
    assert np.array_equal(base.data, again.data)
    for block in (1, 7, n):
        monkeypatch.setattr(patches, "HOST_BLOCK", block)
        got, info = patches.create_patch_centers(ra, dec, k, weights=w, degrees=False, return_info=True)
        assert np.array_equal(got.data, base.data), block
        assert info["inertia"] == base_info["inertia"] and info["seeds"].tolist() == base_info["seeds"].tolist()
        assert np.array_equal(info["sums"], base_info["sums"]) and np.array_equal(info["counts"], base_info["counts"])


def test_inertia_never_grows_beyond_the_quantisation():
    """Unweighted: J_{t+1} <= J_t + 4 n. The floor contributes less than n; a centre displaced by the 2^-30 quantisation of
    the sums changes each d 2^29 by less than 3."""
    n, k = 5000, 12
    ra, dec = sky(n, 31, cap=True)
    _, info = patches.create_patch_centers(ra, dec, k, degrees=False, return_info=True)
    j = info["inertia"]
    assert info["iterations"] == len(j) >= 3 and info["route"] == "numpy"
    for a, b in zip(j[:-1], j[1:]):
        assert b <= a + 4 * n
    assert j[-1] < j[0]
    assert int(info["counts"].sum()) == n


def test_converged_run_repeats_its_sums():
    n, k = 3000, 6
    ra, dec = sky(n, 41)
    centers, info = patches.create_patch_centers(ra, dec, k, degrees=False, return_info=True)
    assert info["converged"] and info["iterations"] < 100
    x, y, z = radec_to_xyz(ra, dec)
    # the centres the run ended on, before their trip through (ra, dec): one more round from the last sums
    seeds = info["seeds"]
    c = np.column_stack([x[seeds], y[seeds], z[seeds]])
    for _ in range(info["iterations"] - 1):
        s, cnt, _, _ = patches.numpy_round(x, y, z, c)
        c = patches.update_centres(s, cnt, c)
    assert np.array_equal(yaw.AngularCoordinates.from_3d(c).data, centers.data)
    s, cnt, _, _ = patches.numpy_round(x, y, z, c)
    assert np.array_equal(s, info["sums"]) and np.array_equal(cnt, info["counts"])
    c2 = patches.update_centres(s, cnt, c)
    s2, cnt2, _, _ = patches.numpy_round(x, y, z, c2)  # one more round
    assert np.array_equal(c2, c) and np.array_equal(s2, s) and np.array_equal(cnt2, cnt)
    stopped, early = patches.create_patch_centers(ra, dec, k, degrees=False, max_iterations=2, return_info=True)
    assert early["iterations"] == 2 and not early["converged"] and early["inertia"] == info["inertia"][:2]


def test_errors():
    ra, dec = sky(50, 51)
    few = np.concatenate([np.full(30, 1.0), np.full(20, 2.0)]), np.concatenate([np.full(30, 0.5), np.full(20, -0.25)])
    with pytest.raises(ValueError, match="distinct"):
        patches.create_patch_centers(*few, 3, degrees=False)
    assert len(patches.create_patch_centers(*few, 2, degrees=False)) == 2
    with pytest.raises(ValueError, match="all zero"):
        patches.create_patch_centers(ra, dec, 4, weights=np.zeros(50), degrees=False)
    w = np.ones(50)
    w[3] = 1e300
    with pytest.raises(ValueError, match="range"):
        patches.create_patch_centers(ra, dec, 4, weights=w, degrees=False)
    w[3] = np.inf
    with pytest.raises(ValueError):
        patches.create_patch_centers(ra, dec, 4, weights=w, degrees=False)
    for bad in (0, -2):
        with pytest.raises(ValueError, match="patch_num"):
            patches.create_patch_centers(ra, dec, bad, degrees=False)
    with pytest.raises(ValueError, match="51 patches from 50"):
        patches.create_patch_centers(ra, dec, 51, degrees=False)
    with pytest.raises(ValueError, match="patch_method"):
        yaw.Catalog.from_arrays(ra, dec, patch_num=4, degrees=False, patch_method="treecorr")
    with pytest.raises(ValueError, match="patch_method"):  # also where centres take precedence
        yaw.Catalog.from_arrays(ra, dec, patch_centers=yaw.AngularCoordinates([[1.0, 0.0]]), degrees=False, patch_method="all")


def test_edge_shapes():
    n = 40
    ra, dec = sky(n, 61)
    x, y, z = radec_to_xyz(ra, dec)
    one, info = patches.create_patch_centers(ra, dec, 1, degrees=False, return_info=True)
    a = np.rint(np.column_stack([x, y, z]) * 2.0 ** 30).astype(np.int64).sum(axis=0)
    assert info["converged"] and info["iterations"] == 2 and info["counts"].tolist() == [n]
    assert info["sums"].tolist() == [a.tolist()]
    af = a.astype(np.float64)
    mean = af / np.sqrt((af[0] ** 2 + af[1] ** 2) + af[2] ** 2)
    assert np.array_equal(one.data, yaw.AngularCoordinates.from_3d(mean).data)
    # k = n: every point is drawn once and is its own centre
    every, info = patches.create_patch_centers(ra, dec, n, degrees=False, return_info=True)
    assert sorted(info["seeds"].tolist()) == list(range(n))
    assert info["counts"].tolist() == [1] * n and info["inertia"][-1] == 0 and info["converged"]
    # an antipodal pair: d = 4 exactly, q = 2^31
    pair_x, pair_y, pair_z = np.array([1.0, -1.0]), np.zeros(2), np.zeros(2)
    route = patches._HostRoute(pair_x, pair_y, pair_z, None, None)
    assert route.seed((1.0, 0.0, 0.0), True) == 2 ** 31 and route.q.tolist() == [0, 2 ** 31]
    assert route.pick(0) == 1 and route.pick(2 ** 31 - 1) == 1
    sums, counts, inertia, ids = patches.numpy_round(pair_x, pair_y, pair_z, np.array([[1.0, 0.0, 0.0]]))
    assert inertia == 2 ** 31 and sums.tolist() == [[0, 0, 0]] and counts.tolist() == [2]
    kept = patches.update_centres(sums, counts, np.array([[1.0, 0.0, 0.0]]))  # zero norm: the centre stays
    assert kept.tolist() == [[1.0, 0.0, 0.0]]
    both, info = patches.centers_from_xyz((pair_x, pair_y, pair_z), None, 2, return_info=True)
    assert sorted(info["seeds"].tolist()) == [0, 1] and info["counts"].tolist() == [1, 1]


def test_default_patch_method_is_the_probe_path():
    n = 4000
    ra, dec = sky(n, 71, cap=True)
    w = np.random.default_rng(8).uniform(0.5, 1.5, n)
    cat = yaw.Catalog.from_arrays(ra, dec, weights=w, patch_num=8, degrees=False)
    probe_size = int(100_000 * np.sqrt(8))
    step = max(1, n // probe_size)
    x, y, z = radec_to_xyz(ra[::step], dec[::step])
    expect = catalog.kmeans_centers(np.column_stack([x, y, z]), w[::step], 8)
    assigned = catalog.nearest_center(radec_to_xyz(ra, dec), expect.to_3d())
    assert np.array_equal(np.array(cat.get_num_records()), np.bincount(assigned, minlength=8))
    explicit = yaw.Catalog.from_arrays(ra, dec, weights=w, patch_num=8, degrees=False, patch_method="probe")
    assert np.array_equal(explicit.get_centers().data, cat.get_centers().data)
    given = yaw.Catalog.from_arrays(ra, dec, weights=w, patch_centers=expect, degrees=False)
    assert np.array_equal(given.get_centers().data, cat.get_centers().data) and np.array_equal(given.get_centers().data, expect.data)


def test_full_patch_method_is_create_patch_centers():
    n = 4000
    ra, dec = sky(n, 81, cap=True)
    w = np.random.default_rng(9).uniform(0.5, 1.5, n)
    centres = patches.create_patch_centers(np.rad2deg(ra), np.rad2deg(dec), 8, weights=w)
    assert np.array_equal(centres.data, patches.create_patch_centers(ra, dec, 8, weights=w, degrees=False).data)
    full = yaw.Catalog.from_arrays(ra, dec, weights=w, patch_num=8, degrees=False, patch_method="full")
    given = yaw.Catalog.from_arrays(ra, dec, weights=w, patch_centers=centres, degrees=False)
    assert full.num_patches == 8 and full.get_num_records() == given.get_num_records()
    assert np.array_equal(full.get_centers().data, given.get_centers().data) and np.array_equal(full.get_centers().data, centres.data)
    assert np.array_equal(full._ra, given._ra) and np.array_equal(full._w, given._w)
    frame = dict(ra=np.rad2deg(ra), dec=np.rad2deg(dec), w=w)
    framed = yaw.Catalog.from_dataframe(None, frame, ra_name="ra", dec_name="dec", weight_name="w", patch_num=8, patch_method="full")
    assert framed.get_num_records() == full.get_num_records()
    # ids take precedence: the method is ignored
    ids = np.arange(n) % 3
    by_ids = yaw.Catalog.from_arrays(ra, dec, patch_ids=ids, patch_num=8, degrees=False, patch_method="full")
    assert by_ids.num_patches == 3


def test_healpix_map_footprint_in_six_patches():
    from yet_another_wizz_amd.randoms import pix2loc_nest

    nside = 16
    npix = 12 * nside * nside
    _, zc = pix2loc_nest(4, np.arange(npix))
    values = np.where(zc > 0.0, 1.0 + 0.001 * np.arange(npix), -1.6375e30)  # the northern half, the rest UNSEEN
    cat = yaw.Catalog.from_healpix_map(None, values, nested=True, patch_num=6, patch_method="full")
    sizes = np.array(cat.get_num_records())
    assert cat.num_patches == 6 and sizes.min() > 0 and sizes.sum() == np.count_nonzero(zc > 0.0)
