"""The strip grid in latitude (``strip_grid``) and the trimmed u-bands (``band_trim``) against the CPU oracle.

Both are culling only: a partner at the largest separation must stay inside every window and band wherever it sits. The
inputs put such partners where the trimmed bounds are tight or change form: lane objects with sort key u = z from -1 + 1e-6 to
1 - 1e-6 (the cap formula clips to -1 / +1 near the poles), objects near v = y = +/-1 (latitude strips are widest in v there),
objects a hair either side of latitude-strip boundaries, and for each of them partners at the largest separation angle of its
bin (to within 1e-16 .. 1e-9, the edge moved onto the squared chord of an engineered pair) along +/-u, +/-v and a random
tangent. The library runs with the catalogues' own sort axis (auto_orient = 0: u = z, strips along y). Cases: per-bin
threshold rows (binned x binned), cross counts (binned x unbinned), self counts (half bands), one, two and four objects per
lane, three windows per item and merged triple runs, a fine-bin grid. Counts must equal the oracle bit for bit, weighted sums
to 1e-10, and both switches on must evaluate fewer entries than both off.
"""
from __future__ import annotations

import numpy as np
import pytest

from conftest import ARCMIN
from oracle import oracle

pytestmark = pytest.mark.gpu
RTOL_W = 1e-10
B, P = 2, 2
EDGES = {"e2": np.array([2.0, 20.0]), "e3": np.array([2.0, 9.0, 20.0]),
         "fine": oracle.ang_bins_for(oracle.parse_ang_limits([2.0 * ARCMIN], [20.0 * ARCMIN]), -1.0, 16) / ARCMIN}
BIN_SCALE = (1.0, 0.8)  # bin k's angles x BIN_SCALE[k] (per-bin rows)
THETA = 20.0 * ARCMIN
MICRO = int(np.ceil(1.02e6 * THETA / 50.0) * 50.0)  # grid spacing: just above the largest separation (reach 1)
JOBS = np.array([(p, q) for p in range(P) for q in range(P)], dtype=np.int32)
PAIRS = {"cross": ("c1", "c2u"), "binned": ("c1", "c2b"), "self": ("c2b", "c2b")}


def _unit(v):
    return v / np.linalg.norm(v, axis=1, keepdims=True)


def _catalogues():
    rng = np.random.default_rng(20261016)
    # lane objects where the bounds are tight or change form
    zs = np.concatenate([np.linspace(-1 + 1e-6, 1 - 1e-6, 1500), 1 - 10.0 ** -np.arange(1, 7), -1 + 10.0 ** -np.arange(1, 7)])
    phi = rng.uniform(0, 2 * np.pi, len(zs))
    a_u = np.column_stack([np.sqrt(1 - zs ** 2) * np.cos(phi), np.sqrt(1 - zs ** 2) * np.sin(phi), zs])
    ys = np.concatenate([1 - 10.0 ** -rng.uniform(1, 7, 300), -1 + 10.0 ** -rng.uniform(1, 7, 300)])
    phi = rng.uniform(0, 2 * np.pi, len(ys))
    a_v = np.column_stack([np.sqrt(1 - ys ** 2) * np.cos(phi), ys, np.sqrt(1 - ys ** 2) * np.sin(phi)])
    dth = MICRO * 1e-6  # latitude (about y) a hair either side of strip boundaries g * dth - pi / 2
    g = rng.integers(1, int(np.pi / dth), 600)
    lat = g * dth - np.pi / 2 + rng.choice([-1e-12, -1e-9, 0.0, 1e-9, 1e-12], len(g))
    phi = rng.uniform(0, 2 * np.pi, len(g))
    a_s = np.column_stack([np.cos(lat) * np.cos(phi), np.sin(lat), np.cos(lat) * np.sin(phi)])
    a = np.concatenate([a_u, a_v, a_s])
    k_a = rng.integers(0, B, len(a))
    # partners at the largest separation of the object's bin along +/-u, +/-v and a random tangent
    dirs = []
    for axis in (2, 1):
        e = np.zeros(3)
        e[axis] = 1.0
        t = e - (a @ e)[:, None] * a
        dirs += [t, -t]
    dirs.append(rng.normal(size=a.shape))
    delta = rng.choice([0.0, 1e-16, -1e-16, 2e-16, -2e-16, 1e-12, -1e-12, 1e-9, -1e-9], (len(dirs), len(a)))
    src, b = [], []
    for d, dl in zip(dirs, delta):
        d = _unit(d - (d * a).sum(1, keepdims=True) * a)
        ang = THETA * np.array(BIN_SCALE)[k_a] * (1.0 + dl)
        b.append(_unit(a * np.cos(ang)[:, None] + d * np.sin(ang)[:, None]))
        src.append(np.arange(len(a)))
    b, src = np.concatenate(b), np.concatenate(src)

    def radec(v):
        return np.arctan2(v[:, 1], v[:, 0]) % (2 * np.pi), np.arcsin(np.clip(v[:, 2], -1.0, 1.0))

    def sky(n):
        return rng.uniform(0, 2 * np.pi, n), np.arcsin(rng.uniform(-1, 1, n))

    zedges = np.array([0.1, 0.5, 0.9])
    zbin = np.array([0.3, 0.7])
    ra_a, dec_a = radec(a)
    ra_b, dec_b = radec(b)
    # the library's predicate on the coordinates the catalogues hold: squared chords of the engineered pairs, per bin
    xa, xb = np.column_stack(oracle.to_3d(ra_a[src], dec_a[src])), np.column_stack(oracle.to_3d(ra_b, dec_b))
    dd = xa - xb
    s = (dd[:, 0] * dd[:, 0] + dd[:, 1] * dd[:, 1]) + dd[:, 2] * dd[:, 2]
    ties = [np.sort(s[k_a[src] == k]) for k in range(B)]

    ra_1, dec_1 = sky(8000)
    ra1, dec1 = np.concatenate([ra_a, ra_1]), np.concatenate([dec_a, dec_1])
    z1 = np.concatenate([zbin[k_a], rng.uniform(0.11, 0.89, len(ra_1))])
    ra_2, dec_2 = sky(8000)
    ra2, dec2 = np.concatenate([ra_b, ra_2, ra_a]), np.concatenate([dec_b, dec_2, dec_a])
    z2 = np.concatenate([zbin[k_a[src]], rng.uniform(0.11, 0.89, len(ra_2)), zbin[k_a]])
    w1 = 10.0 ** rng.uniform(-3, 3, len(ra1))
    w2 = 10.0 ** rng.uniform(-3, 3, len(ra2))

    def patch_of(ra, dec):
        return (np.cos(ra) * np.cos(dec) > 0.0).astype(np.int64)

    cats = {
        "c1": oracle.sort_catalog(ra1, dec1, z1, w1, patch_of(ra1, dec1), P, zedges, "right"),
        "c2b": oracle.sort_catalog(ra2, dec2, z2, w2, patch_of(ra2, dec2), P, zedges, "right"),
        "c2u": oracle.sort_catalog(ra2, dec2, None, w2, patch_of(ra2, dec2), P, None, "right"),
    }
    return cats, ties


def _thresholds(grid, ties):
    """[B, E] thresholds; every edge moved onto the nearest squared chord of an engineered pair of its bin."""
    t = np.stack([oracle.thresholds_for(EDGES[grid] * ARCMIN * BIN_SCALE[k]) for k in range(B)])
    for k in range(B):
        j = np.clip(np.searchsorted(ties[k], t[k, -1]), 0, len(ties[k]) - 1)
        t[k, -1] = ties[k][j]
    return t


@pytest.fixture(scope="module")
def inputs():
    cats, ties = _catalogues()
    return cats, {g: _thresholds(g, ties) for g in EDGES}


@pytest.fixture(scope="module")
def expected(inputs):
    cats, ts = inputs
    return {(pair, g): oracle.count_jobs(cats[PAIRS[pair][0]], cats[PAIRS[pair][1]], JOBS, ts[g])
            for pair in PAIRS for g in EDGES}


def _count_all(device, cats, ts, expected, grid_on: bool):
    """Every case on catalogues uploaded with the strip grid and band trimming both on or both off: evaluated entries."""
    from yet_another_wizz_amd import _lib

    ctx = _lib.Context(device)
    evaluated = {}
    try:
        ctx.set_option("strip_grid", int(grid_on))
        ctx.set_option("band_trim", int(grid_on))
        ctx.set_option("auto_orient", 0)
        ctx.set_option("seg_strips_min_run", 1)
        dev = {n: _lib.DeviceCatalog(ctx, c["x"], c["y"], c["z"], c["w"], P, c["nb"], c["off"], strip_micro=MICRO)
               for n, c in cats.items()}
        for pair, (n1, n2) in PAIRS.items():
            for g in EDGES:
                exp_c, exp_s = expected[(pair, g)]
                assert exp_c.sum() > 1000
                for tile_r in (1, 2, 4):
                    for triple in (0, 2):
                        ctx.set_option("tile_r", tile_r)
                        ctx.set_option("triple_runs", triple)
                        counts, sums, st = _lib.count_pairs(ctx, dev[n1], dev[n2], JOBS, ts[g], kernel="band",
                                                            want_counts=True, want_sums=True)
                        key = (pair, g, tile_r, triple)
                        assert st.kernel_used == _lib.KERNEL_BAND, key
                        assert np.array_equal(counts, exp_c), (grid_on, key)
                        np.testing.assert_allclose(sums, exp_s, rtol=RTOL_W, atol=0, err_msg=str((grid_on, key)))
                        evaluated[key] = st.evaluated_pairs
        for d in dev.values():
            d.free()
    finally:
        ctx.close()
    return evaluated


def test_trimmed_culling_against_oracle(inputs, expected):
    cats, ts = inputs
    on = _count_all(0, cats, ts, expected, True)
    off = _count_all(0, cats, ts, expected, False)
    for key in on:
        assert on[key] < off[key], (key, on[key], off[key])


def test_options_are_validated():
    from yet_another_wizz_amd import _lib

    ctx = _lib.Context(0)
    try:
        for key in ("strip_grid", "band_trim"):
            ctx.set_option(key, 0)
            ctx.set_option(key, 1)
            with pytest.raises(_lib.YawhipError):
                ctx.set_option(key, 2)
    finally:
        ctx.close()
