"""GPU: the shear count kernel (``yawhip_shear_count``) and ``crosscorrelate_shear`` on the device, against the numpy brute
force of tests/shear_oracle.py.

The rule for the signed sums: per (job, bin, fine bin) cell ``|T - T_o| <= 1e-10 * A`` and the same for ``X``, with ``A`` the
cancellation-free magnitude ``sum |ww| (|g1| + |g2|)`` of the cell's pairs -- the project's weighted-sum tolerance (the per-pair
float64 error of the projection is ~1e-12 at separations >= 0.5 arcmin, which no test here goes below); a cell without pairs
must be exactly 0. ``W`` is a weighted pair count and is held to rtol 1e-10, and to equality where nothing is weighted."""
import functools

import numpy as np
import pytest

import helpers
import shear_oracle
from conftest import ARCMIN
from yet_another_wizz_amd import _lib, engine
from yet_another_wizz_amd.catalog import radec_to_xyz

pytestmark = pytest.mark.gpu
RTOL_W = helpers.RTOL_W
DEG = np.pi / 180.0
JOBS = np.array([(0, 0), (1, 1), (2, 2), (0, 1), (1, 0), (1, 2)], dtype=np.int32)
N_BINS = 4


def thresholds(nf, n_bins=N_BINS, rmin=0.5, rmax=12.0):
    """f64[B, nf + 1]: log-spaced edges from >= 0.5 to <= 12 arcmin, other limits in every bin."""
    rows = [np.geomspace(rmin * (1.0 + 0.1 * k), rmax * (1.0 - 0.05 * k), nf + 1) * ARCMIN for k in range(n_bins)]
    return (2.0 * np.sin(0.5 * np.array(rows))) ** 2


@functools.lru_cache(maxsize=None)
def scene():
    """Three patches side by side in a 3 x 3 degree box (patch p: ra in [p, p + 1] degrees). Sources: 1, 257 and 1500 objects
    -- a single lane, one past a full lane tile, several tiles with a ragged last one. Lenses in four redshift bins: segment
    (0, 3) is empty, segment (1, 2) holds 700 lenses inside 2 arcmin (its window spans several 256-object stages)."""
    rng = np.random.default_rng(2024)

    def box(p, n):
        return rng.uniform(p, p + 1.0, n) * DEG, rng.uniform(0.0, 3.0, n) * DEG

    src_ra, src_dec, src_off = [], [], [0]
    for p, n in enumerate((1, 257, 1500)):
        ra, dec = box(p, n)
        if p == 0:
            ra, dec = np.array([0.95 * DEG]), np.array([1.5 * DEG])  # the single source: near the edge to patch 1
        src_ra.append(ra), src_dec.append(dec), src_off.append(src_off[-1] + n)
    lens_ra, lens_dec, lens_off = [], [], [0]
    for p in range(3):
        for k in range(N_BINS):
            n = 0 if (p, k) == (0, 3) else int(rng.integers(250, 350))
            ra, dec = box(p, n)
            if (p, k) == (1, 2):  # a knot of 700 inside 2 arcmin, at the edge to patch 2
                r, theta = 2.0 * ARCMIN * np.sqrt(rng.uniform(0, 1, 700)), rng.uniform(0, 2 * np.pi, 700)
                ra, dec = 1.97 * DEG + r * np.cos(theta), 1.2 * DEG + r * np.sin(theta)
                n = 700
            lens_ra.append(ra), lens_dec.append(dec), lens_off.append(lens_off[-1] + n)
    src_ra, src_dec, lens_ra, lens_dec = (np.concatenate(c) for c in (src_ra, src_dec, lens_ra, lens_dec))
    sx, sy, sz = radec_to_xyz(src_ra, src_dec)
    lx, ly, lz = radec_to_xyz(lens_ra, lens_dec)
    src = dict(x=sx, y=sy, z=sz, w=rng.uniform(0.5, 2.0, len(sx)), g1=rng.normal(0, 0.3, len(sx)), g2=rng.normal(0, 0.3, len(sx)),
               off=np.array(src_off, dtype=np.int64))
    lens = dict(x=lx, y=ly, z=lz, w=rng.uniform(0.5, 2.0, len(lx)), nb=N_BINS, off=np.array(lens_off, dtype=np.int64))
    return lens, src


def weighted_scene(weights):
    """The scene with ``weights`` = "both" / "lenses" / "none" of the weight columns kept."""
    lens, src = scene()
    lens = dict(lens, w=lens["w"] if weights in ("both", "lenses") else None)
    src = dict(src, w=src["w"] if weights == "both" else None)
    return lens, src


@functools.lru_cache(maxsize=None)
def expected(weights, nf):
    """The oracle's (T, X, W, A) of the scene: computed once per weighting and edge count, shared, never modified."""
    lens, src = weighted_scene(weights)
    out = shear_oracle.shear_jobs(lens, src, JOBS, thresholds(nf))
    for a in out:
        a.setflags(write=False)
    return out


def upload(ctx, lens, src, sort_axis, src_axis=None):
    n_patches = len(src["off"]) - 1
    lenses = _lib.DeviceCatalog(ctx, lens["x"], lens["y"], lens["z"], lens["w"], n_patches, lens["nb"], lens["off"], sort_axis=sort_axis)
    sources = _lib.ShearSources(ctx, src["x"], src["y"], src["z"], src["w"], src["g1"], src["g2"], n_patches, src["off"],
                                sort_axis=sort_axis if src_axis is None else src_axis)
    return lenses, sources


def check_against_oracle(key, got, exp):
    T, X, W = got
    T_o, X_o, W_o, A = exp
    for name, ours, ref in (("T", T, T_o), ("X", X, X_o)):
        err = np.abs(ours - ref)
        worst = float(np.max(err / np.where(A > 0, A, 1.0)))
        print(f"{key} {name}: worst |ours - oracle| / A = {worst:.3e} over {np.count_nonzero(A)} cells with pairs")
        assert np.all(err <= 1e-10 * A), (key, name, worst)  # every cell (A == 0 allows no error at all)
        assert np.all(ours[A == 0] == 0.0) and not np.any(np.signbit(ours[A == 0])), (key, name)
    assert np.all(W[W_o == 0] == 0.0), key
    np.testing.assert_allclose(W, W_o, rtol=RTOL_W, atol=0, err_msg=key)


# --------------------------------------------------------------------------- 1. fine sums against the oracle
@pytest.mark.parametrize("sort_axis", [0, 1, 2])
@pytest.mark.parametrize("nf", [1, 12, 50])
@pytest.mark.parametrize("weights", ["both", "lenses", "none"])
def test_fine_sums_match_the_oracle(weights, nf, sort_axis):
    ctx = engine.get_context(0)
    exp = expected(weights, nf)
    assert np.count_nonzero(exp[3]) >= 21 and np.any(exp[3] == 0)  # cells with pairs in every job, and empty ones
    lenses, sources = upload(ctx, *weighted_scene(weights), sort_axis)
    try:
        T, X, W, stats = _lib.shear_count(ctx, lenses, sources, JOBS, thresholds(nf))
    finally:
        lenses.free(), sources.free()
    assert stats.n_workgroups == len(JOBS) * N_BINS and 0 < stats.evaluated_pairs <= stats.candidate_pairs
    check_against_oracle(f"{weights} nf={nf} axis={sort_axis}", (T, X, W), exp)


def test_unbinned_lenses_under_two_redshift_bins():
    """Lenses without redshift bins (``nb = 1``) under the thresholds of two bins: both cells of a job stream the one lens
    segment of its patch, each with the edges of its own bin."""
    lens, src = weighted_scene("both")
    lens = dict(lens, nb=1, off=lens["off"][::N_BINS].copy())  # the scene's lenses with their bin boundaries dropped
    t = thresholds(12, n_bins=2)
    exp = shear_oracle.shear_jobs(lens, src, JOBS, t)
    assert np.all(exp[3].sum(axis=2) > 0)  # both bins hold pairs in every job ...
    assert not np.any(np.all(exp[2][:, 0] == exp[2][:, 1], axis=1))  # ... and no job has the same sums in the two
    ctx = engine.get_context(0)
    lenses, sources = upload(ctx, lens, src, 2)
    try:
        T, X, W, stats = _lib.shear_count(ctx, lenses, sources, JOBS, t)
    finally:
        lenses.free(), sources.free()
    assert stats.n_workgroups == len(JOBS) * 2 and 0 < stats.evaluated_pairs <= stats.candidate_pairs
    check_against_oracle("unbinned lenses, two bins", (T, X, W), exp)


# --------------------------------------------------------------------------- 2. W against the shipped count
@pytest.mark.parametrize("axes", [(2, 2), (1, 1), (2, 0)], ids=["z", "y", "lens z, sources x"])
@pytest.mark.parametrize("weights", ["both", "none"])
def test_w_equals_the_exact_pair_count(weights, axes):
    """The shear kernel selects precisely the pairs the tested count selects -- also when the two sides are sorted along
    different axes and the window is the whole segment."""
    ctx = engine.get_context(0)
    lens, src = weighted_scene(weights)
    t = thresholds(12)
    lenses, sources = upload(ctx, lens, src, axes[0], axes[1])
    plain = _lib.DeviceCatalog(ctx, src["x"], src["y"], src["z"], src["w"], 3, 1, src["off"], sort_axis=axes[0])
    try:
        _, _, W, _ = _lib.shear_count(ctx, lenses, sources, JOBS, t)
        counts, sums, _ = _lib.count_pairs(ctx, lenses, plain, JOBS, t, kernel="exact")
    finally:
        lenses.free(), sources.free(), plain.free()
    if weights == "none":
        assert counts.sum() > 10000 and np.array_equal(W, counts.astype(np.float64))
    else:
        assert np.all(W[sums == 0] == 0.0)
        np.testing.assert_allclose(W, sums, rtol=RTOL_W, atol=0)


# --------------------------------------------------------------------------- 3. window edges
@pytest.mark.parametrize("sort_axis", [0, 1, 2])
def test_window_edges(sort_axis):
    """Sources displaced from a lens along the sort axis only, by the chord of an inner / outer bin edge times (1 -/+ 1e-9),
    around the lenses that come first and last in their segment: the key window of a lane tile has to reach exactly as far
    as the predicate does. (The displaced sources are not unit vectors; neither count needs that.)"""
    rng = np.random.default_rng(7 + sort_axis)
    ra, dec = rng.uniform(40.0, 40.5, 40) * DEG, rng.uniform(30.0, 30.5, 40) * DEG
    lens_xyz = np.array(radec_to_xyz(ra, dec))  # [3, n]
    t = (2.0 * np.sin(0.5 * np.array([[0.5, 3.0, 12.0]]) * ARCMIN)) ** 2
    first, last = np.argmin(lens_xyz[sort_axis]), np.argmax(lens_xyz[sort_axis])
    placed = []
    for at in (first, last):
        for edge in (t[0, 0], t[0, 2]):
            for factor in (1.0 - 1e-9, 1.0 + 1e-9):
                for sign in (-1.0, 1.0):
                    p = lens_xyz[:, at].copy()
                    p[sort_axis] += sign * np.sqrt(edge) * factor
                    placed.append(p)
    fra, fdec = rng.uniform(40.0, 40.5, 300) * DEG, rng.uniform(30.0, 30.5, 300) * DEG  # filler: two lane tiles
    src_xyz = np.concatenate([np.array(placed).T, np.array(radec_to_xyz(fra, fdec))], axis=1)
    n = src_xyz.shape[1]
    lens = dict(x=lens_xyz[0].copy(), y=lens_xyz[1].copy(), z=lens_xyz[2].copy(), w=None, nb=1, off=np.array([0, 40], dtype=np.int64))
    src = dict(x=src_xyz[0].copy(), y=src_xyz[1].copy(), z=src_xyz[2].copy(), w=None, g1=rng.normal(0, 0.3, n), g2=rng.normal(0, 0.3, n),
               off=np.array([0, n], dtype=np.int64))
    jobs = np.array([[0, 0]], dtype=np.int32)
    T_o, X_o, W_o, A = shear_oracle.shear_jobs(lens, src, jobs, t)
    only_placed = dict(src, **{c: src[c][:len(placed)] for c in ("x", "y", "z", "g1", "g2")}, off=np.array([0, len(placed)]))
    W_placed = shear_oracle.shear_jobs(lens, only_placed, jobs, t)[2]
    assert 0 < W_placed.sum() and W_placed[0, 0, 0] > 0 and W_placed[0, 0, 1] > 0  # edge pairs on both sides of being counted
    ctx = engine.get_context(0)
    lenses, sources = upload(ctx, lens, src, sort_axis)
    plain = _lib.DeviceCatalog(ctx, src["x"], src["y"], src["z"], None, 1, 1, src["off"], sort_axis=sort_axis)
    try:
        T, X, W, _ = _lib.shear_count(ctx, lenses, sources, jobs, t)
        counts, _, _ = _lib.count_pairs(ctx, lenses, plain, jobs, t, kernel="exact")
    finally:
        lenses.free(), sources.free(), plain.free()
    assert np.array_equal(W, W_o) and np.array_equal(W, counts.astype(np.float64))
    check_against_oracle(f"edges axis={sort_axis}", (T, X, W), (T_o, X_o, W_o, A))


# --------------------------------------------------------------------------- 4. reproducibility
def test_two_calls_return_the_same_bits():
    ctx = engine.get_context(0)
    lenses, sources = upload(ctx, *weighted_scene("both"), 2)
    try:
        one = _lib.shear_count(ctx, lenses, sources, JOBS, thresholds(50))[:3]
        two = _lib.shear_count(ctx, lenses, sources, JOBS, thresholds(50))[:3]
    finally:
        lenses.free(), sources.free()
    assert np.count_nonzero(one[0]) > 100
    for a, b in zip(one, two):
        assert np.array_equal(a, b)


# --------------------------------------------------------------------------- 5. pole guard
def test_a_source_on_the_pole_adds_to_w_only():
    ctx = engine.get_context(0)
    (lx,), (ly,), (lz,) = radec_to_xyz(np.array([1.0]), np.array([0.5 * np.pi - 3.0 * ARCMIN]))
    (ox,), (oy,), (oz,) = radec_to_xyz(np.array([1.3]), np.array([0.5 * np.pi - 5.0 * ARCMIN]))
    t = (2.0 * np.sin(0.5 * np.array([[0.5, 12.0]]) * ARCMIN)) ** 2
    jobs = np.array([[0, 0]], dtype=np.int32)
    lens = dict(x=np.array([lx]), y=np.array([ly]), z=np.array([lz]), w=np.array([1.5]), nb=1, off=np.array([0, 1], dtype=np.int64))
    with_pole = dict(x=np.array([0.0, ox]), y=np.array([0.0, oy]), z=np.array([1.0, oz]), w=np.array([0.75, 1.25]),
                     g1=np.array([0.5, 0.1]), g2=np.array([0.3, -0.2]), off=np.array([0, 2], dtype=np.int64))
    without = dict(x=np.array([ox]), y=np.array([oy]), z=np.array([oz]), w=np.array([1.25]), g1=np.array([0.1]),
                   g2=np.array([-0.2]), off=np.array([0, 1], dtype=np.int64))
    results = []
    for src in (with_pole, without):
        lenses, sources = upload(ctx, lens, src, 2)
        try:
            results.append(_lib.shear_count(ctx, lenses, sources, jobs, t)[:3])
        finally:
            lenses.free(), sources.free()
    (T, X, W), (T1, X1, W1) = results
    assert np.all(np.isfinite(T)) and np.all(np.isfinite(X))
    assert T1[0, 0, 0] != 0.0 and np.array_equal(T, T1) and np.array_equal(X, X1)  # nothing from the source on the pole ...
    assert W[0, 0, 0] == W1[0, 0, 0] + 1.5 * 0.75 and W1[0, 0, 0] == 1.5 * 1.25    # ... but W includes it
    check_against_oracle("pole", (T, X, W), shear_oracle.shear_jobs(lens, with_pole, jobs, t))


# --------------------------------------------------------------------------- 6. end to end
@pytest.mark.parametrize("with_randoms", [False, True], ids=["dd", "dd-dr"])
def test_crosscorrelate_shear_end_to_end(with_randoms):
    """The scenario of the CPU driver test through the real library: the same assertions."""
    from test_shear_host import check_shear_scenario

    check_shear_scenario(with_randoms)


# --------------------------------------------------------------------------- 7. error paths
def test_mismatched_handles_are_refused():
    ctx = engine.get_context(0)
    other = _lib.Context(0)
    lens, src = weighted_scene("none")
    t = thresholds(1)
    lenses, sources = upload(ctx, lens, src, 2)
    foreign = _lib.DeviceCatalog(other, lens["x"], lens["y"], lens["z"], None, 3, N_BINS, lens["off"])
    two_patches = _lib.ShearSources(ctx, src["x"], src["y"], src["z"], None, src["g1"], src["g2"], 2,
                                    np.array([0, 258, len(src["x"])], dtype=np.int64))
    try:
        with pytest.raises(_lib.YawhipError, match="another context"):
            _lib.shear_count(ctx, foreign, sources, JOBS, t)
        with pytest.raises(_lib.YawhipError, match="another context"):
            _lib.shear_count(other, foreign, sources, JOBS, t)
        with pytest.raises(_lib.YawhipError, match="patch counts differ"):
            _lib.shear_count(ctx, lenses, two_patches, JOBS, t)
        with pytest.raises(_lib.YawhipError, match="not ascending"):
            _lib.shear_count(ctx, lenses, sources, JOBS, t[:, ::-1].copy())
        with pytest.raises(_lib.YawhipError, match="does not fit"):
            _lib.shear_count(ctx, lenses, sources, JOBS, thresholds(1, n_bins=3))
    finally:
        lenses.free(), sources.free(), foreign.free(), two_patches.free()
        other.close()
