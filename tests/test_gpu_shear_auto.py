"""GPU: the shear-shear count kernel (``yawhip_shear_auto_count``) and ``autocorrelate_shear`` on the device, against the numpy
brute force of tests/shear_auto_oracle.py.

The rule for the signed sums: per (job, bin, fine bin) cell ``|P - P_o|``, ``|M - M_o|`` and ``|C - C_o|`` are at most
``1e-10 * A``, with ``A = sum |w_a w_b| (|g1a| + |g2a|) (|g1b| + |g2b|)`` the cancellation-free magnitude of the cell's pairs --
the project's weighted-sum tolerance (the per-pair float64 error of a rotation is ~1e-12 at separations
>= 0.5 arcmin, which no test here goes below); a cell without pairs must be exactly 0. ``W`` is a weighted pair count and is
held to rtol 1e-10, and to the pair count of the shipped exact kernel where nothing is weighted."""
import functools

import numpy as np
import pytest

import helpers
import shear_auto_oracle
from conftest import ARCMIN
from yet_another_wizz_amd import _lib, engine
from yet_another_wizz_amd.catalog import radec_to_xyz

pytestmark = pytest.mark.gpu
RTOL_W = helpers.RTOL_W
DEG = np.pi / 180.0
JOBS = np.array([(0, 0), (0, 1), (1, 1), (1, 2)], dtype=np.int32)
N_BINS = 2


def chord2(arcmin):
    return (2.0 * np.sin(0.5 * np.asarray(arcmin, dtype=np.float64) * ARCMIN)) ** 2


def thresholds(nf, n_bins=N_BINS, rmin=0.5, rmax=12.0):
    """f64[B, nf + 1]: log-spaced edges from >= 0.5 to <= 12 arcmin, other limits in every bin."""
    return chord2([np.geomspace(rmin * (1.0 + 0.1 * k), rmax * (1.0 - 0.05 * k), nf + 1) for k in range(n_bins)])


def catalogue(ra, dec, sizes, rng, nb):
    """The oracle's dict of the objects (ra, dec) in the order given, cut into (patch, bin) segments of ``sizes``."""
    x, y, z = radec_to_xyz(ra, dec)
    n = len(x)
    return dict(x=x, y=y, z=z, w=rng.uniform(0.5, 2.0, n), g1=rng.normal(0, 0.3, n), g2=rng.normal(0, 0.3, n), nb=nb,
                off=np.concatenate([[0], np.cumsum(sizes)]).astype(np.int64))


@functools.lru_cache(maxsize=None)
def scene():
    """Three patches side by side in a 3 x 3 degree box (patch p: ra in [p, p + 1] degrees), two redshift bins. Segment sizes
    (patch, bin): (0, 0) a single object near the edge to patch 1, (0, 1) EMPTY, (1, 0) 257 -- one past a lane tile and one past
    a stage --, (1, 1) a knot of 700 inside 2 arcmin at the edge to patch 2 (several tiles and stages, every pair in range),
    (2, 0) 1500 (several lane tiles with a ragged last one), (2, 1) 300."""
    rng = np.random.default_rng(2025)
    sizes = [1, 0, 257, 700, 1500, 300]
    ra, dec = [], []
    for seg, n in enumerate(sizes):
        p = seg // N_BINS
        r, d = rng.uniform(p, p + 1.0, n) * DEG, rng.uniform(0.0, 3.0, n) * DEG
        if seg == 0:
            r, d = np.array([0.95 * DEG]), np.array([1.5 * DEG])
        if seg == 3:
            rad, theta = 2.0 * ARCMIN * np.sqrt(rng.uniform(0, 1, n)), rng.uniform(0, 2 * np.pi, n)
            r, d = 1.97 * DEG + rad * np.cos(theta), 1.2 * DEG + rad * np.sin(theta)
        ra.append(r), dec.append(d)
    return catalogue(np.concatenate(ra), np.concatenate(dec), sizes, rng, N_BINS)


def weighted_scene(weighted):
    cat = scene()
    return cat if weighted else dict(cat, w=None)


@functools.lru_cache(maxsize=None)
def expected(weighted, nf):
    """The oracle's (P, M, C, W, A) of the scene: computed once per weighting and edge count, shared, never modified."""
    out = shear_auto_oracle.shear_auto_jobs(weighted_scene(weighted), JOBS, thresholds(nf))
    for a in out:
        a.setflags(write=False)
    return out


def upload(ctx, cat, sort_axis=2):
    n_patches = (len(cat["off"]) - 1) // cat["nb"]
    return _lib.ShearSources(ctx, cat["x"], cat["y"], cat["z"], cat["w"], cat["g1"], cat["g2"], n_patches, cat["off"],
                             sort_axis=sort_axis, n_bins=cat["nb"])


def count(cat, jobs, t, sort_axis=2):
    ctx = engine.get_context(0)
    sources = upload(ctx, cat, sort_axis)
    try:
        return _lib.shear_auto_count(ctx, sources, jobs, t)
    finally:
        sources.free()


def check_against_oracle(key, got, exp):
    P, M, C, W = got
    P_o, M_o, C_o, W_o, A = exp
    for name, ours, ref in (("P", P, P_o), ("M", M, M_o), ("C", C, C_o)):
        err = np.abs(ours - ref)
        worst = float(np.max(err / np.where(A > 0, A, 1.0)))
        print(f"{key} {name}: worst |ours - oracle| / A = {worst:.3e} over {np.count_nonzero(A)} cells with pairs")
        assert np.all(err <= 1e-10 * A), (key, name, worst)  # every cell (A == 0 allows no error at all)
        assert np.all(ours[A == 0] == 0.0) and not np.any(np.signbit(ours[A == 0])), (key, name)
    assert np.all(W[W_o == 0] == 0.0), key
    np.testing.assert_allclose(W, W_o, rtol=RTOL_W, atol=0, err_msg=key)


def exact_pair_count(cat, jobs, t, sort_axis=2):
    """The unweighted pair count of the shipped exact kernel on the same segments and jobs, the diagonal halved."""
    ctx = engine.get_context(0)
    n_patches = (len(cat["off"]) - 1) // cat["nb"]
    plain = _lib.DeviceCatalog(ctx, cat["x"], cat["y"], cat["z"], None, n_patches, cat["nb"], cat["off"], sort_axis=sort_axis)
    try:
        counts, _, _ = _lib.count_pairs(ctx, plain, plain, jobs, t, kernel="exact")
    finally:
        plain.free()
    jobs = np.asarray(jobs).reshape(-1, 2)
    return counts.astype(np.float64) * np.where(jobs[:, 0] == jobs[:, 1], 0.5, 1.0)[:, None, None]


# --------------------------------------------------------------------------- 1. fine sums against the oracle
@pytest.mark.parametrize("sort_axis", [0, 1, 2])
@pytest.mark.parametrize("nf", [1, 12, 50])
@pytest.mark.parametrize("weighted", [True, False], ids=["weighted", "unweighted"])
def test_fine_sums_match_the_oracle(weighted, nf, sort_axis):
    exp = expected(weighted, nf)
    A = exp[4]
    # cells without pairs -- (0, 0): one object alone, and the empty segment (0, 1) -- next to cells with pairs in every job
    assert np.all(A[0] == 0) and np.all(A[1, 1] == 0) and A[1, 0].sum() > 0 and np.all(A[2:].sum(axis=2) > 0)
    P, M, C, W, stats = count(weighted_scene(weighted), JOBS, thresholds(nf), sort_axis)
    assert stats.n_workgroups == len(JOBS) * N_BINS and stats.evaluated_pairs > 0
    check_against_oracle(f"{'weighted' if weighted else 'unweighted'} nf={nf} axis={sort_axis}", (P, M, C, W), exp)


# --------------------------------------------------------------------------- 2. W against the shipped count
@pytest.mark.parametrize("sort_axis", [2, 0])
def test_w_equals_the_exact_pair_count(sort_axis):
    cat = weighted_scene(False)
    t = thresholds(12)
    W = count(cat, JOBS, t, sort_axis)[3]
    pairs = exact_pair_count(cat, JOBS, t, sort_axis)
    assert pairs.sum() > 100000 and np.array_equal(W, pairs)


# --------------------------------------------------------------------------- 3. the diagonal
def test_diagonal_cells_hold_every_unordered_pair_once():
    """One patch against the oracle's unordered sum; then the same objects cut into two patches: the cross job holds the
    oracle's pairs between the two parts, and the three cells together every pair of the whole."""
    rng = np.random.default_rng(31)
    n, cut = 1100, 470
    ra, dec = rng.uniform(10.0, 10.6, n) * DEG, rng.uniform(-0.3, 0.3, n) * DEG
    t = thresholds(12, n_bins=1)
    whole = catalogue(ra, dec, [n], rng, 1)
    split = dict(whole, off=np.array([0, cut, n], dtype=np.int64))
    got_whole = count(whole, [[0, 0]], t)[:4]
    exp_whole = shear_auto_oracle.shear_auto_jobs(whole, [[0, 0]], t)
    check_against_oracle("diagonal", got_whole, exp_whole)
    jobs = np.array([(0, 0), (1, 1), (0, 1)], dtype=np.int32)
    got_split = count(split, jobs, t)[:4]
    exp_split = shear_auto_oracle.shear_auto_jobs(split, jobs, t)
    assert exp_split[3][2].sum() > 1000  # pairs across the cut
    check_against_oracle("split", got_split, exp_split)
    unweighted = (dict(whole, w=None), dict(split, w=None))
    W_whole, W_split = count(unweighted[0], [[0, 0]], t)[3], count(unweighted[1], jobs, t)[3]
    assert np.array_equal(W_whole[0], W_split.sum(axis=0)) and np.array_equal(W_whole, exact_pair_count(unweighted[0], [[0, 0]], t))


# --------------------------------------------------------------------------- 4. window edges
@pytest.mark.parametrize("anchors", ["streamed", "in lanes"])
@pytest.mark.parametrize("sort_axis", [0, 1, 2])
def test_window_edges(sort_axis, anchors):
    """Partners displaced from an anchor along the sort axis only, by the chord of an inner / outer bin edge times
    (1 -/+ 1e-9), around the anchors that come first and last in their segment: the key window of a lane tile has to reach
    exactly as far as the predicate does. The anchors are the streamed segment (patch 0 of job (0, 1)) or sit in the lanes
    (patch 1). (The displaced partners are not unit vectors; the count does not need that.)"""
    rng = np.random.default_rng(7 + sort_axis)
    ra, dec = rng.uniform(40.0, 40.5, 40) * DEG, rng.uniform(30.0, 30.5, 40) * DEG
    anchor_xyz = np.array(radec_to_xyz(ra, dec))  # [3, n]
    t = chord2([[0.5, 3.0, 12.0]])
    first, last = np.argmin(anchor_xyz[sort_axis]), np.argmax(anchor_xyz[sort_axis])
    placed = []
    for at in (first, last):
        for edge in (t[0, 0], t[0, 2]):
            for factor in (1.0 - 1e-9, 1.0 + 1e-9):
                for sign in (-1.0, 1.0):
                    p = anchor_xyz[:, at].copy()
                    p[sort_axis] += sign * np.sqrt(edge) * factor
                    placed.append(p)
    fra, fdec = rng.uniform(40.0, 40.5, 300) * DEG, rng.uniform(30.0, 30.5, 300) * DEG  # filler: two lane tiles / stages
    partner_xyz = np.concatenate([np.array(placed).T, np.array(radec_to_xyz(fra, fdec))], axis=1)
    parts = (anchor_xyz, partner_xyz) if anchors == "streamed" else (partner_xyz, anchor_xyz)
    xyz = np.concatenate(parts, axis=1)
    n = xyz.shape[1]
    cat = dict(x=xyz[0].copy(), y=xyz[1].copy(), z=xyz[2].copy(), w=None, g1=rng.normal(0, 0.3, n), g2=rng.normal(0, 0.3, n), nb=1,
               off=np.array([0, parts[0].shape[1], n], dtype=np.int64))
    jobs = np.array([[0, 1]], dtype=np.int32)
    exp = shear_auto_oracle.shear_auto_jobs(cat, jobs, t)
    # the anchors and the placed partners alone: edge pairs are counted, in both fine bins
    only = np.r_[0:40 + len(placed)] if anchors == "streamed" else np.r_[0:len(placed), n - 40:n]
    few = dict(cat, **{c: cat[c][only] for c in ("x", "y", "z", "g1", "g2")},
               off=np.array([0, 40 if anchors == "streamed" else len(placed), 40 + len(placed)], dtype=np.int64))
    W_placed = shear_auto_oracle.shear_auto_jobs(few, jobs, t)[3]
    assert W_placed[0, 0, 0] > 0 and W_placed[0, 0, 1] > 0
    P, M, C, W, _ = count(cat, jobs, t, sort_axis)
    assert np.array_equal(W, exp[3]) and np.array_equal(W, exact_pair_count(cat, jobs, t, sort_axis))
    check_against_oracle(f"edges axis={sort_axis} anchors {anchors}", (P, M, C, W), exp)


# --------------------------------------------------------------------------- 5. reproducibility
def test_two_calls_return_the_same_bits():
    ctx = engine.get_context(0)
    sources = upload(ctx, weighted_scene(True))
    try:
        one = _lib.shear_auto_count(ctx, sources, JOBS, thresholds(50))[:4]
        two = _lib.shear_auto_count(ctx, sources, JOBS, thresholds(50))[:4]
    finally:
        sources.free()
    assert np.count_nonzero(one[0]) > 100
    for a, b in zip(one, two):
        assert np.array_equal(a, b)


# --------------------------------------------------------------------------- 6. pole guard
@pytest.mark.parametrize("pole_patch", [0, 1], ids=["pole streamed", "pole in lanes"])
def test_an_object_on_the_pole_adds_to_w_only(pole_patch):
    """One object exactly at dec = +90 degrees with partners 1 to 5 arcmin away, in its own patch (diagonal job) and in the
    other (job (0, 1), the pole object on either side of the pair): its pairs add to W and to nothing else."""
    rng = np.random.default_rng(41)
    n = 7
    ra, dec = rng.uniform(0.0, 2.0 * np.pi, n), 0.5 * np.pi - rng.uniform(1.0, 5.0, n) * ARCMIN
    x, y, z = radec_to_xyz(ra, dec)
    at = 0 if pole_patch == 0 else 4  # first object of its patch
    x, y, z = (np.insert(c, at, v) for c, v in ((x, 0.0), (y, 0.0), (z, 1.0)))
    w = np.array([0.5, 0.75, 1.0, 1.25, 1.5, 1.75, 2.0, 0.25])  # dyadic: the sums of products are exact
    cat = dict(x=x, y=y, z=z, w=w, g1=rng.normal(0, 0.3, n + 1), g2=rng.normal(0, 0.3, n + 1), nb=1, off=np.array([0, 4, 8], dtype=np.int64))
    keep = np.arange(n + 1) != at
    without = dict(cat, **{c: cat[c][keep] for c in ("x", "y", "z", "w", "g1", "g2")},
                   off=np.array([0, 3, 7] if pole_patch == 0 else [0, 4, 7], dtype=np.int64))
    t = chord2([[0.5, 12.0]])
    jobs = np.array([(0, 0), (1, 1), (0, 1)], dtype=np.int32)
    exp, exp_without = shear_auto_oracle.shear_auto_jobs(cat, jobs, t), shear_auto_oracle.shear_auto_jobs(without, jobs, t)
    for a, b in zip(exp[:3], exp_without[:3]):
        assert np.array_equal(a, b)  # (the oracle: nothing from the pole object)
    P, M, C, W, _ = count(cat, jobs, t)
    assert np.all(np.isfinite(P)) and np.all(np.isfinite(M)) and np.all(np.isfinite(C))
    check_against_oracle(f"pole in patch {pole_patch}", (P, M, C, W), exp)
    W_without = count(without, jobs, t)[3]
    own, other = (0, 1) if pole_patch == 0 else (1, 0)
    in_own = w[:4].sum() - w[at] if pole_patch == 0 else w[4:].sum() - w[at]
    in_other = w[4:].sum() if pole_patch == 0 else w[:4].sum()
    assert W[own, 0, 0] == W_without[own, 0, 0] + w[at] * in_own          # every partner is within 5' of the pole
    assert W[2, 0, 0] == W_without[2, 0, 0] + w[at] * in_other
    assert W[other, 0, 0] == W_without[other, 0, 0] > 0


# --------------------------------------------------------------------------- 7. the edge cap
def test_the_edge_cap_runs():
    """256 edges, the most the entry point takes (its largest block of LDS), on the knot and its neighbour."""
    t = thresholds(255)
    jobs = np.array([(1, 1), (1, 2)], dtype=np.int32)
    check_against_oracle("nf=255", count(scene(), jobs, t)[:4], shear_auto_oracle.shear_auto_jobs(scene(), jobs, t))


# --------------------------------------------------------------------------- 8. end to end
def test_autocorrelate_shear_end_to_end():
    """The scenario of the CPU driver test through the real library: the same assertions."""
    from test_shear_auto_host import check_auto_scenario

    check_auto_scenario()


# --------------------------------------------------------------------------- 9. refusals
def test_refusals():
    ctx = engine.get_context(0)
    cat = weighted_scene(False)
    binned = upload(ctx, cat)
    unbinned = _lib.ShearSources(ctx, cat["x"], cat["y"], cat["z"], None, cat["g1"], cat["g2"], 3, cat["off"][::N_BINS].copy())
    lenses = _lib.DeviceCatalog(ctx, cat["x"], cat["y"], cat["z"], None, 3, N_BINS, cat["off"])
    try:
        with pytest.raises(_lib.YawhipError, match="binned in redshift"):
            _lib.shear_count(ctx, lenses, binned, JOBS, thresholds(1))
        with pytest.raises(_lib.YawhipError, match="does not fit"):
            _lib.shear_auto_count(ctx, unbinned, JOBS, thresholds(1))
        with pytest.raises(_lib.YawhipError, match="p <= q"):
            _lib.shear_auto_count(ctx, binned, np.array([(0, 0), (2, 1)], dtype=np.int32), thresholds(1))
        with pytest.raises(_lib.YawhipError, match="max edges 256"):
            _lib.shear_auto_count(ctx, binned, JOBS, thresholds(256))
        P, M, C, W, _ = _lib.shear_auto_count(ctx, binned, JOBS, thresholds(1))  # the handle is still good
        assert W.sum() > 0
    finally:
        binned.free(), unbinned.free(), lenses.free()
