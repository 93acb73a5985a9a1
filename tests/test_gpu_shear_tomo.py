"""GPU: the shear-shear count between (patch, bin) segments of one or two handles (``yawhip_shear_pair_count``) and
``correlate_shear_tomographic`` on the device, against the numpy brute force of tests/shear_pair_oracle.py.

The scene and the rule for the signed sums are those of tests/test_gpu_shear_auto.py: per cell and fine bin ``|P - P_o|``,
``|M - M_o|`` and ``|C - C_o|`` are at most ``1e-10 * A`` with ``A = sum |w_a w_b| (|g1a| + |g2a|) (|g1b| + |g2b|)``, a cell
without pairs is exactly 0, ``W`` is held to ``helpers.RTOL_W`` (nothing here is closer than 0.5 arcmin)."""
import functools

import numpy as np
import pytest

import helpers
import shear_pair_oracle
from conftest import ARCMIN
from test_gpu_shear_auto import DEG, JOBS, N_BINS, catalogue, check_against_oracle, chord2, scene, thresholds, upload, weighted_scene
from yet_another_wizz_amd import _lib, engine
from yet_another_wizz_amd.catalog import radec_to_xyz

pytestmark = pytest.mark.gpu
RTOL_W = helpers.RTOL_W

PATCH_JOBS = [(0, 0), (0, 1), (1, 0), (1, 1), (1, 2)]


def one_handle_cells():
    """(ka, kb) in {(0, 0), (0, 1), (1, 1)} x the patch jobs x BOTH thresholds rows; inside one bin only p <= q."""
    return np.array([(p, q, ka, kb, row) for ka, kb in ((0, 0), (0, 1), (1, 1)) for p, q in PATCH_JOBS for row in (0, 1)
                     if ka != kb or p <= q], dtype=np.int32)


@functools.lru_cache(maxsize=None)
def expected(weighted, nf):
    """The oracle's (P, M, C, W, A) of ``one_handle_cells`` on the scene: once per weighting and edge count, never modified."""
    cat = weighted_scene(weighted)
    out = shear_pair_oracle.shear_pair_cells(cat, cat, one_handle_cells(), thresholds(nf))
    for a in out:
        a.setflags(write=False)
    return out


@functools.lru_cache(maxsize=None)
def second_scene():
    """A second catalogue on the patches of the scene with other segment sizes (patch, bin): (0, 0) 300, (0, 1) 257, (1, 0)
    EMPTY, (1, 1) 40 objects inside the scene's knot, (2, 0) 500, (2, 1) a single object."""
    rng = np.random.default_rng(2026)
    sizes = [300, 257, 0, 40, 500, 1]
    ra, dec = [], []
    for seg, n in enumerate(sizes):
        p = seg // N_BINS
        r, d = rng.uniform(p, p + 1.0, n) * DEG, rng.uniform(0.0, 3.0, n) * DEG
        if seg == 3:
            rad, theta = 2.0 * ARCMIN * np.sqrt(rng.uniform(0, 1, n)), rng.uniform(0, 2 * np.pi, n)
            r, d = 1.97 * DEG + rad * np.cos(theta), 1.2 * DEG + rad * np.sin(theta)
        ra.append(r), dec.append(d)
    return catalogue(np.concatenate(ra), np.concatenate(dec), sizes, rng, N_BINS)


def two_handle_cells():
    """Every (ka, kb) x patch pairs in both orders and p == q; the thresholds row is ka."""
    return np.array([(p, q, ka, kb, ka) for ka in (0, 1) for kb in (0, 1)
                     for p, q in ((0, 0), (1, 1), (2, 2), (0, 1), (1, 0), (1, 2), (2, 1))], dtype=np.int32)


def swapped(cells):
    return np.ascontiguousarray(cells[:, [1, 0, 3, 2, 4]])


def count(cat_a, cat_b, cells, t, axis_a=2, axis_b=2):
    """One call on fresh handles; ``cat_b is cat_a`` is ONE handle passed twice."""
    ctx = engine.get_context(0)
    a = upload(ctx, cat_a, axis_a)
    b = a if cat_b is cat_a else upload(ctx, cat_b, axis_b)
    try:
        return _lib.shear_pair_count(ctx, a, b, cells, t)
    finally:
        a.free()
        if b is not a:
            b.free()


# --------------------------------------------------------------------------- 1. one handle against the oracle
@pytest.mark.parametrize("sort_axis", [0, 1, 2])
@pytest.mark.parametrize("nf", [1, 12, 50])
@pytest.mark.parametrize("weighted", [True, False], ids=["weighted", "unweighted"])
def test_one_handle_matches_the_oracle(weighted, nf, sort_axis):
    exp = expected(weighted, nf)
    cells, A = one_handle_cells(), exp[4]
    with_pairs = A.sum(axis=1) > 0
    # cells without pairs -- the single object, the empty segment -- next to cells with pairs, in both thresholds rows,
    # inside a bin (diagonal and not) and across the two bins
    assert np.any(~with_pairs) and all(np.any(with_pairs & (cells[:, 4] == row) & (cells[:, 2] == ka) & (cells[:, 3] == kb))
                                       for row in (0, 1) for ka, kb in ((0, 0), (0, 1), (1, 1)))
    cat = weighted_scene(weighted)
    P, M, C, W, stats = count(cat, cat, cells, thresholds(nf), sort_axis, sort_axis)
    assert stats.n_workgroups == len(cells) and stats.evaluated_pairs > 0
    check_against_oracle(f"{'weighted' if weighted else 'unweighted'} nf={nf} axis={sort_axis}", (P, M, C, W), exp)


def test_the_edge_cap_runs():
    """256 edges, the most the entry point takes (its largest block of LDS), on the knot, across its bins and patches."""
    t = thresholds(255)
    cells = np.array([(1, 1, 1, 1, 1), (1, 1, 0, 1, 0), (1, 2, 1, 0, 1), (2, 1, 0, 1, 0)], dtype=np.int32)
    cat = scene()
    check_against_oracle("nf=255", count(cat, cat, cells, t)[:4], shear_pair_oracle.shear_pair_cells(cat, cat, cells, t))


# --------------------------------------------------------------------------- 2. the auto count's bits
@pytest.mark.parametrize("sort_axis", [2, 0])
def test_same_bin_cells_return_the_bits_of_the_auto_count(sort_axis):
    ctx = engine.get_context(0)
    t = thresholds(50)
    cells = np.array([(p, q, k, k, k) for p, q in JOBS for k in range(N_BINS)], dtype=np.int32)
    sources = upload(ctx, weighted_scene(True), sort_axis)
    try:
        auto = _lib.shear_auto_count(ctx, sources, JOBS, t)
        pair = _lib.shear_pair_count(ctx, sources, sources, cells, t)
    finally:
        sources.free()
    assert np.count_nonzero(auto[0]) > 100
    for ours, ref in zip(pair[:4], auto[:4]):
        assert np.array_equal(ours.reshape(ref.shape), ref)
    assert pair[4].evaluated_pairs == auto[4].evaluated_pairs and pair[4].candidate_pairs == auto[4].candidate_pairs


# --------------------------------------------------------------------------- 3. two handles
@pytest.mark.parametrize("sort_axis", [2, 1])
def test_two_handles_match_the_oracle(sort_axis):
    a, b, cells, t = scene(), second_scene(), two_handle_cells(), thresholds(12)
    exp = shear_pair_oracle.shear_pair_cells(a, b, cells, t)
    assert np.count_nonzero(exp[4].sum(axis=1)) >= 12 and np.any(exp[4].sum(axis=1) == 0)
    check_against_oracle(f"two handles axis={sort_axis}", count(a, b, cells, t, sort_axis, sort_axis)[:4], exp)


def test_no_cell_between_two_handles_is_diagonal():
    """The scene uploaded twice: cell (p, p, k, k) of the two handles holds every ORDERED pair -- the oracle's both-ways sum
    and twice the unordered count of the one-handle cell."""
    cat, t = weighted_scene(False), thresholds(12)
    cells = np.array([(1, 1, 1, 1, 1), (2, 2, 0, 0, 0), (1, 1, 0, 0, 0), (0, 0, 0, 0, 0)], dtype=np.int32)
    twin = dict(cat)
    got = count(cat, twin, cells, t)
    exp = shear_pair_oracle.shear_pair_cells(cat, twin, cells, t)
    check_against_oracle("twin handles", got[:4], exp)
    once = count(cat, cat, cells, t)
    assert once[3][:3].sum() > 100000 and np.array_equal(got[3], 2.0 * once[3]) and np.array_equal(got[3], exp[3])
    assert np.all(np.abs(got[0] - 2.0 * once[0]) <= 1e-10 * exp[4])


def test_different_sort_axes_stream_the_whole_segment():
    """Handles sorted along different axes: no key window. Against the oracle; W is that of the windowed call."""
    a, b, cells, t = scene(), second_scene(), two_handle_cells(), thresholds(12)
    exp = shear_pair_oracle.shear_pair_cells(a, b, cells, t)
    *got, stats = count(a, b, cells, t, 2, 0)
    check_against_oracle("axes 2 and 0", got, exp)
    plain_a, plain_b = dict(a, w=None), dict(b, w=None)
    *mixed, stats_mixed = count(plain_a, plain_b, cells, t, 1, 2)
    *same, stats_same = count(plain_a, plain_b, cells, t, 2, 2)
    assert same[3].sum() > 10000 and np.array_equal(mixed[3], same[3])
    assert stats_mixed.evaluated_pairs == stats_mixed.candidate_pairs > stats_same.evaluated_pairs  # every pair of every cell


# --------------------------------------------------------------------------- 4. swap symmetry
@pytest.mark.parametrize("weighted", [True, False], ids=["weighted", "unweighted"])
def test_swapping_the_handles_and_the_cells(weighted):
    a, b = (scene(), second_scene()) if weighted else (dict(scene(), w=None), dict(second_scene(), w=None))
    cells, t = two_handle_cells(), thresholds(12)
    A = shear_pair_oracle.shear_pair_cells(a, b, cells, t)[4]
    ctx = engine.get_context(0)
    h_a, h_b = upload(ctx, a), upload(ctx, b)
    try:
        ab = _lib.shear_pair_count(ctx, h_a, h_b, cells, t)
        ba = _lib.shear_pair_count(ctx, h_b, h_a, swapped(cells), t)
    finally:
        h_a.free(), h_b.free()
    assert np.count_nonzero(A) > 50
    for name, one, two in zip("PMC", ab[:3], ba[:3]):
        worst = float(np.max(np.abs(one - two) / np.where(A > 0, A, 1.0)))
        print(f"swap {name}: worst |ab - ba| / A = {worst:.3e}")
        assert np.all(np.abs(one - two) <= 1e-10 * A), (name, worst)
    if weighted:
        np.testing.assert_allclose(ab[3], ba[3], rtol=RTOL_W, atol=0)
    else:
        assert np.array_equal(ab[3], ba[3])


# --------------------------------------------------------------------------- 5. window edges
@pytest.mark.parametrize("anchors", ["streamed", "in lanes"])
@pytest.mark.parametrize("sort_axis", [0, 1, 2])
def test_window_edges_between_two_bins(sort_axis, anchors):
    """The window-edge scene of the auto count with anchors and partners in the two redshift bins of one patch: partners
    displaced along the sort axis only, by the chord of the inner / outer edge times (1 -/+ 1e-9), around the anchors that come
    first and last in their segment; the anchors are bin 0 (streamed) or bin 1 (in the lanes) of cell (0, 0, 0, 1)."""
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
    cat = dict(x=xyz[0].copy(), y=xyz[1].copy(), z=xyz[2].copy(), w=None, g1=rng.normal(0, 0.3, n), g2=rng.normal(0, 0.3, n), nb=2,
               off=np.array([0, parts[0].shape[1], n], dtype=np.int64))
    cells = np.array([(0, 0, 0, 1, 0)], dtype=np.int32)
    exp = shear_pair_oracle.shear_pair_cells(cat, cat, cells, t)
    only = np.r_[0:40 + len(placed)] if anchors == "streamed" else np.r_[0:len(placed), n - 40:n]
    few = dict(cat, **{c: cat[c][only] for c in ("x", "y", "z", "g1", "g2")},
               off=np.array([0, 40 if anchors == "streamed" else len(placed), 40 + len(placed)], dtype=np.int64))
    W_placed = shear_pair_oracle.shear_pair_cells(few, few, cells, t)[3]
    assert W_placed[0, 0] > 0 and W_placed[0, 1] > 0  # edge pairs are counted, in both fine bins
    P, M, C, W, _ = count(cat, cat, cells, t, sort_axis, sort_axis)
    assert np.array_equal(W, exp[3])
    check_against_oracle(f"edges axis={sort_axis} anchors {anchors}", (P, M, C, W), exp)


# --------------------------------------------------------------------------- 6. pole guard
@pytest.mark.parametrize("pole_bin", [0, 1], ids=["pole streamed", "pole in lanes"])
def test_an_object_on_the_pole_adds_to_w_only(pole_bin):
    """One object exactly at dec = +90 degrees in bin 0 (streamed) or bin 1 (in the lanes) of one patch, partners 1 to 5
    arcmin away in the other bin: its pairs add to W and to nothing else."""
    rng = np.random.default_rng(41)
    n = 7
    ra, dec = rng.uniform(0.0, 2.0 * np.pi, n), 0.5 * np.pi - rng.uniform(1.0, 5.0, n) * ARCMIN
    x, y, z = radec_to_xyz(ra, dec)
    at = 0 if pole_bin == 0 else 4  # first object of its bin
    x, y, z = (np.insert(c, at, v) for c, v in ((x, 0.0), (y, 0.0), (z, 1.0)))
    w = np.array([0.5, 0.75, 1.0, 1.25, 1.5, 1.75, 2.0, 0.25])  # dyadic: the sums of products are exact
    cat = dict(x=x, y=y, z=z, w=w, g1=rng.normal(0, 0.3, n + 1), g2=rng.normal(0, 0.3, n + 1), nb=2, off=np.array([0, 4, 8], dtype=np.int64))
    keep = np.arange(n + 1) != at
    without = dict(cat, **{c: cat[c][keep] for c in ("x", "y", "z", "w", "g1", "g2")},
                   off=np.array([0, 3, 7] if pole_bin == 0 else [0, 4, 7], dtype=np.int64))
    t = chord2([[0.5, 12.0]])
    cells = np.array([(0, 0, 0, 1, 0)], dtype=np.int32)
    exp, exp_without = shear_pair_oracle.shear_pair_cells(cat, cat, cells, t), shear_pair_oracle.shear_pair_cells(without, without, cells, t)
    for a, b in zip(exp[:3], exp_without[:3]):
        assert np.array_equal(a, b)  # (the oracle: nothing from the pole object)
    P, M, C, W, _ = count(cat, cat, cells, t)
    assert np.all(np.isfinite(P)) and np.all(np.isfinite(M)) and np.all(np.isfinite(C))
    check_against_oracle(f"pole in bin {pole_bin}", (P, M, C, W), exp)
    W_without = count(without, without, cells, t)[3]
    in_other = w[4:].sum() if pole_bin == 0 else w[:4].sum()  # every partner is within 5' of the pole
    assert W[0, 0] == W_without[0, 0] + w[at] * in_other and W_without[0, 0] > 0


# --------------------------------------------------------------------------- 7. reproducibility
def test_two_calls_return_the_same_bits():
    ctx = engine.get_context(0)
    a, b = upload(ctx, scene()), upload(ctx, second_scene(), 0)
    try:
        calls = [(a, a, one_handle_cells(), thresholds(50)), (a, b, two_handle_cells(), thresholds(50))]
        for h_a, h_b, cells, t in calls:
            one = _lib.shear_pair_count(ctx, h_a, h_b, cells, t)[:4]
            two = _lib.shear_pair_count(ctx, h_a, h_b, cells, t)[:4]
            assert np.count_nonzero(one[0]) > 100
            for x, y in zip(one, two):
                assert np.array_equal(x, y)
    finally:
        a.free(), b.free()


# --------------------------------------------------------------------------- 8. end to end
def test_correlate_shear_tomographic_end_to_end(monkeypatch):
    """The scenario of the CPU driver test (3 patches x 3 bins, one and two catalogues) through the real library: the same
    assertions against the oracle's fine bins, and the result of the driver on the oracle stand-in."""
    import yet_another_wizz_amd as yaw
    from test_shear_tomo_host import check_tomo_scenario, tomo_scenario

    device = check_tomo_scenario()
    monkeypatch.setattr(engine, "count_shear_pair_fine", shear_pair_oracle.count_shear_pair_fine)
    config, sources = tomo_scenario()
    stand_in = yaw.correlate_shear_tomographic(config, sources)
    for rows_d, rows_s in zip(device, stand_in):
        for triple_d, triple_s in zip(rows_d, rows_s):
            for c, (cf_d, cf_s) in enumerate(zip(triple_d, triple_s)):
                assert np.array_equal(cf_d.dd.number_counts.counts == 0, cf_s.dd.number_counts.counts == 0)
                np.testing.assert_allclose(cf_d.dd.number_counts.counts, cf_s.dd.number_counts.counts, rtol=RTOL_W, atol=0)
                tol = dict(rtol=1e-10) if c == 0 else dict(rtol=1e-8, atol=1e-12)
                np.testing.assert_allclose(cf_d.sample().data, cf_s.sample().data, **tol)
                np.testing.assert_allclose(cf_d.sample().samples, cf_s.sample().samples, **tol)


# --------------------------------------------------------------------------- 9. refusals
def test_refusals():
    ctx = engine.get_context(0)
    other = _lib.Context(0)
    cat = weighted_scene(False)
    a = upload(ctx, cat)
    one_patch = _lib.ShearSources(ctx, cat["x"], cat["y"], cat["z"], None, cat["g1"], cat["g2"], 1,
                                  np.array([0, len(cat["x"])], dtype=np.int64))  # one patch, one bin
    foreign = upload(other, cat)
    t = thresholds(1)

    def refused(match, h_a, h_b, cell, t=t, context=ctx):
        with pytest.raises(_lib.YawhipError, match=match):
            _lib.shear_pair_count(context, h_a, h_b, np.array([(0, 0, 0, 0, 0), cell], dtype=np.int32), t)

    try:
        refused("patch id outside", a, a, (3, 0, 0, 1, 0))          # p outside a's patches
        refused("patch id outside", a, a, (-1, 0, 0, 1, 0))
        refused("patch id outside", a, one_patch, (0, 1, 0, 0, 0))  # q outside b's
        refused("patch id outside", one_patch, a, (1, 0, 0, 0, 0))
        refused("redshift bin outside", a, a, (0, 1, 2, 1, 0))      # ka outside a's bins
        refused("redshift bin outside", a, a, (0, 1, 0, -1, 0))
        refused("redshift bin outside", a, one_patch, (0, 0, 0, 1, 0))  # kb outside b's
        refused("thresholds row outside", a, a, (0, 1, 0, 1, 2))    # row >= n_rows
        refused("thresholds row outside", a, a, (0, 1, 0, 1, -1))
        refused("p <= q", a, a, (2, 1, 1, 1, 0))                    # inside one bin of one handle
        refused("not ascending", a, a, (0, 1, 0, 1, 0), t=t[:, ::-1].copy())
        refused("max edges 256", a, a, (0, 1, 0, 1, 0), t=thresholds(256))
        refused("another context", a, foreign, (0, 1, 0, 1, 0))
        refused("another context", foreign, a, (0, 1, 0, 1, 0))
        refused("another context", a, a, (0, 1, 0, 1, 0), context=other)
        with pytest.raises(_lib.YawhipError, match="another context"):
            _lib.shear_pair_count(ctx, a, foreign, np.empty((0, 5), dtype=np.int32), t)  # checked before the early return
        # p > q is fine across two bins and between two handles; no cells at all: nothing to do
        P, M, C, W, stats = _lib.shear_pair_count(ctx, a, a, np.empty((0, 5), dtype=np.int32), t)
        assert P.shape == W.shape == (0, 1) and stats.n_workgroups == 0
        P, M, C, W, _ = _lib.shear_pair_count(ctx, a, a, np.array([(2, 1, 0, 1, 0), (1, 2, 1, 1, 1)], dtype=np.int32), t)
        assert np.all(W.sum(axis=1) > 0)  # the handle is still good
    finally:
        a.free(), one_patch.free(), foreign.free()
        other.close()
