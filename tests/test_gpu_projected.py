"""GPU: the projected pair count (``yawhip_proj_count``) and ``autocorrelate_projected`` on the device, against the numpy brute
force of tests/proj_oracle.py, on the scenes of tests/proj_scenes.py (whose membership tests/test_projected_host.py proves
exact with mpmath).

Membership is tested EXACTLY: with unit weights ``W`` is the integer number of pairs per cell and fine bin and must equal the
oracle's with ``np.array_equal``. Weighted sums are held to ``|ours - oracle| <= K eps A`` per cell and fine bin, ``A`` the sum
of ``|w_a w_b|`` over its member pairs."""
import functools

import numpy as np
import pytest

import proj_oracle as oracle
import proj_scenes as scenes
from yet_another_wizz_amd import _lib, engine
from yet_another_wizz_amd.catalog import radec_to_xyz

pytestmark = pytest.mark.gpu
DEG = np.pi / 180.0
EPS = 2.0**-53
# The oracle's own worst |W - exact| / (eps A) against the 50-digit sums of tests/test_projected_host.py
# (test_the_oracles_membership_is_exact_on_the_device_scene prints it and asserts that it still holds); K is four times
# that, rounded up to a power of two, as DESIGN.md sections 15 and 19 set theirs. The device's own ratio is in section 20.
K_ORACLE_RATIO = 5.411  # measured: 5.4107
K = 32.0
COLUMNS = ("x", "y", "z", "w", "d", "c")


def upload(ctx, h, sort_axis=2):
    n_patches = (len(h["off"]) - 1) // h["nb"]
    return _lib.ProjHandle(ctx, h["x"], h["y"], h["z"], h["w"], h["d"], h["c"], n_patches, h["nb"], h["off"], sort_axis=sort_axis)


def count(a, b, cells, r2, pmax, axis_a=2, axis_b=None):
    """``yawhip_proj_count`` of the oracle's handles ``a``, ``b`` (``b is a``: one handle passed twice) -> (W, CountStats)."""
    ctx = engine.get_context(0)
    first = upload(ctx, a, axis_a)
    second = first if b is a else upload(ctx, b, axis_a if axis_b is None else axis_b)
    try:
        W, stats = _lib.proj_count(ctx, first, second, cells, r2, pmax)
    finally:
        first.free(), second.free()
    assert stats.n_workgroups == len(cells) and 0 < stats.evaluated_pairs <= stats.candidate_pairs
    return W, stats


def one_segment(xyz, d, c, w=None):
    """A handle of one patch and one bin from coordinates [3, n]."""
    n = xyz.shape[1]
    return dict(zip("xyz", (col.copy() for col in xyz)), w=w, d=np.broadcast_to(np.asarray(d, dtype=np.float64), (n,)).copy(),
                c=np.broadcast_to(np.asarray(c, dtype=np.float64), (n,)).copy(), nb=1, off=np.array([0, n], dtype=np.int64))


def box_xyz(rng, n, lo=40.0, hi=40.5):
    return np.array(radec_to_xyz(rng.uniform(lo, hi, n) * DEG, rng.uniform(30.0, 30.0 + hi - lo, n) * DEG))


DIAGONAL, ACROSS = np.array([[0, 0, 0, 1]], dtype=np.int32), np.array([[0, 0, 0, 0]], dtype=np.int32)
PER_SEGMENT = {4: 24, 1: 96}


@functools.lru_cache(maxsize=None)
def scene(nb, weighted):
    a, b = (scenes.handle(seed, nb, PER_SEGMENT[nb], weighted) for seed in (scenes.SEED_A, scenes.SEED_B))
    return a, b


@functools.lru_cache(maxsize=None)
def expected(nb, nf, weighted, two):
    """The oracle's (W, A, N) of the scene, one handle or two: computed once per case, shared, never modified."""
    a, b = scene(nb, weighted)
    cells = scenes.cells_two_handles(nb) if two else scenes.cells_one_handle(nb)
    out = oracle.proj_cells(a, b if two else a, cells, scenes.radius_edges(nf, nb), scenes.PMAX)
    for arr in out:
        arr.setflags(write=False)
    return out


# --------------------------------------------------------------------------- 1. exact membership
def test_the_scene_stays_off_the_edges_and_off_the_cut():
    """The condition under which tests/test_projected_host.py proves the oracle's membership exact, asserted from the scene
    (in float64; the CPU test asserts it at 50 digits for four bins and twelve fine bins)."""
    for nb in (1, 4):
        a, b = scene(nb, False)
        for nf in (1, 12, 50):
            r2 = scenes.radius_edges(nf, nb)
            assert min(oracle.nearest_margin(a, a, scenes.cells_one_handle(nb), r2, scenes.PMAX)) > 1e-9
            assert min(oracle.nearest_margin(a, b, scenes.cells_two_handles(nb), r2, scenes.PMAX)) > 1e-9


@pytest.mark.parametrize("sort_axis", [0, 1, 2])
@pytest.mark.parametrize("nf", [1, 12, 50])
@pytest.mark.parametrize("nb", [1, 4])
def test_membership_is_the_oracles(nb, nf, sort_axis):
    a, b = scene(nb, False)
    r2 = scenes.radius_edges(nf, nb)
    for two in (False, True):
        cells = scenes.cells_two_handles(nb) if two else scenes.cells_one_handle(nb)
        exp_w, _, exp_n = expected(nb, nf, False, two)
        diagonal = cells[:, 3] != 0
        assert two or (exp_n[diagonal].sum() > 0 and exp_n[~diagonal].sum() > 0)  # diagonal and off-diagonal cells hold pairs
        assert np.any(exp_n.sum(axis=1) == 0) == (nb > 1)  # the empty segment
        W, stats = count(a, b if two else a, cells, r2, scenes.PMAX, sort_axis)
        assert np.array_equal(W, exp_n) and np.array_equal(exp_w, exp_n)
        sizes_a, sizes_b = np.diff(a["off"]), np.diff((b if two else a)["off"])
        candidates = sum(n * (n - 1) // 2 if diag else n * m for n, m, diag in zip(sizes_a[cells[:, 0]], sizes_b[cells[:, 1]], diagonal))
        assert stats.candidate_pairs == candidates


def long_segment(rng, n, sort_axis, near=900.0):
    """``n`` objects in one segment whose ``d`` alternates by a factor 7 in the order of the sort key, ``c`` 0 .. 120."""
    xyz = box_xyz(rng, n)
    d = np.empty(n)
    d[np.argsort(xyz[sort_axis], kind="stable")] = np.where(np.arange(n) % 2 == 0, near * 7.0, near)
    return one_segment(xyz, d, rng.uniform(0.0, 120.0, n))


@pytest.mark.parametrize("sort_axis", [0, 2])
def test_a_diagonal_cell_over_one_long_segment(sort_axis):
    """600 objects in ONE segment against itself: three stages, a padded last lane tile, and the first stage of every tile
    holding indices <= the lane's. The count is the oracle's, and half the count of the segment against a bit-identical copy
    uploaded as a second handle -- that one sees every pair twice and every object with itself at ``R2 = 0``, which no bin
    holds as long as the first edge is > 0."""
    h = long_segment(np.random.default_rng(5 + sort_axis), 600, sort_axis)
    r2 = np.array([np.geomspace(0.1, 4.0, 13)]) ** 2
    assert r2[0, 0] > 0.0
    exp = oracle.proj_cells(h, h, DIAGONAL, r2, scenes.PMAX)[2]
    near_only = oracle.proj_cells(dict(h, d=np.where(h["d"] < 1000.0, h["d"], 1e9)), h, DIAGONAL, r2, scenes.PMAX, same=True)[2]
    assert near_only.sum() > 0 and (exp - near_only).sum() > 0 and np.all(exp[0] > 0)  # every kind of pair holds some
    W, stats = count(h, h, DIAGONAL, r2, scenes.PMAX, sort_axis)
    assert np.array_equal(W, exp) and stats.candidate_pairs == 600 * 599 // 2
    copy = {key: (value.copy() if isinstance(value, np.ndarray) else value) for key, value in h.items()}
    both, stats = count(h, copy, ACROSS, r2, scenes.PMAX, sort_axis)
    assert np.array_equal(both, 2.0 * W) and stats.candidate_pairs == 600 * 600


@pytest.mark.parametrize("sort_axis", [0, 2])
def test_a_long_segment_streamed_against_lanes_of_another(sort_axis):
    """600 streamed against 300 in the lanes, off the diagonal: three stages, the last ragged; a full lane tile and a padded
    one. Two segments of ONE handle, and of two."""
    rng = np.random.default_rng(9 + sort_axis)
    a, b = long_segment(rng, 600, sort_axis), long_segment(rng, 300, sort_axis)
    r2 = np.array([np.geomspace(0.1, 4.0, 13)]) ** 2
    exp = oracle.proj_cells(a, b, ACROSS, r2, scenes.PMAX)[2]
    assert np.all(exp[0] > 0)
    W, stats = count(a, b, ACROSS, r2, scenes.PMAX, sort_axis)
    assert np.array_equal(W, exp) and stats.candidate_pairs == 600 * 300
    one = dict({c: np.concatenate([a[c], b[c]]) for c in "xyzdc"}, w=None, nb=1, off=np.array([0, 600, 900], dtype=np.int64))
    W, stats = count(one, one, np.array([[0, 1, 0, 0]], dtype=np.int32), r2, scenes.PMAX, sort_axis)
    assert np.array_equal(W, exp)


@pytest.mark.parametrize("sort_axis", [0, 1, 2])
def test_partners_next_to_an_edge_on_it_and_on_the_cut(sort_axis):
    """Partners displaced from an object along the sort axis only, by the chord of the angle at which ``R^2`` is the inner /
    outer edge times ``(1 -/+ 1e-9)`` or the edge itself, around the objects that come first and last in their segment.
    Every ``d`` is 1024, so ``D`` and ``DD`` are exact and ``R2 = DD th2`` is an exact scaling: the two edges are then SET
    to the ``R2`` of one placed pair each, which must fall into the bin below its edge. Every ``c`` is a multiple of 1/4: a
    partner displaced upwards lies EXACTLY ``pmax = 40`` behind its object (it counts), one displaced downwards at the same
    ``c`` (it counts with ``pmax = 0``)."""
    rng = np.random.default_rng(17 + sort_axis)
    base_xyz = box_xyz(rng, 40)
    base_c = rng.integers(0, 400, 40) * 0.25
    r2 = np.array([[0.2, 0.9, 2.5]]) ** 2
    first, last = int(np.argmin(base_xyz[sort_axis])), int(np.argmax(base_xyz[sort_axis]))
    placed, placed_c, owner = [], [], []
    for at in (first, last):
        for edge in (r2[0, 0], r2[0, 2]):
            for factor in (1.0 - 1e-9, 1.0, 1.0 + 1e-9):
                for sign in (-1.0, 1.0):
                    p = base_xyz[:, at].copy()
                    p[sort_axis] += sign * 2.0 * np.sin(0.5 * np.sqrt(edge * factor) / 1024.0)
                    placed.append(p), placed_c.append(base_c[at] + (40.0 if sign > 0 else 0.0)), owner.append((at, edge, factor))
    filler = box_xyz(rng, 300)
    a = one_segment(base_xyz, 1024.0, base_c)
    b = one_segment(np.concatenate([np.array(placed).T, filler], axis=1), 1024.0, np.concatenate([placed_c, rng.integers(0, 400, 300) * 0.25]))
    only_placed = one_segment(np.array(placed).T, 1024.0, np.array(placed_c))

    def pair_r2(i, j):
        return float(oracle.pair_terms(a, b, np.array([i]), np.array([j]))[0][0])

    # the pair placed at factor 1.0 below the first object sets the inner edge, the one above the last object the outer edge
    on_inner = next(i for i, (at, edge, factor) in enumerate(owner) if at == first and edge == r2[0, 0] and factor == 1.0)
    on_outer = next(i for i, (at, edge, factor) in enumerate(owner) if at == last and edge == r2[0, 2] and factor == 1.0) + 1
    r2[0, 0], r2[0, 2] = pair_r2(first, on_inner), pair_r2(last, on_outer)
    assert abs(r2[0, 0] / 0.04 - 1.0) < 1e-10 and abs(r2[0, 2] / 6.25 - 1.0) < 1e-10
    inf = float("inf")
    W_placed = oracle.proj_cells(a, only_placed, ACROSS, r2, inf)[2]
    assert W_placed[0, 0] > 0 and W_placed[0, 1] > 0  # edge pairs on both sides of being counted
    R2 = oracle.pair_terms(a, only_placed, np.arange(40)[:, None], np.arange(len(placed))[None, :])[0]
    for column, which, sign in ((0, 0, 1), (2, 1, -1)):  # one ulp less of the inner edge takes the pairs ON it in, of the outer edge out
        n_on = np.count_nonzero(R2 == r2[0, column])
        moved = r2.copy()
        moved[0, column] = np.nextafter(moved[0, column], 0.0)
        assert n_on >= 1 and oracle.proj_cells(a, only_placed, ACROSS, moved, inf)[2][0, which] == W_placed[0, which] + sign * n_on
    # the cut: pairs exactly at pmax count, one ulp less of pmax drops them; pmax = 0 keeps the pairs at equal c
    at_cut = oracle.proj_cells(a, only_placed, ACROSS, r2, 40.0)[2]
    assert at_cut.sum() > oracle.proj_cells(a, only_placed, ACROSS, r2, np.nextafter(40.0, 0.0))[2].sum() > 0
    assert 0 < oracle.proj_cells(a, only_placed, ACROSS, r2, 0.0)[2].sum() < at_cut.sum() <= W_placed.sum()
    for pmax in (40.0, 0.0, inf):
        exp = oracle.proj_cells(a, b, ACROSS, r2, pmax)[2]
        W, _ = count(a, b, ACROSS, r2, pmax, sort_axis)
        assert np.array_equal(W, exp), pmax


@pytest.mark.parametrize("sort_axis", [0, 1, 2])
def test_the_window_follows_the_nearest_object(sort_axis):
    """One object eight times nearer than the other 299 of its segment, with partners as near at the far end of ITS reach
    along the sort axis, eight window widths of the others away."""
    rng = np.random.default_rng(29 + sort_axis)
    xyz = box_xyz(rng, 300, 40.0, 42.0)
    d = np.full(300, 1600.0)
    near = 123
    d[near] = 200.0
    r2 = np.array([np.geomspace(0.3, 2.0, 6)]) ** 2  # 2 Mpc: 4.3 arcmin at 1600 Mpc, 34 arcmin at 200 Mpc
    placed = []
    for factor in (0.7, 1.0 - 1e-6, 1.0 + 1e-6):
        for sign in (-1.0, 1.0):
            p = xyz[:, near].copy()
            p[sort_axis] += sign * 2.0 * np.sin(0.5 * np.sqrt(r2[0, -1] * factor) / 200.0)
            placed.append(p)
    a = one_segment(xyz, d, 50.0)
    b = one_segment(np.concatenate([np.array(placed).T, box_xyz(rng, 400, 40.0, 42.0)], axis=1), np.concatenate([np.full(6, 200.0), np.full(400, 1600.0)]), 50.0)
    alone = one_segment(xyz[:, near:near + 1], 200.0, 50.0)
    only_placed = one_segment(np.array(placed).T, 200.0, 50.0)
    assert oracle.proj_cells(alone, only_placed, ACROSS, r2, 1.0)[2][0, -1] == 4.0  # four of the six inside the last bin
    exp = oracle.proj_cells(a, b, ACROSS, r2, 1.0)[2]
    for first, second in ((a, b), (b, a)):  # the nearest object on either side
        W, stats = count(first, second, ACROSS, r2, 1.0, sort_axis)
        assert np.array_equal(W, exp)


@pytest.mark.parametrize("sort_axis", [0, 2])
def test_tied_sort_keys_across_a_tile_boundary(sort_axis):
    """150 of 600 objects share ONE sort key, from rank 180 to rank 329 of their segment: the tie straddles the boundary of the
    first lane tile and of the first stage, and whichever order the device's sort leaves them in, a diagonal cell holds every
    unordered pair once."""
    rng = np.random.default_rng(41 + sort_axis)
    h = long_segment(rng, 600, sort_axis)
    order = np.argsort(h["xyz"[sort_axis]], kind="stable")
    h["xyz"[sort_axis]][order[180:330]] = h["xyz"[sort_axis]][order[255]]
    other = long_segment(rng, 300, sort_axis)
    other["xyz"[sort_axis]][:100] = h["xyz"[sort_axis]][order[255]]
    r2 = np.array([np.geomspace(0.1, 4.0, 7)]) ** 2
    exp = oracle.proj_cells(h, h, DIAGONAL, r2, scenes.PMAX)[2]
    tied = dict(h, **{c: h[c][order[180:330]] for c in "xyzdc"}, off=np.array([0, 150], dtype=np.int64))
    assert oracle.proj_cells(tied, tied, DIAGONAL, r2, scenes.PMAX)[2].sum() > 100  # pairs among the tied objects themselves
    W, _ = count(h, h, DIAGONAL, r2, scenes.PMAX, sort_axis)
    assert np.array_equal(W, exp)
    W, _ = count(h, other, ACROSS, r2, scenes.PMAX, sort_axis)
    assert np.array_equal(W, oracle.proj_cells(h, other, ACROSS, r2, scenes.PMAX)[2])


def test_different_sort_axes_stream_the_whole_segment():
    a, b = scene(4, False)
    cells, r2 = scenes.cells_two_handles(4), scenes.radius_edges(12, 4)
    windowed, st_windowed = count(a, b, cells, r2, scenes.PMAX, 2, 2)
    whole, st_whole = count(a, b, cells, r2, scenes.PMAX, 2, 0)
    assert st_whole.evaluated_pairs == st_whole.candidate_pairs >= st_windowed.evaluated_pairs
    assert np.array_equal(whole, windowed) and np.array_equal(whole, expected(4, 12, False, True)[2])


# --------------------------------------------------------------------------- 2. weighted sums, reproducibility
@pytest.mark.parametrize("sort_axis", [0, 2])
@pytest.mark.parametrize("nb, nf", [(4, 12), (1, 50)])
def test_weighted_sums_match_the_oracle(nb, nf, sort_axis):
    a, b = scene(nb, True)
    r2 = scenes.radius_edges(nf, nb)
    worst = 0.0
    for two in (False, True):
        cells = scenes.cells_two_handles(nb) if two else scenes.cells_one_handle(nb)
        exp_w, exp_a, exp_n = expected(nb, nf, True, two)
        W, _ = count(a, b if two else a, cells, r2, scenes.PMAX, sort_axis)
        assert np.array_equal(W == 0.0, exp_n == 0.0)
        worst = max(worst, float(np.max(np.abs(W - exp_w)[exp_a > 0] / (EPS * exp_a[exp_a > 0]))))
        print(f"nb={nb} nf={nf} axis={sort_axis} {'two handles' if two else 'one handle'}: worst |ours - oracle| / (eps A) = {worst:.3f}")
        assert np.all(np.abs(W - exp_w) <= K * EPS * exp_a)


def test_two_calls_return_the_same_bits():
    a, _ = scene(1, True)
    ctx = engine.get_context(0)
    handle = upload(ctx, a)
    try:
        one = _lib.proj_count(ctx, handle, handle, scenes.cells_one_handle(1), scenes.radius_edges(50, 1), scenes.PMAX)[0]
        two = _lib.proj_count(ctx, handle, handle, scenes.cells_one_handle(1), scenes.radius_edges(50, 1), scenes.PMAX)[0]
    finally:
        handle.free()
    assert np.count_nonzero(one) > 100 and np.array_equal(one, two)


# --------------------------------------------------------------------------- 3. refusals
def test_uploads_refuse_columns_out_of_range():
    ctx = engine.get_context(0)
    a, _ = scene(4, False)
    for column, values in (("d", (0.0, -1.0, np.nan, np.inf)), ("c", (np.nan, np.inf, -np.inf))):
        for value in values:
            bad = dict(a, **{column: a[column].copy()})
            bad[column][17] = value
            with pytest.raises(_lib.YawhipError, match=f"column {column}"):
                upload(ctx, bad)
    upload(ctx, dict(a, c=-a["c"])).free()  # a negative line-of-sight coordinate is fine


def test_mismatched_handles_reaches_and_arguments_are_refused():
    ctx = engine.get_context(0)
    other = _lib.Context(0)
    a, _ = scene(4, False)
    n_patches = 2 * len(scenes.SITES)
    r2 = scenes.radius_edges(1, 4)
    cells = scenes.cells_one_handle(4)
    jobs = np.array([[0, 0]], dtype=np.int32)
    handle, foreign = upload(ctx, a), upload(other, a)
    lenses = _lib.DsigmaLenses(ctx, a["x"], a["y"], a["z"], None, a["d"], a["c"], n_patches, 4, a["off"])
    radial = _lib.DsigmaLenses(ctx, a["x"], a["y"], a["z"], None, a["d"], a["c"], n_patches, 4, a["off"], m=a["d"] ** 2)
    binned = _lib.ShearSources(ctx, a["x"], a["y"], a["z"], None, a["d"], a["c"], n_patches, a["off"], n_bins=4)
    unbinned = scenes.handle(scenes.SEED_B, 1, 8, False)
    sources = _lib.ShearSources(ctx, unbinned["x"], unbinned["y"], unbinned["z"], None, unbinned["d"], unbinned["c"], n_patches, unbinned["off"], u=unbinned["c"])
    catalog = _lib.DeviceCatalog(ctx, a["x"], a["y"], a["z"], None, n_patches, 4, a["off"])
    try:
        # the new count takes projected handles only, on either side
        for first, second in ((lenses, handle), (handle, radial), (binned, handle), (handle, sources)):
            with pytest.raises(_lib.YawhipError, match="not one of yawhip_proj_upload"):
                _lib.proj_count(ctx, first, second, cells[len(cells) // 2:], r2, 40.0)
        with pytest.raises(_lib.YawhipError, match="another context"):
            _lib.proj_count(ctx, handle, foreign, cells[len(cells) // 2:], r2, 40.0)
        # the five other counts refuse a projected handle
        with pytest.raises(_lib.YawhipError, match="not a shear catalogue"):
            _lib.shear_count(ctx, catalog, handle, jobs, r2)
        with pytest.raises(_lib.YawhipError, match="not a shear catalogue"):
            _lib.shear_auto_count(ctx, handle, jobs, r2)
        with pytest.raises(_lib.YawhipError, match="not a shear catalogue"):
            _lib.shear_pair_count(ctx, handle, binned, np.array([[0, 0, 0, 0, 0]], dtype=np.int32), r2)
        with pytest.raises(_lib.YawhipError, match="lenses are not a handle of yawhip_dsigma_upload_lenses"):
            _lib.dsigma_count(ctx, handle, sources, jobs, r2)
        with pytest.raises(_lib.YawhipError, match="lenses are not a handle of yawhip_dsigma_upload_lenses"):
            _lib.dsigma_count_radial(ctx, handle, sources, jobs, r2)
        with pytest.raises(_lib.YawhipError, match="sources are not a handle of yawhip_dsigma_upload_sources"):
            _lib.dsigma_count(ctx, lenses, handle, jobs, r2)
        # the cap: the nearest object of the scene is 800 away, 0.01 is a chord of 0.1: a radius of 100 is too much ...
        with pytest.raises(_lib.YawhipError, match="an object is too close for the largest radius"):
            _lib.proj_count(ctx, handle, handle, cells, np.array([[0.0, 100.0**2]] * 4), 40.0)
        # ... and exactly at the cap, per row: the first radius beyond smax = 0.01 of row 2 alone
        per_bin = [np.concatenate([a["d"][a["off"][p * 4 + k]:a["off"][p * 4 + k + 1]] for p in range(n_patches)]).min() for k in range(4)]
        fits = np.array([[0.0, 0.0099 * per_bin[k] ** 2] for k in range(4)])
        _lib.proj_count(ctx, handle, handle, cells, fits, 40.0)
        beyond = fits.copy()
        beyond[2, 1] = 0.0101 * per_bin[2] ** 2
        with pytest.raises(_lib.YawhipError, match="an object is too close for the largest radius"):
            _lib.proj_count(ctx, handle, handle, cells, beyond, 40.0)
        _lib.proj_count(ctx, handle, handle, cells[cells[:, 2] != 2], beyond, 40.0)  # no cell of the row: no reach
        with pytest.raises(_lib.YawhipError, match="not finite|not ascending"):
            _lib.proj_count(ctx, handle, handle, cells, np.array([[0.0, np.inf]] * 4), 40.0)
        with pytest.raises(_lib.YawhipError, match="not ascending"):
            _lib.proj_count(ctx, handle, handle, cells, scenes.radius_edges(3, 4)[:, ::-1].copy(), 40.0)
        with pytest.raises(_lib.YawhipError, match="bad sizes"):
            _lib.proj_count(ctx, handle, handle, cells, scenes.radius_edges(256, 4), 40.0)  # 257 edges
        for pmax in (-1.0, -0.0 - 1e-300, float("nan")):
            with pytest.raises(_lib.YawhipError, match="pmax"):
                _lib.proj_count(ctx, handle, handle, cells, r2, pmax)
        for bad_cell, what in (((32, 0, 0, 0), "segment"), ((0, -1, 0, 0), "segment"), ((0, 1, 4, 0), "row"), ((0, 0, 0, 0), "diagonal"),
                               ((0, 1, 0, 1), "diagonal")):
            with pytest.raises(_lib.YawhipError, match=what):
                _lib.proj_count(ctx, handle, handle, np.array([bad_cell], dtype=np.int32), r2, 40.0)
        W, _ = _lib.proj_count(ctx, handle, handle, np.empty((0, 4), dtype=np.int32), r2, 40.0)  # nothing to do
        assert W.shape == (0, 1)
    finally:
        for h in (handle, foreign, lenses, radial, binned, sources, catalog):
            h.free()
        other.close()


# --------------------------------------------------------------------------- 4. agreement with the number counts
def one_distance_scene(seed=3):
    """Three patches side by side, one redshift bin, 150 data objects and 260 randoms around every centre, all at z = 0.5;
    two scales in Mpc and the same two as angles ``R / D0``. Returns the two configurations, the catalogues, their layouts
    with redshifts, and the smallest relative distance of any pair's ``R^2`` from an edge (the oracle's arithmetic)."""
    import yet_another_wizz_amd as yaw
    from yet_another_wizz_amd import cosmology, measurements
    from test_projected_host import NEIGHBOURS
    from test_shear_host import ring_around

    z0 = 0.5
    D0 = float(cosmology.Planck15.angular_diameter_distance(z0))
    rng = np.random.default_rng(seed)
    kw = dict(patch_centers=yaw.AngularCoordinates(np.array(NEIGHBOURS)), degrees=False)
    cats = []
    for n in (150, 260):
        ra, dec = (np.concatenate(c) for c in zip(*(ring_around(rng, ra_c, dec_c, n, 1e-5, 1.8e-3) for ra_c, dec_c in NEIGHBOURS)))
        cats.append(yaw.Catalog.from_arrays(ra, dec, redshifts=np.full(len(ra), z0), **kw))
    edges = np.array([0.1, 1.0])
    rmin, rmax = np.array([0.2, 0.7]), np.array([1.5, 2.5])  # Mpc
    radial = yaw.Configuration.create(rmin=rmin, rmax=rmax, unit="Mpc", edges=edges)
    angular = yaw.Configuration.create(rmin=rmin / D0, rmax=rmax / D0, unit="rad", edges=edges)
    layouts = [cat.build_trees(edges, closed=radial.binning.closed, with_redshifts=True) for cat in cats]
    r2 = measurements.threshold_table(measurements.radial_plans(radial))
    handles = [oracle.as_handle(layout, *engine.proj_columns(layout, radial.cosmology, "Mpc")) for layout in layouts]
    assert all(np.all(h["d"] == D0) for h in handles)
    margin = np.inf
    for first, second in ((handles[0], handles[0]), (handles[0], handles[1])):
        cells = np.array([(p, q, 0, first is second and p == q) for p in range(3) for q in range(3) if first is not second or p <= q])
        margin = min(margin, oracle.nearest_margin(first, second, cells, r2, float("inf"))[0])
    return radial, angular, cats, layouts, margin


def test_one_distance_and_no_cut_give_the_tensors_of_count_pairs():
    """Every object at ONE redshift, so ``d = D0`` for all, no line-of-sight cut that bites and unit weights: a pair's radius is
    ``D0 theta``, and ``count_projected_pairs`` returns the ``NormalisedCounts`` of ``PatchLinkage.count_pairs`` with the
    angular scales ``theta = R / D0`` -- DD with its halved diagonal, and DR. The pairs stay 1e-6 (relative) off every edge,
    asserted from the scene, so the two tables of edges, which differ by their rounding, name the same pairs. This ties the
    new kernel to the bit-exact band kernels without going through the oracle."""
    import yet_another_wizz_amd as yaw
    from yet_another_wizz_amd import measurements

    radial, angular, cats, layouts, margin = one_distance_scene()
    assert margin > 1e-6
    data, random = cats
    edges = radial.binning.edges
    links = yaw.PatchLinkage.from_catalogs(radial, data, random, max_angle=measurements.radial_max_angle(radial, *layouts))
    pi_max = 1e6  # no pair of the scene is cut: every |chi_a - chi_b| is 0
    projected = [links.count_projected_pairs(data, pi_max=pi_max), links.count_projected_pairs(data, random, pi_max=pi_max)]
    for cat in cats:
        cat.build_trees(edges, closed=angular.binning.closed)
    links = yaw.PatchLinkage.from_catalogs(angular, data, random)
    plain = [links.count_pairs(data), links.count_pairs(data, random)]
    for ours, theirs in zip(projected, plain):
        assert len(ours) == len(theirs) == 2
        for a, b in zip(ours, theirs):
            assert np.count_nonzero(a.counts.counts) >= 5 and a.counts.counts.sum() > 1000
            assert np.array_equal(a.counts.counts, b.counts.counts) and a.auto == b.auto
            assert a.sum_weights == b.sum_weights and a == b
    for cat in cats:
        cat.drop_layouts()


# --------------------------------------------------------------------------- 5. end to end
@pytest.mark.parametrize("count_rr", [True, False], ids=["LS", "DP"])
def test_the_driver_end_to_end(count_rr, monkeypatch):
    """The scenario of the CPU driver test through the real library, held per slot to 1e-12 of the oracle's sums recombined by
    hand, and to the driver on the stand-in."""
    from test_projected_host import check_driver

    on_device = check_driver("kpc", count_rr, rtol=1e-12)
    monkeypatch.setattr(engine, "count_projected_fine", oracle.count_projected_fine)
    stand_in = check_driver("kpc", count_rr, rtol=1e-12)
    for ours, theirs in zip(on_device, stand_in):
        for kind in ("dd", "dr") + (("rr",) if count_rr else ()):
            np.testing.assert_allclose(getattr(ours, kind).counts.counts, getattr(theirs, kind).counts.counts, rtol=1e-12, atol=0)
        np.testing.assert_allclose(ours.sample().data, theirs.sample().data, rtol=1e-9, atol=1e-11)


def test_the_linkage_reaches_past_neighbouring_patches():
    """The nearby sample of the CPU driver test through the real library: a reach of 4.7 degrees over patches of 3, DD, DR and
    RR equal to the patch-free brute force as integers, the four pi planes summing to them."""
    from test_projected_host import check_wide_linkage

    check_wide_linkage()
