"""GPU: the pi-binned projected pair count (``yawhip_proj_count_pi``) and ``autocorrelate_projected(pi_bins=...)`` on the device,
against the numpy brute force of tests/proj_pi_oracle.py, on the scenes of tests/proj_scenes.py (whose membership in radius
and in pi tests/test_projected_pi_host.py proves exact with mpmath), and against ``yawhip_proj_count`` on the same handles.

Membership is tested EXACTLY: with unit weights ``W`` is the integer number of pairs per pi bin, cell and fine bin and must
equal the oracle's with ``np.array_equal``. Weighted sums are held to ``|ours - oracle| <= K eps A`` per pi bin, cell and fine
bin, ``A`` the sum of ``|w_a w_b|`` over its member pairs."""
import ctypes
import functools

import numpy as np
import pytest

import proj_oracle
import proj_pi_oracle as oracle
import proj_scenes as scenes
from proj_pi_oracle import UNEVEN, UNIFORM_4, UNIFORM_30
from test_gpu_projected import ACROSS, DIAGONAL, box_xyz, long_segment, one_segment, scene, upload
from yet_another_wizz_amd import _lib, engine

pytestmark = pytest.mark.gpu
EPS = 2.0**-53
# The oracle's own worst |W - exact| / (eps A) per pi bin, cell and fine bin against the 50-digit sums of
# tests/test_projected_pi_host.py (test_the_oracles_membership_in_pi_is_exact_on_the_device_scene prints it and asserts that it
# still holds); K is four times that, rounded up to a power of two, as DESIGN.md sections 15, 19 and 20 set theirs. The
# device's own ratio is in section 22.
K_ORACLE_RATIO = 4.089  # measured: 4.0881 (over the three edge sets, one handle and two)
K = 32.0  # 4 x 4.089 = 16.4, rounded up to a power of two (the measurement gives section 20's figure; it is not borrowed)
ONE_BIN = np.array([0.0, scenes.PMAX])
EDGE_SETS = {"one": ONE_BIN, "uniform4": UNIFORM_4, "uniform30": UNIFORM_30, "uneven": UNEVEN}
CAP_AT_13_EDGES, CAP_AT_256_EDGES = 104, 4  # include/yawhip.h: the largest n_pi whose carve-up fits 64 KiB of LDS


def lds_bytes(n_edges, n_pi):
    """The carve-up of include/yawhip.h: two stages of 48-byte objects, thresholds, pi edges, four histograms."""
    return 2 * 256 * 48 + 8 * (((n_edges + 1) & ~1) + ((n_pi + 2) & ~1)) + 4 * n_pi * (n_edges - 1) * 8


def count_pi(a, b, cells, r2, pe, axis_a=2, axis_b=None, pmax=None):
    """``yawhip_proj_count_pi`` of the oracle's handles ``a``, ``b`` (``b is a``: one handle passed twice) -> (W, CountStats);
    with ``pmax`` also ``yawhip_proj_count`` on the same handles -> (W, CountStats, W1, CountStats1)."""
    ctx = engine.get_context(0)
    first = upload(ctx, a, axis_a)
    second = first if b is a else upload(ctx, b, axis_a if axis_b is None else axis_b)
    try:
        W, stats = _lib.proj_count_pi(ctx, first, second, cells, r2, pe)
        single = () if pmax is None else _lib.proj_count(ctx, first, second, cells, r2, pmax)
    finally:
        first.free(), second.free()
    assert W.shape == (len(pe) - 1, len(cells), np.shape(r2)[1] - 1)
    assert stats.n_workgroups == len(cells) and 0 < stats.evaluated_pairs <= stats.candidate_pairs
    return (W, stats, *single)


@functools.lru_cache(maxsize=None)
def expected(nb, nf, weighted, two, edges):
    """The oracle's (W, A, N) of the scene, one handle or two, for the edge set ``edges`` (a name of EDGE_SETS, or a number of
    uniform bins to 40): computed once per case, shared, never modified."""
    a, b = scene(nb, weighted)
    cells = scenes.cells_two_handles(nb) if two else scenes.cells_one_handle(nb)
    pe = EDGE_SETS[edges] if isinstance(edges, str) else np.linspace(0.0, scenes.PMAX, edges + 1)
    out = oracle.proj_pi_cells(a, b if two else a, cells, scenes.radius_edges(nf, nb), pe)
    for arr in out:
        arr.setflags(write=False)
    return out


def candidates_by_hand(a, b, cells):
    sizes_a, sizes_b = np.diff(a["off"]), np.diff(b["off"])
    return sum(n * (n - 1) // 2 if diag else n * m for n, m, diag in zip(sizes_a[cells[:, 0]], sizes_b[cells[:, 1]], cells[:, 3] != 0))


# --------------------------------------------------------------------------- 1. exact membership
def test_the_scene_stays_off_the_pi_edges():
    """The condition under which tests/test_projected_pi_host.py proves the oracle's membership in pi exact, asserted from the
    scene in float64 for every ``nb`` and every edge set used here (the radius edges: tests/test_gpu_projected.py)."""
    for nb in (1, 4):
        a, b = scene(nb, False)
        for pe in EDGE_SETS.values():
            for first, second, cells in ((a, a, scenes.cells_one_handle(nb)), (a, b, scenes.cells_two_handles(nb))):
                margin, least = oracle.nearest_pi_margin(first, second, cells, pe)
                assert margin > 1e-9 and least > 0.0


@pytest.mark.parametrize("sort_axis", [0, 1, 2])
@pytest.mark.parametrize("edges", list(EDGE_SETS))
@pytest.mark.parametrize("nf", [1, 12])
@pytest.mark.parametrize("nb", [1, 4])
def test_membership_is_the_oracles(nb, nf, edges, sort_axis):
    a, b = scene(nb, False)
    r2 = scenes.radius_edges(nf, nb)
    pe = EDGE_SETS[edges]
    for two in (False, True):
        cells = scenes.cells_two_handles(nb) if two else scenes.cells_one_handle(nb)
        exp_w, _, exp_n = expected(nb, nf, False, two, edges)
        assert np.all(exp_n.sum(axis=(1, 2)) > 0)  # every pi bin holds pairs
        assert np.any(exp_n.sum(axis=(0, 2)) == 0) == (nb > 1)  # the empty segment
        W, stats = count_pi(a, b if two else a, cells, r2, pe, sort_axis)
        assert np.array_equal(W, exp_n) and np.array_equal(exp_w, exp_n)
        assert stats.candidate_pairs == candidates_by_hand(a, b if two else a, cells)


# --------------------------------------------------------------------------- 2. the tie to yawhip_proj_count
@pytest.mark.parametrize("edges", ["uniform4", "uniform30", "uneven"])
@pytest.mark.parametrize("nb", [1, 4])
def test_the_planes_sum_to_the_single_cylinder_count_of_the_same_walk(nb, edges):
    """On the same handles, cells and radius edges: over unit weights the planes sum to ``yawhip_proj_count`` at
    ``pmax = pe[-1]`` as integers, and the two calls report the same candidate and evaluated pairs (one walk, one window)."""
    a, b = scene(nb, False)
    r2, pe = scenes.radius_edges(12, nb), EDGE_SETS[edges]
    for two in (False, True):
        cells = scenes.cells_two_handles(nb) if two else scenes.cells_one_handle(nb)
        W, stats, W1, stats1 = count_pi(a, b if two else a, cells, r2, pe, pmax=float(pe[-1]))
        assert W1.sum() > 1000 and np.array_equal(W.sum(axis=0), W1)
        assert stats.candidate_pairs == stats1.candidate_pairs and stats.evaluated_pairs == stats1.evaluated_pairs


def test_one_weighted_plane_is_the_single_cylinder_count():
    a, b = scene(4, True)
    r2 = scenes.radius_edges(12, 4)
    for two in (False, True):
        cells = scenes.cells_two_handles(4) if two else scenes.cells_one_handle(4)
        W, stats, W1, stats1 = count_pi(a, b if two else a, cells, r2, ONE_BIN, pmax=scenes.PMAX)
        A = expected(4, 12, True, two, "one")[1][0]
        assert np.all(np.abs(W[0] - W1) <= K * EPS * A) and (stats.candidate_pairs, stats.evaluated_pairs) == (stats1.candidate_pairs, stats1.evaluated_pairs)


# --------------------------------------------------------------------------- 3. long segments, ties, sort axes
R2_LONG = np.array([np.geomspace(0.1, 4.0, 13)]) ** 2


@pytest.mark.parametrize("sort_axis", [0, 2])
def test_a_diagonal_cell_over_one_long_segment(sort_axis):
    """600 objects in ONE segment against itself, ``d`` alternating by a factor 7: three stages, a padded last lane tile, and
    the first stage of every tile holding indices <= the lane's. Four pi bins. The count is the oracle's, and half the count
    of the segment against a bit-identical copy uploaded as a second handle."""
    h = long_segment(np.random.default_rng(5 + sort_axis), 600, sort_axis)
    exp = oracle.proj_pi_cells(h, h, DIAGONAL, R2_LONG, UNIFORM_4)[2]
    assert np.all(exp.sum(axis=(1, 2)) > 0) and np.count_nonzero(exp) > 40
    W, stats, W1, stats1 = count_pi(h, h, DIAGONAL, R2_LONG, UNIFORM_4, sort_axis, pmax=40.0)
    assert np.array_equal(W, exp) and stats.candidate_pairs == 600 * 599 // 2
    # the same walk as yawhip_proj_count's, where the key window leaves objects out
    assert np.array_equal(W.sum(axis=0), W1) and stats.evaluated_pairs == stats1.evaluated_pairs <= stats.candidate_pairs
    print(f"axis {sort_axis}: {stats.evaluated_pairs} of {stats.candidate_pairs} candidate pairs evaluated")
    copy = {key: (value.copy() if isinstance(value, np.ndarray) else value) for key, value in h.items()}
    both, stats = count_pi(h, copy, ACROSS, R2_LONG, UNIFORM_4, sort_axis)
    assert np.array_equal(both, 2.0 * W) and stats.candidate_pairs == 600 * 600


@pytest.mark.parametrize("sort_axis", [0, 2])
def test_a_long_segment_streamed_against_lanes_of_another(sort_axis):
    """600 streamed against 300 in the lanes, off the diagonal: three stages, the last ragged; a full lane tile and a padded
    one."""
    rng = np.random.default_rng(9 + sort_axis)
    a, b = long_segment(rng, 600, sort_axis), long_segment(rng, 300, sort_axis)
    exp = oracle.proj_pi_cells(a, b, ACROSS, R2_LONG, UNIFORM_4)[2]
    assert np.all(exp.sum(axis=(1, 2)) > 0)
    W, stats = count_pi(a, b, ACROSS, R2_LONG, UNIFORM_4, sort_axis)
    assert np.array_equal(W, exp) and stats.candidate_pairs == 600 * 300


@pytest.mark.parametrize("sort_axis", [0, 2])
def test_tied_sort_keys_across_a_tile_boundary(sort_axis):
    """150 of 600 objects share ONE sort key, from rank 180 to rank 329 of their segment (the scene of
    tests/test_gpu_projected.py): whichever order the device's sort leaves them in, a diagonal cell holds every unordered
    pair once, in its pi bin."""
    rng = np.random.default_rng(41 + sort_axis)
    h = long_segment(rng, 600, sort_axis)
    order = np.argsort(h["xyz"[sort_axis]], kind="stable")
    h["xyz"[sort_axis]][order[180:330]] = h["xyz"[sort_axis]][order[255]]
    other = long_segment(rng, 300, sort_axis)
    other["xyz"[sort_axis]][:100] = h["xyz"[sort_axis]][order[255]]
    r2 = np.array([np.geomspace(0.1, 4.0, 7)]) ** 2
    exp = oracle.proj_pi_cells(h, h, DIAGONAL, r2, UNEVEN)[2]
    tied = dict(h, **{c: h[c][order[180:330]] for c in "xyzdc"}, off=np.array([0, 150], dtype=np.int64))
    assert oracle.proj_pi_cells(tied, tied, DIAGONAL, r2, UNEVEN)[2].sum() > 100  # pairs among the tied objects themselves
    W, _ = count_pi(h, h, DIAGONAL, r2, UNEVEN, sort_axis)
    assert np.array_equal(W, exp)
    W, _ = count_pi(h, other, ACROSS, r2, UNEVEN, sort_axis)
    assert np.array_equal(W, oracle.proj_pi_cells(h, other, ACROSS, r2, UNEVEN)[2])


def test_different_sort_axes_stream_the_whole_segment():
    a, b = scene(4, False)
    cells, r2 = scenes.cells_two_handles(4), scenes.radius_edges(12, 4)
    windowed, st_windowed = count_pi(a, b, cells, r2, UNEVEN, 2, 2)
    whole, st_whole = count_pi(a, b, cells, r2, UNEVEN, 2, 0)
    assert st_whole.evaluated_pairs == st_whole.candidate_pairs >= st_windowed.evaluated_pairs
    assert np.array_equal(whole, windowed) and np.array_equal(whole, expected(4, 12, False, True, "uneven")[2])


# --------------------------------------------------------------------------- 4. the pi edges
@pytest.mark.parametrize("sort_axis", [0, 1, 2])
def test_partners_on_the_pi_edges_at_equal_c_and_beyond_the_last_radius(sort_axis):
    """Every ``d`` is 1024 and every ``c`` a multiple of 1/4, so ``p`` is exact. Around each of 40 objects six partners are
    displaced along the sort axis by the chord of a radius of 1.0 (inside the one fine bin 0.2 .. 2.5), at ``c`` behind their
    object by 0 (``p == 0``: bin 0), 10 (ON the inner edge ``pe[1]``: bin 0), 25 (ON ``pe[2]``: bin 1), 40 (ON the last edge:
    bin 2, it counts) and 40.25 (beyond it: dropped, unless the last edge is ``+inf``); a sixth at ``c`` equal sits at a radius
    of 2.5, and the last radius edge is then SET to ``DD s2`` of one such pair: that pair passes the outer test
    (``fl(DD s2) <= r2max``) and has ``R2 = DD th2 > r2max``, so it is in no plane. One ulp less of an inner edge moves the
    partners ON it up one bin; one ulp less of the last edge drops the partners ON it."""
    rng = np.random.default_rng(57 + sort_axis)
    base_xyz = box_xyz(rng, 40)
    base_c = rng.integers(0, 400, 40) * 0.25
    offsets = (0.0, 10.0, 25.0, 40.0, 40.25)
    placed, placed_c = [], []
    for at in range(40):
        for n, more in enumerate(offsets):
            p = base_xyz[:, at].copy()
            p[sort_axis] += (1.0 if n % 2 else -1.0) * 2.0 * np.sin(0.5 * (1.0 + 0.01 * n) / 1024.0)
            placed.append(p), placed_c.append(base_c[at] + more)
        p = base_xyz[:, at].copy()
        p[sort_axis] += 2.0 * np.sin(0.5 * 2.5 / 1024.0)
        placed.append(p), placed_c.append(base_c[at])
    a = one_segment(base_xyz, 1024.0, base_c)
    only_placed = one_segment(np.array(placed).T, 1024.0, np.array(placed_c))
    b = one_segment(np.concatenate([np.array(placed).T, box_xyz(rng, 300)], axis=1), 1024.0, np.concatenate([placed_c, rng.integers(0, 400, 300) * 0.25]))
    # the last radius edge: fl(DD s2) of object 0 and its sixth partner
    dx = [b[c][5] - a[c][0] for c in "xyz"]
    s2 = (dx[0] * dx[0] + dx[1] * dx[1]) + dx[2] * dx[2]
    r2 = np.array([[0.2**2, (1024.0 * 1024.0) * s2]])
    assert abs(r2[0, 1] / 6.25 - 1.0) < 1e-5 and float(proj_oracle.pair_terms(a, b, np.array([0]), np.array([5]))[0][0]) > r2[0, 1]
    pe = np.array([0.0, 10.0, 25.0, 40.0])
    inf = float("inf")
    # what the oracle says of the placed partners alone: 40 each at p = 0, 10, 25, 40 in range, none of the sixth kind
    own = np.zeros((40, len(placed)), dtype=bool)
    own[np.repeat(np.arange(40), 6), np.arange(len(placed))] = True
    R2, p, _ = proj_oracle.pair_terms(a, only_placed, np.arange(40)[:, None], np.arange(len(placed))[None, :])
    in_range = (R2 > r2[0, 0]) & (R2 <= r2[0, 1])
    assert np.array_equal(np.sort(p[own & in_range]), np.repeat([0.0, 10.0, 25.0, 40.0, 40.25], 40))
    assert not np.any(in_range[0, 5]) and np.count_nonzero(in_range & (p == 10.0)) >= 40
    N = lambda edges: oracle.proj_pi_cells(a, only_placed, ACROSS, r2, edges)[2][:, 0, 0]
    on = [int(np.count_nonzero(in_range & (p == edge))) for edge in pe]
    base = N(pe)
    assert base[0] >= on[0] + on[1] and base[1] >= on[2] and base[2] >= on[3] and min(on) >= 40
    inner = pe.copy()
    inner[1] = np.nextafter(10.0, 0.0)  # the partners ON pe[1] move from bin 0 to bin 1
    assert np.array_equal(N(inner), base + np.array([-on[1], on[1], 0]))
    last = pe.copy()
    last[3] = np.nextafter(40.0, 0.0)  # the partners ON the last edge are dropped
    assert np.array_equal(N(last), base - np.array([0, 0, on[3]]))
    open_ended = pe.copy()
    open_ended[3] = inf  # the partners beyond 40 count too
    assert N(open_ended)[2] >= base[2] + 40
    for edges in (pe, inner, last, open_ended, np.array([0.0, inf]), np.array([0.0, np.nextafter(0.0, 1.0), 40.0])):
        exp = oracle.proj_pi_cells(a, b, ACROSS, r2, edges)[2]
        W, _ = count_pi(a, b, ACROSS, r2, edges, sort_axis)
        assert np.array_equal(W, exp), edges
    assert exp[0, 0, 0] >= on[0]  # the last set: bin 0 is [0, 5e-324] and holds the pairs at p == 0


# --------------------------------------------------------------------------- 5. the LDS cap
@pytest.mark.parametrize("n_edges, cap", [(13, CAP_AT_13_EDGES), (256, CAP_AT_256_EDGES)])
def test_the_largest_n_pi_that_fits_runs_and_one_more_is_refused(n_edges, cap):
    """The formula of include/yawhip.h admits ``cap`` pi bins at ``n_edges`` and not one more; at the cap the count is the
    float64 oracle's (unit weights, uniform edges to 40, one redshift bin), one more is refused with the cap in the message."""
    assert lds_bytes(n_edges, cap) <= 65536 < lds_bytes(n_edges, cap + 1)
    a, _ = scene(1, False)
    cells, r2 = scenes.cells_one_handle(1), scenes.radius_edges(n_edges - 1, 1)
    if n_edges == 13:
        exp = expected(1, 12, False, False, cap)[2]
    else:
        exp = oracle.proj_pi_cells(a, a, cells, r2, np.linspace(0.0, scenes.PMAX, cap + 1))[2]
    assert np.all(exp.sum(axis=(1, 2)) > 0)
    W, _ = count_pi(a, a, cells, r2, np.linspace(0.0, scenes.PMAX, cap + 1))
    assert np.array_equal(W, exp)
    ctx = engine.get_context(0)
    handle = upload(ctx, a)
    try:
        with pytest.raises(_lib.YawhipError, match=f"do not fit the LDS of a workgroup: at most {cap} pi bins at n_edges={n_edges}"):
            _lib.proj_count_pi(ctx, handle, handle, cells, r2, np.linspace(0.0, scenes.PMAX, cap + 2))
    finally:
        handle.free()


def test_the_engine_states_the_cap_in_pi_bins():
    """``engine.count_projected_pi_fine`` turns the library's refusal into a ``ValueError`` with the cap for the number of
    radius edges."""
    from test_projected_pi_host import unit_scenario
    import yet_another_wizz_amd as yaw

    config, data, random = unit_scenario()
    n_edges = yaw.measurements.threshold_table(yaw.measurements.radial_plans(config)).shape[1]
    cap = next(n for n in range(1, 2000) if lds_bytes(n_edges, n + 1) > 65536)
    with pytest.raises(ValueError, match=f"{cap + 1} pi bins are too many for {n_edges} radius edges.*at most {cap} pi bins"):
        yaw.autocorrelate_projected(config, data, random, pi_max=60.0, pi_bins=cap + 1)
    for cat in (data, random):
        cat.drop_layouts()


# --------------------------------------------------------------------------- 6. weighted sums, reproducibility, every element
@pytest.mark.parametrize("sort_axis", [0, 2])
@pytest.mark.parametrize("edges", ["uniform30", "uneven"])
@pytest.mark.parametrize("nb", [4, 1])
def test_weighted_sums_match_the_oracle(nb, edges, sort_axis):
    a, b = scene(nb, True)
    r2 = scenes.radius_edges(12, nb)
    worst = 0.0
    for two in (False, True):
        cells = scenes.cells_two_handles(nb) if two else scenes.cells_one_handle(nb)
        exp_w, exp_a, exp_n = expected(nb, 12, True, two, edges)
        W, _ = count_pi(a, b if two else a, cells, r2, EDGE_SETS[edges], sort_axis)
        assert np.array_equal(W == 0.0, exp_n == 0.0)
        worst = max(worst, float(np.max(np.abs(W - exp_w)[exp_a > 0] / (EPS * exp_a[exp_a > 0]))))
        print(f"nb={nb} {edges} axis={sort_axis} {'two handles' if two else 'one handle'}: worst |ours - oracle| / (eps A) = {worst:.3f}")
        assert np.all(np.abs(W - exp_w) <= K * EPS * exp_a)


def test_two_calls_return_the_same_bits():
    a, _ = scene(1, True)
    ctx = engine.get_context(0)
    handle = upload(ctx, a)
    try:
        one = _lib.proj_count_pi(ctx, handle, handle, scenes.cells_one_handle(1), scenes.radius_edges(12, 1), UNIFORM_30)[0]
        two = _lib.proj_count_pi(ctx, handle, handle, scenes.cells_one_handle(1), scenes.radius_edges(12, 1), UNIFORM_30)[0]
    finally:
        handle.free()
    assert np.count_nonzero(one) > 1000 and np.array_equal(one, two)


def raw_call(ctx, a, b, cells, r2, n_pi, pe, out):
    """``yawhip_proj_count_pi`` on the caller's buffers (None: a NULL pointer) -> its status."""
    dp, ip = ctypes.POINTER(ctypes.c_double), ctypes.POINTER(ctypes.c_int32)
    ptr = lambda arr, typ: None if arr is None else arr.ctypes.data_as(typ)
    return _lib.load_library().yawhip_proj_count_pi(ctx._h, a._h, b._h, len(cells), ptr(cells, ip), r2.shape[0], r2.shape[1], ptr(r2, dp), n_pi,
                                                    ptr(pe, dp), ptr(out, dp), None)


def test_every_element_is_written():
    """Through a raw call on a buffer filled with NaN (``_lib._shear_counts`` allocates with ``np.empty``, which poisons
    nothing): cells over the empty segment on either side (two of the scene's and three added), and a last row of radius edges without any cell, give zeros; no
    element keeps its NaN; and the buffer is the wrapper's result."""
    a, _ = scene(4, False)
    assert a["off"][5] == a["off"][6]  # segment 5 is empty
    cells = np.ascontiguousarray(np.concatenate([scenes.cells_one_handle(4), np.array([[5, 4, 1, 0], [4, 5, 0, 0], [5, 5, 1, 1]], dtype=np.int32)]))
    r2 = np.ascontiguousarray(np.concatenate([scenes.radius_edges(12, 4), [np.geomspace(1e3, 1e6, 13)]]))  # row 4: no cell, any reach
    pe = UNEVEN.copy()
    out = np.full((len(pe) - 1, len(cells), 12), np.nan)
    ctx = engine.get_context(0)
    handle = upload(ctx, a)
    try:
        assert raw_call(ctx, handle, handle, cells, r2, len(pe) - 1, pe, out) == 0
        W, _ = _lib.proj_count_pi(ctx, handle, handle, cells, r2, pe)
    finally:
        handle.free()
    assert not np.any(np.isnan(out)) and np.array_equal(out, W)
    touches_empty = (cells[:, 0] == 5) | (cells[:, 1] == 5)
    assert touches_empty.sum() == 5 and np.all(out[:, touches_empty] == 0.0) and np.count_nonzero(out) > 1000
    assert np.array_equal(out[:, :-3], expected(4, 12, False, False, "uneven")[2])


# --------------------------------------------------------------------------- 7. refusals
def test_mismatched_handles_edges_and_arguments_are_refused():
    ctx = engine.get_context(0)
    other = _lib.Context(0)
    a, _ = scene(4, False)
    n_patches = 2 * len(scenes.SITES)
    r2 = scenes.radius_edges(1, 4)
    cells = scenes.cells_one_handle(4)
    off_diagonal = cells[len(cells) // 2:]
    handle, foreign = upload(ctx, a), upload(other, a)
    lenses = _lib.DsigmaLenses(ctx, a["x"], a["y"], a["z"], None, a["d"], a["c"], n_patches, 4, a["off"])
    radial = _lib.DsigmaLenses(ctx, a["x"], a["y"], a["z"], None, a["d"], a["c"], n_patches, 4, a["off"], m=a["d"] ** 2)
    binned = _lib.ShearSources(ctx, a["x"], a["y"], a["z"], None, a["d"], a["c"], n_patches, a["off"], n_bins=4)
    unbinned = scenes.handle(scenes.SEED_B, 1, 8, False)
    sources = _lib.ShearSources(ctx, unbinned["x"], unbinned["y"], unbinned["z"], None, unbinned["d"], unbinned["c"], n_patches, unbinned["off"], u=unbinned["c"])
    pe = UNIFORM_4
    try:
        # every other kind of handle, in either position
        for wrong in (lenses, radial, binned, sources):
            for first, second in ((wrong, handle), (handle, wrong)):
                with pytest.raises(_lib.YawhipError, match="not one of yawhip_proj_upload"):
                    _lib.proj_count_pi(ctx, first, second, off_diagonal, r2, pe)
        with pytest.raises(_lib.YawhipError, match="another context"):
            _lib.proj_count_pi(ctx, handle, foreign, off_diagonal, r2, pe)
        # n_pi and the edges
        with pytest.raises(_lib.YawhipError, match="n_pi must be >= 1"):
            _lib.proj_count_pi(ctx, handle, handle, cells, r2, np.array([0.0]))
        for first_edge in (1.0, -0.5, np.nan, np.nextafter(0.0, 1.0)):
            with pytest.raises(_lib.YawhipError, match="first pi edge must be 0"):
                _lib.proj_count_pi(ctx, handle, handle, cells, r2, np.array([first_edge, 20.0, 40.0]))
        for bad in ([0.0, np.nan, 40.0], [0.0, 20.0, np.nan], [0.0, 30.0, 20.0], [0.0, 20.0, 20.0], [0.0, 0.0, 40.0], [0.0, np.inf, np.inf],
                    [0.0, np.inf, 40.0], [0.0, -1.0]):
            with pytest.raises(_lib.YawhipError, match="strictly ascending"):
                _lib.proj_count_pi(ctx, handle, handle, cells, r2, np.array(bad))
        flat_r2, flat_cells = np.ascontiguousarray(r2), np.ascontiguousarray(cells)
        out = np.zeros((4, len(cells), 1))
        assert raw_call(ctx, handle, handle, flat_cells, flat_r2, 4, None, out) != 0  # a NULL pe
        assert "pe not NULL" in _lib.load_library().yawhip_last_error().decode()
        assert raw_call(ctx, handle, handle, flat_cells, flat_r2, 4, pe.copy(), None) != 0  # a NULL result
        assert raw_call(ctx, handle, handle, flat_cells, flat_r2, 4, pe.copy(), out) == 0 and out.sum() > 0
        _lib.proj_count_pi(ctx, handle, handle, cells, r2, np.array([0.0, 20.0, np.inf]))  # the last edge may be +inf
        # yawhip_proj_count's refusals, once each through this entry point
        with pytest.raises(_lib.YawhipError, match="an object is too close for the largest radius"):
            _lib.proj_count_pi(ctx, handle, handle, cells, np.array([[0.0, 100.0**2]] * 4), pe)
        per_bin = [np.concatenate([a["d"][a["off"][p * 4 + k]:a["off"][p * 4 + k + 1]] for p in range(n_patches)]).min() for k in range(4)]
        fits = np.array([[0.0, 0.0099 * per_bin[k] ** 2] for k in range(4)])
        _lib.proj_count_pi(ctx, handle, handle, cells, fits, pe)
        beyond = fits.copy()
        beyond[2, 1] = 0.0101 * per_bin[2] ** 2
        with pytest.raises(_lib.YawhipError, match="an object is too close for the largest radius"):
            _lib.proj_count_pi(ctx, handle, handle, cells, beyond, pe)
        _lib.proj_count_pi(ctx, handle, handle, cells[cells[:, 2] != 2], beyond, pe)  # no cell of the row: no reach
        with pytest.raises(_lib.YawhipError, match="bad sizes"):
            _lib.proj_count_pi(ctx, handle, handle, cells, scenes.radius_edges(256, 4), pe)  # 257 edges
        with pytest.raises(_lib.YawhipError, match="not ascending"):
            _lib.proj_count_pi(ctx, handle, handle, cells, scenes.radius_edges(3, 4)[:, ::-1].copy(), pe)
        for bad_cell in ((0, 0, 0, 0), (0, 1, 0, 1)):
            with pytest.raises(_lib.YawhipError, match="diagonal"):
                _lib.proj_count_pi(ctx, handle, handle, np.array([bad_cell], dtype=np.int32), r2, pe)
        W, _ = _lib.proj_count_pi(ctx, handle, handle, np.empty((0, 4), dtype=np.int32), r2, pe)  # nothing to do
        assert W.shape == (4, 0, 1)
    finally:
        for h in (handle, foreign, lenses, radial, binned, sources):
            h.free()
        other.close()


# --------------------------------------------------------------------------- 8. end to end
@pytest.mark.parametrize("count_rr", [True, False], ids=["LS", "DP"])
def test_the_driver_end_to_end(count_rr, monkeypatch):
    """The scenario of the CPU driver test through the real library, held per slot to 1e-12 of the oracle's sums recombined by
    hand, and to the driver on the stand-in."""
    from test_projected_pi_host import check_pi_driver

    on_device = check_pi_driver("kpc", count_rr, rtol=1e-12)
    monkeypatch.setattr(engine, "count_projected_pi_fine", oracle.count_projected_pi_fine)
    stand_in = check_pi_driver("kpc", count_rr, rtol=1e-12)
    for ours, theirs in zip(on_device, stand_in):
        for mine, other in zip(ours.pi_bins, theirs.pi_bins):
            for kind in ("dd", "dr") + (("rr",) if count_rr else ()):
                np.testing.assert_allclose(getattr(mine, kind).counts.counts, getattr(other, kind).counts.counts, rtol=1e-12, atol=0)
        np.testing.assert_allclose(ours.sample().data, theirs.sample().data, rtol=1e-9, atol=1e-11)


def test_the_cylinder_is_the_single_cylinder_count_on_the_device():
    """``cylinder()`` against ``autocorrelate_projected(pi_bins=None)``, both on the device: equal counts for unit weights."""
    from test_projected_pi_host import check_cylinder, driver_config, driver_scenario, unit_scenario

    config, data, random = unit_scenario()
    check_cylinder(config, data, random, exact=True)
    data, random = driver_scenario()
    check_cylinder(driver_config("kpc"), data, random, exact=False)
