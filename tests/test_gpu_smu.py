"""GPU: the redshift-space pair count (``yawhip_proj_count_smu``) and ``autocorrelate_multipoles`` on the device, against the
numpy brute force of tests/smu_oracle.py, on the scenes of tests/smu_scenes.py (whose membership in s and in mu
tests/test_smu_host.py proves exact with mpmath), and against ``yawhip_proj_count`` on the same handles.

Membership is tested EXACTLY: with unit weights ``W`` is the integer number of pairs per mu bin, cell and fine bin and must
equal the oracle's with ``np.array_equal``. Weighted sums are held to ``|ours - oracle| <= K eps A`` per mu bin, cell and fine
bin, ``A`` the sum of ``|w_a w_b|`` over its member pairs."""
import ctypes
import functools

import numpy as np
import pytest

import proj_oracle
import smu_oracle as oracle
import smu_scenes as scenes
from smu_scenes import MU_4, MU_30, MU_UNEVEN, squares
from test_gpu_projected import ACROSS, DIAGONAL, box_xyz, long_segment, one_segment, upload
from yet_another_wizz_amd import _lib, engine

pytestmark = pytest.mark.gpu
EPS = 2.0**-53
# The oracle's own worst |W - exact| / (eps A) per mu bin, cell and fine bin against the 50-digit sums of
# tests/test_smu_host.py (test_the_oracles_membership_is_exact_on_the_device_scene prints it and asserts that it still holds);
# K is four times that, rounded up to a power of two, as DESIGN.md sections 15, 19, 20 and 22 set theirs. Measured on this
# scene, not borrowed from section 20. The device's own ratio is in section 23.
K_ORACLE_RATIO = 5.329  # measured: 5.3281 (over the three mu sets, one handle and two)
K = 32.0  # 4 x 5.329 = 21.3, rounded up to a power of two
ONE_PLANE = np.array([0.0, 1.0])
MU_SETS = {"one": ONE_PLANE, **scenes.MU_SETS}
CAP_AT_13_EDGES, CAP_AT_256_EDGES = 104, 4  # include/yawhip.h: the largest n_mu whose carve-up fits 64 KiB of LDS


def lds_bytes(n_edges, n_mu):
    """The carve-up of include/yawhip.h: two stages of 48-byte objects, thresholds, mu edges, four histograms."""
    return 2 * 256 * 48 + 8 * (((n_edges + 1) & ~1) + ((n_mu + 2) & ~1)) + 4 * n_mu * (n_edges - 1) * 8


def count_smu(a, b, cells, s2, m2, axis_a=2, axis_b=None, single=False):
    """``yawhip_proj_count_smu`` of the oracle's handles ``a``, ``b`` (``b is a``: one handle passed twice) -> (W, CountStats);
    with ``single`` also ``yawhip_proj_count`` without a cut on the same handles and table -> (W, CountStats, W1, CountStats1)."""
    ctx = engine.get_context(0)
    first = upload(ctx, a, axis_a)
    second = first if b is a else upload(ctx, b, axis_a if axis_b is None else axis_b)
    try:
        W, stats = _lib.proj_count_smu(ctx, first, second, cells, s2, m2)
        more = _lib.proj_count(ctx, first, second, cells, s2, float("inf")) if single else ()
    finally:
        first.free(), second.free()
    assert W.shape == (len(m2) - 1, len(cells), np.shape(s2)[1] - 1)
    assert stats.n_workgroups == len(cells) and 0 < stats.evaluated_pairs <= stats.candidate_pairs
    return (W, stats, *more)


@functools.lru_cache(maxsize=None)
def expected(nb, nf, weighted, two, mu):
    """The oracle's (W, A, N) of the scene, one handle or two, for the mu set ``mu`` (a name of MU_SETS, or a number of equal
    bins): computed once per case, shared, never modified."""
    a, b = scenes.scene(nb, weighted)
    cells = scenes.cells_two_handles(nb) if two else scenes.cells_one_handle(nb)
    edges = MU_SETS[mu] if isinstance(mu, str) else np.linspace(0.0, 1.0, mu + 1)
    out = oracle.smu_cells(a, b if two else a, cells, scenes.s_edges(nf, nb), squares(edges))
    for arr in out:
        arr.setflags(write=False)
    return out


def candidates_by_hand(a, b, cells):
    sizes_a, sizes_b = np.diff(a["off"]), np.diff(b["off"])
    return sum(n * (n - 1) // 2 if diag else n * m for n, m, diag in zip(sizes_a[cells[:, 0]], sizes_b[cells[:, 1]], cells[:, 3] != 0))


# --------------------------------------------------------------------------- 1. exact membership
def test_the_scene_stays_off_the_edges():
    """The conditions under which tests/test_smu_host.py proves the oracle's membership exact, asserted from the scene in
    float64 for every ``nb`` and every mu set used here (DESIGN.md section 23 has the figures: nearest to an s edge 2.7e-6,
    nearest ``fl(m2_k S2)`` to ``P2`` 8.8e-7, fewest pairs per mu plane 132 and per s bin 5)."""
    for nb in (1, 4):
        a, b = scenes.scene(nb, False)
        for name, mu in scenes.MU_SETS.items():
            for two in (False, True):
                cells = scenes.cells_two_handles(nb) if two else scenes.cells_one_handle(nb)
                margin_s, margin_mu = oracle.nearest_margins(a, b if two else a, cells, scenes.s_edges(12, nb), squares(mu))
                N = expected(nb, 12, False, two, name)[2]
                assert margin_s > 1e-9 and margin_mu > 1e-9
                assert N.sum(axis=(1, 2)).min() >= 132 and N.sum(axis=(0, 1)).min() >= 5


@pytest.mark.parametrize("sort_axis", [0, 1, 2])
@pytest.mark.parametrize("mu", list(MU_SETS))
@pytest.mark.parametrize("nf", [1, 12])
@pytest.mark.parametrize("nb", [1, 4])
def test_membership_is_the_oracles(nb, nf, mu, sort_axis):
    a, b = scenes.scene(nb, False)
    s2 = scenes.s_edges(nf, nb)
    for two in (False, True):
        cells = scenes.cells_two_handles(nb) if two else scenes.cells_one_handle(nb)
        exp_w, _, exp_n = expected(nb, nf, False, two, mu)
        assert np.all(exp_n.sum(axis=(1, 2)) > 0)  # every mu plane holds pairs
        assert np.any(exp_n.sum(axis=(0, 2)) == 0) == (nb > 1)  # the empty segment
        W, stats = count_smu(a, b if two else a, cells, s2, squares(MU_SETS[mu]), sort_axis)
        assert np.array_equal(W, exp_n) and np.array_equal(exp_w, exp_n)
        assert stats.candidate_pairs == candidates_by_hand(a, b if two else a, cells)


# --------------------------------------------------------------------------- 2. the ties of the contract
@pytest.mark.parametrize("mu", ["uniform4", "uniform30", "uneven"])
@pytest.mark.parametrize("nb", [1, 4])
def test_the_planes_sum_to_the_one_plane_call_of_the_same_walk(nb, mu):
    """Over unit weights the planes sum to the ``n_mu = 1`` call as integers, and both report the candidate and evaluated pairs
    of ``yawhip_proj_count`` on the same cells and table (one walk, one window)."""
    a, b = scenes.scene(nb, False)
    s2 = scenes.s_edges(12, nb)
    for two in (False, True):
        cells = scenes.cells_two_handles(nb) if two else scenes.cells_one_handle(nb)
        W, stats, _, stats1 = count_smu(a, b if two else a, cells, s2, squares(MU_SETS[mu]), single=True)
        one, stats_one = count_smu(a, b if two else a, cells, s2, ONE_PLANE)
        assert one.sum() > 1000 and np.array_equal(W.sum(axis=0), one[0])
        for st in (stats, stats_one):
            assert (st.candidate_pairs, st.evaluated_pairs) == (stats1.candidate_pairs, stats1.evaluated_pairs)


@pytest.mark.parametrize("nb", [1, 4])
def test_a_constant_line_of_sight_column_gives_the_projected_count(nb):
    """``c`` constant: ``p = 0`` and ``S2 = R2`` exactly, so the one plane is ``yawhip_proj_count(pmax = +inf)`` bit for bit,
    and all pairs of a several-plane call sit in plane 0."""
    a, b = (dict(h, c=np.full(len(h["c"]), 2.75)) for h in scenes.scene(nb, False))
    s2 = scenes.s_edges(12, nb)
    for first, second, cells in ((a, a, scenes.cells_one_handle(nb)), (a, b, scenes.cells_two_handles(nb))):
        one, _, W1, _ = count_smu(first, second, cells, s2, ONE_PLANE, single=True)
        assert W1.sum() > 1000 and np.array_equal(one[0], W1)
        W, _ = count_smu(first, second, cells, s2, squares(MU_UNEVEN))
        assert np.array_equal(W[0], W1) and not np.any(W[1:])


def test_one_sky_position_counts_in_the_last_plane_and_exact_duplicates_in_none():
    """Two objects at one sky position with different ``c`` have ``R2 = 0`` and ``S2 = P2``: they ARE counted -- which
    ``yawhip_proj_count`` never does -- and go to the last plane. Exact duplicates (``S2 = 0``) are in no bin."""
    rng = np.random.default_rng(71)
    xyz = box_xyz(rng, 50)
    xyz = np.concatenate([xyz, xyz[:, :20], xyz[:, :10]], axis=1)  # 20 at a first object's position, 10 exact duplicates
    c = np.concatenate([rng.uniform(0.0, 4.0, 50), rng.uniform(0.0, 4.0, 20), np.zeros(10)])
    c[70:] = c[:10]
    h = one_segment(xyz, 1024.0, c)
    s2 = np.array([np.geomspace(0.01, 6.0, 7)]) ** 2
    exp = oracle.smu_cells(h, h, DIAGONAL, s2, squares(MU_4))[2]
    W, _ = count_smu(h, h, DIAGONAL, s2, squares(MU_4))
    assert np.array_equal(W, exp)
    # the pairs at one position: S2 = P2 > 0 for 20 + 10 of them (a duplicate against its twin's partner), S2 = 0 for 10
    R2, p, _ = proj_oracle.pair_terms(h, h, np.arange(80)[:, None], np.arange(80)[None, :])
    at_one_place = np.triu(R2 == 0.0, 1)
    assert at_one_place.sum() == 20 + 10 + 10 and np.count_nonzero(at_one_place & (p == 0.0)) == 10
    in_range = at_one_place & (p * p > s2[0, 0]) & (p * p <= s2[0, -1])
    assert in_range.sum() >= 15 and np.all(oracle.mu_plane((R2 + p * p)[in_range], (p * p)[in_range], squares(MU_4)) == 3)
    # ... alone: the 20 first objects against their partners and duplicates, cell by cell one position each
    cells = np.array([(k, 20 + k, 0, 0) for k in range(20)], dtype=np.int32)
    firsts = dict(one_segment(xyz[:, :20], 1024.0, c[:20]), off=np.arange(21, dtype=np.int64))
    sizes = np.array([1 + (k < 10) for k in range(20)])  # partner k, and for k < 10 its duplicate of the first object
    order = np.concatenate([[50 + k] + ([70 + k] if k < 10 else []) for k in range(20)])
    others = dict(one_segment(xyz[:, order], 1024.0, c[order]), off=np.concatenate([[0] * 21, np.cumsum(sizes)]).astype(np.int64))
    alone = oracle.smu_cells(firsts, others, cells, s2, squares(MU_4))[2]
    assert alone.sum() == in_range[:20, 50:70].sum() >= 10 and not np.any(alone[:3])
    for h_ in (firsts, others):
        h_["n_patches"] = len(h_["off"]) - 1
    W, _, W1, _ = count_smu(firsts, others, cells, s2, squares(MU_4), single=True)
    assert np.array_equal(W, alone) and not np.any(W1)  # yawhip_proj_count never counts them


# --------------------------------------------------------------------------- 3. large cells
S2_LONG = np.array([np.geomspace(0.1, 4.0, 13)]) ** 2


def long_cell(rng, n, sort_axis):
    """``test_gpu_projected.long_segment`` with ``c`` alternating between two sheets 1.5 apart (and spread by 0.5) in the
    order of the sort key."""
    h = long_segment(rng, n, sort_axis)
    c = np.empty(n)
    c[np.argsort(h["xyz"[sort_axis]], kind="stable")] = np.where(np.arange(n) % 2 == 0, 0.0, 1.5)
    return dict(h, c=c + rng.uniform(0.0, 0.5, n))


@pytest.mark.parametrize("sort_axis", [0, 2])
def test_a_diagonal_cell_over_one_long_segment(sort_axis):
    """600 objects in ONE segment against itself, ``d`` alternating by a factor 7 and ``c`` between two sheets: three
    stages, a padded last lane tile, and the first stage of every tile holding indices <= the lane's. Four mu bins. The count
    is the oracle's, and half the count of the segment against a bit-identical copy uploaded as a second handle."""
    h = long_cell(np.random.default_rng(5 + sort_axis), 600, sort_axis)
    exp = oracle.smu_cells(h, h, DIAGONAL, S2_LONG, squares(MU_4))[2]
    assert np.all(exp.sum(axis=(1, 2)) > 0) and np.count_nonzero(exp) > 40
    W, stats, _, stats1 = count_smu(h, h, DIAGONAL, S2_LONG, squares(MU_4), sort_axis, single=True)
    assert np.array_equal(W, exp) and stats.candidate_pairs == 600 * 599 // 2
    assert stats.evaluated_pairs == stats1.evaluated_pairs <= stats.candidate_pairs
    copy = {key: (value.copy() if isinstance(value, np.ndarray) else value) for key, value in h.items()}
    both, stats = count_smu(h, copy, ACROSS, S2_LONG, squares(MU_4), sort_axis)
    assert np.array_equal(both, 2.0 * W) and stats.candidate_pairs == 600 * 600


@pytest.mark.parametrize("sort_axis", [0, 2])
def test_a_long_segment_streamed_against_lanes_of_another(sort_axis):
    """600 streamed against 300 in the lanes, off the diagonal: three stages, the last ragged; a full lane tile and a padded
    one."""
    rng = np.random.default_rng(9 + sort_axis)
    a, b = long_cell(rng, 600, sort_axis), long_cell(rng, 300, sort_axis)
    exp = oracle.smu_cells(a, b, ACROSS, S2_LONG, squares(MU_4))[2]
    assert np.all(exp.sum(axis=(1, 2)) > 0)
    W, stats = count_smu(a, b, ACROSS, S2_LONG, squares(MU_4), sort_axis)
    assert np.array_equal(W, exp) and stats.candidate_pairs == 600 * 300


# --------------------------------------------------------------------------- 4. the edges
@pytest.mark.parametrize("sort_axis", [0, 2])
def test_pairs_on_an_s_edge_on_a_mu_edge_and_beyond_the_last_edge(sort_axis):
    """Edges SET to a chosen pair's own values (one segment of 200 against one of 300, ``d`` 1024).
    An s edge at the pair's ``S2``: the pair is in the lower bin; one ulp less of the edge: in the upper bin. An inner mu edge
    at ``fl(P2 / S2)`` of the pair and at its two float neighbours: the device puts the pair where the float64 oracle does in
    all three cases, and the plane changes across them. A last edge at ``fl(fl(DD s2c) + P2)`` of a pair with a larger
    ``S2``: the pair passes the outer test and is in no plane. ``p = 0`` pairs are in plane 0."""
    rng = np.random.default_rng(83 + sort_axis)
    a = one_segment(box_xyz(rng, 200, 40.0, 40.3), 1024.0, rng.uniform(0.0, 3.0, 200))
    b = one_segment(box_xyz(rng, 300, 40.0, 40.3), 1024.0, rng.uniform(0.0, 3.0, 300))
    b["c"][:40] = a["c"][:40]  # p == 0 against object i of a, wherever it lies
    i, j = np.arange(200)[:, None], np.arange(300)[None, :]
    S2, P2, _ = oracle.smu_terms(a, b, i, j)
    base = np.array([[0.5, 2.0, 4.5]]) ** 2
    inside = np.argwhere((S2 > 1.0) & (S2 < 3.0) & (P2 > 0.2 * S2) & (P2 < 0.8 * S2))
    assert len(inside) > 50
    three_edges = lambda ratio: (np.nextafter(ratio, 0.0), ratio, np.nextafter(ratio, 1.0))
    # the chosen pair: the first whose plane changes across fl(P2 / S2) and its two float neighbours as an inner edge (one ulp
    # of the edge moves fl(m2_k S2) by half an ulp to two ulps of P2, so it does for most pairs and not for all)
    ci, cj = next((i_, j_) for i_, j_ in inside
                  if oracle.mu_plane(S2[i_, j_], P2[i_, j_], [0.0, 0.1, three_edges(P2[i_, j_] / S2[i_, j_])[0], 0.9, 1.0]) == 2
                  and oracle.mu_plane(S2[i_, j_], P2[i_, j_], [0.0, 0.1, three_edges(P2[i_, j_] / S2[i_, j_])[2], 0.9, 1.0]) == 1)
    member = lambda s2, m2: oracle.smu_cells(a, b, ACROSS, s2, m2)[2]
    slot_of = lambda s2, m2: (int(oracle.mu_plane(S2[ci, cj], P2[ci, cj], m2)), int((S2[ci, cj] > s2[0]).sum()) - 1)

    cases = []
    # the s edge
    on, under = base.copy(), base.copy()
    on[0, 1], under[0, 1] = S2[ci, cj], np.nextafter(S2[ci, cj], 0.0)
    assert slot_of(on, squares(MU_4))[1] == 0 and slot_of(under, squares(MU_4))[1] == 1
    cases += [(on, squares(MU_4)), (under, squares(MU_4))]
    # the mu edge: fl(P2 / S2) and its neighbours
    ratio = P2[ci, cj] / S2[ci, cj]
    planes = []
    for edge in three_edges(ratio):
        m2 = np.array([0.0, 0.1, edge, 0.9, 1.0])
        planes.append(slot_of(base, m2)[0])
        cases.append((base, m2))
    assert planes[0] == 2 and planes[-1] == 1 and planes[1] in (1, 2)  # the plane changes across the three
    # the last edge: a pair behind the ballot with S2 beyond it
    dx = [b[c][None, :] - a[c][:, None] for c in "xyz"]
    chord2 = (dx[0] * dx[0] + dx[1] * dx[1]) + dx[2] * dx[2]
    outer = (1024.0 * 1024.0) * chord2 + P2
    beyond = np.argwhere((outer < S2) & (S2 > 3.0) & (S2 < 9.0))
    assert len(beyond) > 0  # (th2 > s2c by more than an ulp of S2 for some pair)
    bi, bj = beyond[0]
    last = base.copy()
    last[0, 2] = outer[bi, bj]
    assert S2[bi, bj] > last[0, 2] >= outer[bi, bj]
    cases.append((last, squares(MU_4)))
    for s2, m2 in cases:
        exp = member(s2, m2)
        W, _ = count_smu(a, b, ACROSS, s2, m2, sort_axis)
        assert exp.sum() > 100 and np.array_equal(W, exp), (s2, m2)
    # p == 0: plane 0
    zero = (P2 == 0.0) & (S2 > base[0, 0]) & (S2 <= base[0, -1])
    only = oracle.smu_cells(a, dict(b, **{c: b[c][:40] for c in "xyzdc"}, off=np.array([0, 40], dtype=np.int64)), ACROSS, base, squares(MU_30))[2]
    assert zero.sum() >= 1 and only[0].sum() >= zero.sum()


# --------------------------------------------------------------------------- 5. the LDS cap
@pytest.mark.parametrize("n_edges, cap", [(13, CAP_AT_13_EDGES), (256, CAP_AT_256_EDGES)])
def test_the_largest_n_mu_that_fits_runs_and_one_more_is_refused(n_edges, cap):
    """The formula of include/yawhip.h admits ``cap`` mu bins at ``n_edges`` and not one more; at the cap the count is the
    float64 oracle's (unit weights, equal bins, one redshift bin), one more is refused with the cap in the message."""
    assert lds_bytes(n_edges, cap) <= 65536 < lds_bytes(n_edges, cap + 1)
    a, _ = scenes.scene(1, False)
    cells, s2 = scenes.cells_one_handle(1), scenes.s_edges(n_edges - 1, 1)
    m2 = squares(np.linspace(0.0, 1.0, cap + 1))
    exp = oracle.smu_cells(a, a, cells, s2, m2)[2]
    assert exp.sum() > 1000 and np.count_nonzero(exp.sum(axis=(1, 2))) >= min(cap, 90)
    W, _ = count_smu(a, a, cells, s2, m2)
    assert np.array_equal(W, exp)
    ctx = engine.get_context(0)
    handle = upload(ctx, a)
    try:
        with pytest.raises(_lib.YawhipError, match=f"do not fit the LDS of a workgroup: at most {cap} mu bins at n_edges={n_edges}"):
            _lib.proj_count_smu(ctx, handle, handle, cells, s2, squares(np.linspace(0.0, 1.0, cap + 2)))
    finally:
        handle.free()


def test_the_engine_states_the_cap_in_mu_bins():
    """``engine.count_smu_fine`` turns the library's refusal into a ``ValueError`` with the cap for the number of s edges."""
    from test_smu_host import unit_scenario
    import yet_another_wizz_amd as yaw

    config, data, random = unit_scenario()
    n_edges = yaw.measurements.threshold_table(yaw.measurements.radial_plans(config)).shape[1]
    cap = next(n for n in range(1, 2000) if lds_bytes(n_edges, n + 1) > 65536)
    with pytest.raises(ValueError, match=f"{cap + 1} mu bins are too many for {n_edges} s edges.*at most {cap} mu bins"):
        yaw.autocorrelate_multipoles(config, data, random, mu_bins=cap + 1)
    for cat in (data, random):
        cat.drop_layouts()


# --------------------------------------------------------------------------- 6. writes and repeatability
def raw_call(ctx, a, b, cells, s2, n_mu, m2, out):
    """``yawhip_proj_count_smu`` on the caller's buffers (None: a NULL pointer) -> its status."""
    dp, ip = ctypes.POINTER(ctypes.c_double), ctypes.POINTER(ctypes.c_int32)
    ptr = lambda arr, typ: None if arr is None else arr.ctypes.data_as(typ)
    return _lib.load_library().yawhip_proj_count_smu(ctx._h, a._h, b._h, len(cells), ptr(cells, ip), s2.shape[0], s2.shape[1], ptr(s2, dp), n_mu,
                                                     ptr(m2, dp), ptr(out, dp), None)


def test_every_element_is_written():
    """Through a raw call on a buffer filled with NaN: cells over the empty segment on either side (two of the scene's and
    three added), and a last row of s edges without any cell, give zeros; no element keeps its NaN; and the buffer is the
    wrapper's result."""
    a, _ = scenes.scene(4, False)
    assert a["off"][5] == a["off"][6]  # segment 5 is empty
    cells = np.ascontiguousarray(np.concatenate([scenes.cells_one_handle(4), np.array([[5, 4, 1, 0], [4, 5, 0, 0], [5, 5, 1, 1]], dtype=np.int32)]))
    s2 = np.ascontiguousarray(np.concatenate([scenes.s_edges(12, 4), [np.geomspace(1e3, 1e6, 13)]]))  # row 4: no cell, any reach
    m2 = squares(MU_UNEVEN)
    out = np.full((len(m2) - 1, len(cells), 12), np.nan)
    ctx = engine.get_context(0)
    handle = upload(ctx, a)
    try:
        assert raw_call(ctx, handle, handle, cells, s2, len(m2) - 1, m2, out) == 0
        W, _ = _lib.proj_count_smu(ctx, handle, handle, cells, s2, m2)
    finally:
        handle.free()
    assert not np.any(np.isnan(out)) and np.array_equal(out, W)
    touches_empty = (cells[:, 0] == 5) | (cells[:, 1] == 5)
    assert touches_empty.sum() == 5 and np.all(out[:, touches_empty] == 0.0) and np.count_nonzero(out) > 1000
    assert np.array_equal(out[:, :-3], expected(4, 12, False, False, "uneven")[2])


def test_two_calls_return_the_same_bits():
    a, _ = scenes.scene(1, True)
    ctx = engine.get_context(0)
    handle = upload(ctx, a)
    try:
        one = _lib.proj_count_smu(ctx, handle, handle, scenes.cells_one_handle(1), scenes.s_edges(12, 1), squares(MU_30))[0]
        two = _lib.proj_count_smu(ctx, handle, handle, scenes.cells_one_handle(1), scenes.s_edges(12, 1), squares(MU_30))[0]
    finally:
        handle.free()
    assert np.count_nonzero(one) > 300 and np.array_equal(one, two)


@pytest.mark.parametrize("sort_axis", [0, 2])
def test_tied_sort_keys_across_a_tile_boundary(sort_axis):
    """150 of 600 objects share ONE sort key, from rank 180 to rank 329 of their segment: whichever order the device's sort
    leaves them in, a diagonal cell holds every unordered pair once, in its mu plane."""
    rng = np.random.default_rng(41 + sort_axis)
    h = long_cell(rng, 600, sort_axis)
    order = np.argsort(h["xyz"[sort_axis]], kind="stable")
    h["xyz"[sort_axis]][order[180:330]] = h["xyz"[sort_axis]][order[255]]
    other = long_cell(rng, 300, sort_axis)
    other["xyz"[sort_axis]][:100] = h["xyz"[sort_axis]][order[255]]
    s2 = np.array([np.geomspace(0.1, 4.0, 7)]) ** 2
    m2 = squares(MU_UNEVEN)
    exp = oracle.smu_cells(h, h, DIAGONAL, s2, m2)[2]
    tied = dict(h, **{c: h[c][order[180:330]] for c in "xyzdc"}, off=np.array([0, 150], dtype=np.int64))
    assert oracle.smu_cells(tied, tied, DIAGONAL, s2, m2)[2].sum() > 100  # pairs among the tied objects themselves
    W, _ = count_smu(h, h, DIAGONAL, s2, m2, sort_axis)
    assert np.array_equal(W, exp)
    W, _ = count_smu(h, other, ACROSS, s2, m2, sort_axis)
    assert np.array_equal(W, oracle.smu_cells(h, other, ACROSS, s2, m2)[2])


def test_different_sort_axes_stream_the_whole_segment():
    a, b = scenes.scene(4, False)
    cells, s2 = scenes.cells_two_handles(4), scenes.s_edges(12, 4)
    windowed, st_windowed = count_smu(a, b, cells, s2, squares(MU_UNEVEN), 2, 2)
    whole, st_whole = count_smu(a, b, cells, s2, squares(MU_UNEVEN), 2, 0)
    assert st_whole.evaluated_pairs == st_whole.candidate_pairs >= st_windowed.evaluated_pairs
    assert np.array_equal(whole, windowed) and np.array_equal(whole, expected(4, 12, False, True, "uneven")[2])


@pytest.mark.parametrize("sort_axis", [0, 2])
@pytest.mark.parametrize("mu", ["uniform30", "uneven"])
@pytest.mark.parametrize("nb", [4, 1])
def test_weighted_sums_match_the_oracle(nb, mu, sort_axis):
    a, b = scenes.scene(nb, True)
    s2 = scenes.s_edges(12, nb)
    worst = 0.0
    for two in (False, True):
        cells = scenes.cells_two_handles(nb) if two else scenes.cells_one_handle(nb)
        exp_w, exp_a, exp_n = expected(nb, 12, True, two, mu)
        W, _ = count_smu(a, b if two else a, cells, s2, squares(MU_SETS[mu]), sort_axis)
        assert np.array_equal(W == 0.0, exp_n == 0.0) and not np.any(np.signbit(W[exp_n == 0.0]))  # exact +0.0 where the oracle is empty
        worst = max(worst, float(np.max(np.abs(W - exp_w)[exp_a > 0] / (EPS * exp_a[exp_a > 0]))))
        print(f"nb={nb} {mu} axis={sort_axis} {'two handles' if two else 'one handle'}: worst |ours - oracle| / (eps A) = {worst:.3f}")
        assert np.all(np.abs(W - exp_w) <= K * EPS * exp_a)


# --------------------------------------------------------------------------- 7. refusals
def test_mismatched_handles_edges_and_arguments_are_refused():
    ctx = engine.get_context(0)
    other = _lib.Context(0)
    a, _ = scenes.scene(4, False)
    n_patches = a["n_patches"]
    s2 = scenes.s_edges(1, 4)
    cells = scenes.cells_one_handle(4)
    off_diagonal = cells[len(cells) // 2:]
    handle, foreign = upload(ctx, a), upload(other, a)
    lenses = _lib.DsigmaLenses(ctx, a["x"], a["y"], a["z"], None, a["d"], a["c"], n_patches, 4, a["off"])
    radial = _lib.DsigmaLenses(ctx, a["x"], a["y"], a["z"], None, a["d"], a["c"], n_patches, 4, a["off"], m=a["d"] ** 2)
    binned = _lib.ShearSources(ctx, a["x"], a["y"], a["z"], None, a["d"], a["c"], n_patches, a["off"], n_bins=4)
    unbinned = scenes.handle(scenes.SEED_B, 1, False)
    sources = _lib.ShearSources(ctx, unbinned["x"], unbinned["y"], unbinned["z"], None, unbinned["d"], unbinned["c"], n_patches, unbinned["off"], u=unbinned["c"])
    m2 = squares(MU_4)
    try:
        # every other kind of handle, in either position
        for wrong in (lenses, radial, binned, sources):
            for first, second in ((wrong, handle), (handle, wrong)):
                with pytest.raises(_lib.YawhipError, match="not one of yawhip_proj_upload"):
                    _lib.proj_count_smu(ctx, first, second, off_diagonal, s2, m2)
        with pytest.raises(_lib.YawhipError, match="another context"):
            _lib.proj_count_smu(ctx, handle, foreign, off_diagonal, s2, m2)
        # n_mu and the edges
        with pytest.raises(_lib.YawhipError, match="n_mu must be >= 1"):
            _lib.proj_count_smu(ctx, handle, handle, cells, s2, np.array([0.0]))
        for ends in ([0.25, 0.5, 1.0], [-0.5, 0.5, 1.0], [np.nan, 0.5, 1.0], [np.nextafter(0.0, 1.0), 0.5, 1.0],
                     [0.0, 0.5, 0.75], [0.0, 0.5, np.nextafter(1.0, 2.0)], [0.0, 0.5, np.nan], [0.0, 0.5, np.inf]):
            with pytest.raises(_lib.YawhipError, match="must start at 0 and end at 1"):
                _lib.proj_count_smu(ctx, handle, handle, cells, s2, np.array(ends))
        for bad in ([0.0, np.nan, 1.0], [0.0, 0.7, 0.3, 1.0], [0.0, 0.5, 0.5, 1.0], [0.0, 0.0, 1.0], [0.0, 1.0, 1.0], [0.0, 1.5, 1.0], [0.0, -0.5, 1.0]):
            with pytest.raises(_lib.YawhipError, match="strictly ascending"):
                _lib.proj_count_smu(ctx, handle, handle, cells, s2, np.array(bad))
        flat_s2, flat_cells = np.ascontiguousarray(s2), np.ascontiguousarray(cells)
        out = np.zeros((4, len(cells), 1))
        assert raw_call(ctx, handle, handle, flat_cells, flat_s2, 4, None, out) != 0  # a NULL m2
        assert "m2 not NULL" in _lib.load_library().yawhip_last_error().decode()
        assert raw_call(ctx, handle, handle, flat_cells, flat_s2, 4, m2.copy(), None) != 0  # a NULL result
        assert raw_call(ctx, handle, handle, flat_cells, flat_s2, 4, m2.copy(), out) == 0 and out.sum() > 0
        # yawhip_proj_count's refusals, once each through this entry point
        with pytest.raises(_lib.YawhipError, match="an object is too close for the largest radius"):
            _lib.proj_count_smu(ctx, handle, handle, cells, np.array([[0.0, 100.0**2]] * 4), m2)
        with pytest.raises(_lib.YawhipError, match="bad sizes"):
            _lib.proj_count_smu(ctx, handle, handle, cells, scenes.s_edges(256, 4), m2)  # 257 edges
        with pytest.raises(_lib.YawhipError, match="not ascending"):
            _lib.proj_count_smu(ctx, handle, handle, cells, scenes.s_edges(3, 4)[:, ::-1].copy(), m2)
        for bad_cell in ((0, 0, 0, 0), (0, 1, 0, 1)):
            with pytest.raises(_lib.YawhipError, match="diagonal"):
                _lib.proj_count_smu(ctx, handle, handle, np.array([bad_cell], dtype=np.int32), s2, m2)
        W, _ = _lib.proj_count_smu(ctx, handle, handle, np.empty((0, 4), dtype=np.int32), s2, m2)  # nothing to do
        assert W.shape == (4, 0, 1)
    finally:
        for h in (handle, foreign, lenses, radial, binned, sources):
            h.free()
        other.close()


# --------------------------------------------------------------------------- 8. long lists
def test_long_lists_alternating_with_the_pi_count_on_one_pair_of_handles():
    """The cell list of tests/test_gpu_shear_long_lists.py (a few thousand cells over 150 patches, two handles) times 8 mu
    planes, as listed and shuffled, alternating with ``yawhip_proj_count_pi`` on ONE pair of handles (few / full / few): the
    call's input block and result block grow and shrink between the two entry points, and each result must be the bits of the
    same call on fresh handles."""
    import test_gpu_shear_long_lists as long_lists

    pa, pb, pe = long_lists.proj_scene()
    pa, pb = (dict(h, c=h["c"] * 2.0**-6) for h in (pa, pb))  # c 0 .. 4.7 against radii of a few: every mu is populated
    pe = pe * 2.0**-6
    count = long_lists.Count("proj2")
    full = long_lists.proj_cells(False)
    mixed = np.ascontiguousarray(full[long_lists.shuffled(len(full))])
    assert len(full) > 2000
    m2 = squares(np.linspace(0.0, 1.0, 9))
    ctx = engine.get_context(0)
    make = lambda: tuple(_lib.ProjHandle(ctx, h["x"], h["y"], h["z"], h["w"], h["d"], h["c"], long_lists.P, long_lists.NB, h["off"]) for h in (pa, pb))

    def fresh(call, cells):
        handles = make()
        try:
            return call(handles, cells)[0]
        finally:
            long_lists.free(handles)

    smu = lambda handles, cells: _lib.proj_count_smu(ctx, *handles, cells, count.t, m2)
    pi = lambda handles, cells: _lib.proj_count_pi(ctx, *handles, cells, count.t, pe)
    live = np.flatnonzero(fresh(smu, full).sum(axis=(0, 2)) > 0)
    assert len(live) > 100
    few = np.ascontiguousarray(full[np.concatenate([live[:4], [0, len(full) - 1]])])
    steps = [(smu, few), (pi, full), (smu, full), (pi, few), (smu, mixed), (pi, mixed), (smu, few)]
    handles = make()
    try:
        got = [call(handles, cells)[0] for call, cells in steps]
    finally:
        long_lists.free(handles)
    for n, ((call, cells), W) in enumerate(zip(steps, got)):
        assert W.shape[1] == len(cells) and np.array_equal(W, fresh(call, cells)), n
    assert got[2].sum() > 1000 and np.all(got[2].sum(axis=(1, 2)) > 0)  # every mu plane holds pairs
    assert np.array_equal(got[4], got[2][:, long_lists.shuffled(len(full))])
    exp = oracle.smu_cells(pa, pb, few, count.t, m2)[2]
    assert exp.sum() > 0 and np.array_equal(got[0], exp) and np.array_equal(got[6], exp)


# --------------------------------------------------------------------------- 9. end to end
@pytest.mark.parametrize("count_rr", [True, False], ids=["LS", "DP"])
def test_the_driver_end_to_end(count_rr, monkeypatch):
    """The scenario of the CPU driver test through the real library, held per slot to 1e-12 of the oracle's sums recombined by
    hand, and to the driver on the stand-in."""
    from test_smu_host import check_smu_driver

    on_device = check_smu_driver("Mpc/h", count_rr, rtol=1e-12)
    monkeypatch.setattr(engine, "count_smu_fine", oracle.count_smu_fine)
    stand_in = check_smu_driver("Mpc/h", count_rr, rtol=1e-12)
    for ours, theirs in zip(on_device, stand_in):
        for mine, other in zip(ours.mu_bins, theirs.mu_bins):
            for kind in ("dd", "dr") + (("rr",) if count_rr else ()):
                np.testing.assert_allclose(getattr(mine, kind).counts.counts, getattr(other, kind).counts.counts, rtol=1e-12, atol=0)


def test_the_nearby_sample_end_to_end(monkeypatch):
    """``autocorrelate_multipoles`` on the nearby sample of tests/test_gpu_projected.py (unit weights, 25 patches, a linkage
    that reaches past neighbouring patches), against the driver on the stand-in: every slot to 1e-12, and the counts -- those
    of unit weights -- equal as integers."""
    import yet_another_wizz_amd as yaw
    from test_projected_host import wide_scenario

    config, data, random = wide_scenario()
    on_device = yaw.autocorrelate_multipoles(config, data, random, mu_bins=MU_UNEVEN)
    monkeypatch.setattr(engine, "count_smu_fine", oracle.count_smu_fine)
    stand_in = yaw.autocorrelate_multipoles(config, data, random, mu_bins=MU_UNEVEN)
    assert len(on_device) == len(stand_in) == 1
    for ours, theirs in zip(on_device, stand_in):
        for mine, other in zip(ours.mu_bins, theirs.mu_bins):
            for kind in ("dd", "dr", "rr"):
                got, exp = getattr(mine, kind).counts.counts, getattr(other, kind).counts.counts
                assert np.all(exp == np.rint(exp)) and np.array_equal(got, exp), kind
                np.testing.assert_allclose(got, exp, rtol=1e-12, atol=0)
        assert sum(getattr(plane, "dd").counts.counts.sum() for plane in theirs.mu_bins) > 100
        for ell in (0, 2, 4):
            with np.errstate(divide="ignore", invalid="ignore"):
                np.testing.assert_array_equal(ours.sample(ell).data, theirs.sample(ell).data)
    for cat in (data, random):
        cat.drop_layouts()
