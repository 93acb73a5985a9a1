"""GPU: the projected shape-shape count (``yawhip_proj_count_shapes``) and ``autocorrelate_alignment`` on the device, against
the numpy brute force of tests/proj_shape_oracle.py, on the scenes of tests/proj_scenes.py with seeded ``g1``, ``g2`` on both
handles, and against ``yawhip_proj_count_pi`` on the shapes' ``(x, y, z, w, d, c)``.

Membership is tested EXACTLY: with unit weights ``W`` is the integer number of pairs per pi bin, cell and fine bin and must
equal the oracle's with ``np.array_equal``. ``PP``, ``XX`` and ``PX`` are held to ``|ours - oracle| <= 1e-10 A`` per pi bin,
cell and fine bin, ``A = sum |w_a w_b| (|g1_a| + |g2_a|) (|g1_b| + |g2_b|)`` over its member pairs: the project's rule for a
signed sum."""
import functools

import numpy as np
import pytest

import proj_scenes as scenes
import proj_shape_oracle as oracle
from proj_pi_oracle import UNEVEN, UNIFORM_4
from shear_oracle import tangential_pattern
from test_gpu_projected import ACROSS, DIAGONAL, box_xyz, long_segment, one_segment, scene, upload
from test_gpu_projected_shear import upload_shapes, with_shear
from test_shear_host import ring_around
from yet_another_wizz_amd import _lib, engine
from yet_another_wizz_amd.catalog import radec_to_xyz

pytestmark = pytest.mark.gpu
RTOL_A = 1e-10  # the project's tolerance of a signed sum, relative to its cancellation-free magnitude A
ONE_BIN = np.array([0.0, scenes.PMAX])
EDGE_SETS = {"one": ONE_BIN, "uniform4": UNIFORM_4, "uneven": UNEVEN}
CAPS = {13: 21, 51: 5}  # include/yawhip.h: the largest n_pi whose carve-up fits 64 KiB of LDS
R2_LONG = np.array([np.geomspace(0.1, 4.0, 13)]) ** 2


def count_shapes(a, b, cells, r2, pe, axis_a=2, axis_b=None, tie=False):
    """``yawhip_proj_count_shapes`` of the oracle's shape handles ``a``, ``b`` (``b is a``: ONE handle passed twice) ->
    ((PP, XX, PX, W), CountStats); ``tie``: also ``yawhip_proj_count_pi`` on the same columns as plain projected handles ->
    (..., W_pi, CountStats_pi)."""
    ctx = engine.get_context(0)
    axis_b = axis_a if axis_b is None else axis_b
    made = [upload_shapes(ctx, a, axis_a)]
    try:
        if b is not a:
            made.append(upload_shapes(ctx, b, axis_b))
        planes, stats = _lib.proj_count_shapes(ctx, made[0], made[-1], cells, r2, pe)
        extra = ()
        if tie:
            first = len(made)
            made.append(upload(ctx, a, axis_a))
            if b is not a:
                made.append(upload(ctx, b, axis_b))
            extra = _lib.proj_count_pi(ctx, made[first], made[-1], cells, r2, pe)
    finally:
        for handle in made:
            handle.free()
    assert len(planes) == 4 and all(p.shape == (len(pe) - 1, len(cells), np.shape(r2)[1] - 1) for p in planes)
    assert stats.n_workgroups == len(cells) and stats.evaluated_pairs <= stats.candidate_pairs
    return (planes, stats, *extra)


@functools.lru_cache(maxsize=None)
def shape_scene(nb, weighted):
    a, b = scene(nb, weighted)
    return with_shear(a, 200 + nb), with_shear(b, 100 + nb)


def scene_cells(nb, two):
    return scenes.cells_two_handles(nb) if two else scenes.cells_one_handle(nb)


@functools.lru_cache(maxsize=None)
def expected(nb, nf, weighted, edges, two):
    """The oracle's (PP, XX, PX, W, A, N) of the scene, two handles (all cells) or one (``p <= q`` and diagonal cells):
    computed once per case, shared, never modified."""
    a, b = shape_scene(nb, weighted)
    out = oracle.proj_shape_cells(a, b if two else a, scene_cells(nb, two), scenes.radius_edges(nf, nb), EDGE_SETS[edges])
    for arr in out:
        arr.setflags(write=False)
    return out


def check_planes(got, exp, label="", factor=1.0):
    """PP, XX, PX under the rule against ``factor`` times the oracle's, cells without pairs exactly 0; returns the worst
    ``|ours - oracle| / A``."""
    exp_a, exp_n = exp[4], exp[5]
    worst = 0.0
    for name, ours, theirs in zip(("PP", "XX", "PX"), got, exp):
        assert np.all(ours[exp_n == 0] == 0.0), (label, name)
        assert np.all(np.abs(ours - factor * theirs) <= RTOL_A * factor * exp_a), (label, name)
        if np.any(exp_a > 0):
            worst = max(worst, float(np.max(np.abs(ours - factor * theirs)[exp_a > 0] / (factor * exp_a[exp_a > 0]))))
    assert np.all(got[3][exp_n == 0] == 0.0), label
    return worst


# --------------------------------------------------------------------------- 1. against the oracle, and the tie to the pi count
@pytest.mark.parametrize("sort_axis", [0, 1, 2])
@pytest.mark.parametrize("edges", list(EDGE_SETS))
@pytest.mark.parametrize("nb, nf", [(1, 1), (1, 50), (4, 12)])
def test_unit_weights_membership_sums_and_the_walk_of_the_pi_count(nb, nf, edges, sort_axis):
    a, b = shape_scene(nb, False)
    r2, pe = scenes.radius_edges(nf, nb), EDGE_SETS[edges]
    for two in (True, False):
        cells, exp = scene_cells(nb, two), expected(nb, nf, False, edges, two)
        diagonal = cells[:, 3] != 0
        assert np.all(exp[5].sum(axis=(1, 2)) > 0) and np.any(exp[5].sum(axis=(0, 2)) == 0) == (nb > 1)  # every pi bin; the empty segment
        assert two or (exp[5][:, diagonal].sum() > 0 and exp[5][:, ~diagonal].sum() > 0)  # diagonal and off-diagonal cells hold pairs
        planes, stats, W_pi, stats_pi = count_shapes(a, b if two else a, cells, r2, pe, sort_axis, tie=True)
        assert np.array_equal(planes[3], exp[5]) and np.array_equal(exp[3], exp[5])  # W: the oracle's integers
        assert np.array_equal(planes[3], W_pi)  # ... and the pi count's on the same columns
        assert (stats.candidate_pairs, stats.evaluated_pairs) == (stats_pi.candidate_pairs, stats_pi.evaluated_pairs)  # same walk, same window
        worst = check_planes(planes, exp, two)
        print(f"nb={nb} nf={nf} {edges} axis={sort_axis} {'two handles' if two else 'one handle'}: worst |ours - oracle| / A = {worst:.3e}")


@pytest.mark.parametrize("sort_axis", [0, 2])
@pytest.mark.parametrize("edges", ["uniform4", "uneven"])
@pytest.mark.parametrize("nb", [1, 4])
def test_weighted_sums_match_the_oracle(nb, edges, sort_axis):
    a, b = shape_scene(nb, True)
    for two in (True, False):
        exp = expected(nb, 12, True, edges, two)
        planes, _ = count_shapes(a, b if two else a, scene_cells(nb, two), scenes.radius_edges(12, nb), EDGE_SETS[edges], sort_axis)
        worst = check_planes(planes, exp, two)
        np.testing.assert_allclose(planes[3], exp[3], rtol=RTOL_A, atol=0)
        print(f"weighted nb={nb} {edges} axis={sort_axis} {'two handles' if two else 'one handle'}: worst |ours - oracle| / A = {worst:.3e}")


def test_handles_of_different_shapes_and_sort_axes():
    """Neither equal patch counts, nor equal bin counts, nor one sort axis: the four bins of the first site of one handle
    against the one bin of the first patch of another, sorted along another axis -- the whole segment is streamed."""
    a, _ = shape_scene(4, False)
    _, b = shape_scene(1, False)
    sub = dict({key: b[key][:int(b["off"][1])] for key in ("x", "y", "z", "d", "c", "g1", "g2")}, w=None, nb=1, off=b["off"][:2].copy())
    cells = np.array([(k, 0, 0, 0) for k in range(8)], dtype=np.int32)  # segments (patch 0 | 1, bin k) of a, all on row 0
    r2 = scenes.radius_edges(12, 1)
    exp = oracle.proj_shape_cells(a, sub, cells, r2, UNEVEN)
    assert exp[5].sum() > 500 and np.all(exp[5].sum(axis=(1, 2)) > 0)
    windowed, st_windowed = count_shapes(a, sub, cells, r2, UNEVEN, 2, 2)
    whole, st_whole = count_shapes(a, sub, cells, r2, UNEVEN, 2, 0)
    assert st_whole.evaluated_pairs == st_whole.candidate_pairs >= st_windowed.evaluated_pairs
    for planes in (windowed, whole):
        assert np.array_equal(planes[3], exp[5])
        check_planes(planes, exp)


# --------------------------------------------------------------------------- 2. the diagonal rule
def test_a_diagonal_cell_is_half_the_full_cell_and_the_sides_swap():
    a, b = shape_scene(1, True)
    unit = dict(a, w=None)
    seg = {key: a[key][:int(a["off"][1])] for key in ("x", "y", "z", "w", "d", "c", "g1", "g2")}
    for weighted in (False, True):
        one = dict(seg, w=seg["w"] if weighted else None, nb=1, off=a["off"][:2].copy())
        copy = {key: (value.copy() if isinstance(value, np.ndarray) else value) for key, value in one.items()}
        r2 = scenes.radius_edges(12, 1)
        exp = oracle.proj_shape_cells(one, one, DIAGONAL, r2, UNIFORM_4)
        assert exp[5].sum() > 500 and r2[0, 0] > 0.0  # (an object meets its copy at R2 == 0, which no bin holds)
        half, st_half = count_shapes(one, one, DIAGONAL, r2, UNIFORM_4)
        full, st_full = count_shapes(one, copy, ACROSS, r2, UNIFORM_4)
        n = len(one["x"])
        assert (st_half.candidate_pairs, st_full.candidate_pairs) == (n * (n - 1) // 2, n * n)
        assert np.array_equal(full[3], 2.0 * half[3]) if not weighted else np.allclose(full[3], 2.0 * half[3], rtol=RTOL_A, atol=0)
        check_planes(half, exp, "diagonal")
        check_planes(full, exp, "full", factor=2.0)
    # an off-diagonal cell with the sides swapped: the same W exactly, the same sums within the tolerance
    cells = scenes.cells_two_handles(1)
    r2 = scenes.radius_edges(12, 1)
    exp = expected(1, 12, False, "uniform4", True)
    b_unit = dict(b, w=None)
    ab, _ = count_shapes(unit, b_unit, cells, r2, UNIFORM_4)
    ba, _ = count_shapes(b_unit, unit, cells[:, [1, 0, 2, 3]], r2, UNIFORM_4)
    assert np.array_equal(ab[3], ba[3]) and np.array_equal(ab[3], exp[5])
    check_planes(ab, exp, "a, b")
    check_planes(ba, exp, "b, a")


# --------------------------------------------------------------------------- 3. bitwise properties
def test_no_shear_gives_exact_zeros_and_a_turn_by_45_degrees_swaps_the_planes_bit_for_bit():
    a, b = shape_scene(4, True)
    cells, r2 = scenes.cells_two_handles(4), scenes.radius_edges(12, 4)
    turn = lambda h: dict(h, g1=-h["g2"], g2=h["g1"])  # noqa: E731  (g1, g2) -> (-g2, g1)
    still = lambda h: dict(h, g1=np.zeros_like(h["g1"]), g2=np.zeros_like(h["g2"]))  # noqa: E731
    (PP, XX, PX, W), _ = count_shapes(a, b, cells, r2, UNIFORM_4)
    assert min(np.count_nonzero(PP), np.count_nonzero(XX), np.count_nonzero(PX)) > 500
    for first, second in ((still(a), b), (a, still(b))):  # g = 0 on one side
        (PP0, XX0, PX0, W0), _ = count_shapes(first, second, cells, r2, UNIFORM_4)
        assert not PP0.any() and not XX0.any() and not PX0.any() and np.array_equal(W0, W)
    # the products and the one sum of each term are sign-symmetric, the order of the adds is the walk's
    (PPr, XXr, PXr, Wr), _ = count_shapes(turn(a), turn(b), cells, r2, UNIFORM_4)
    assert np.array_equal(PPr, XX) and np.array_equal(XXr, PP) and np.array_equal(PXr, -PX) and np.array_equal(Wr, W)
    again, _ = count_shapes(a, b, cells, r2, UNIFORM_4)
    assert all(np.array_equal(one, two) for one, two in zip(again, (PP, XX, PX, W)))  # two calls, the same bits
    # ... and on one handle with diagonal cells
    cells = scenes.cells_one_handle(4)
    (PP, XX, PX, W), _ = count_shapes(a, a, cells, r2, UNIFORM_4)
    turned = turn(a)
    (PPr, XXr, PXr, Wr), _ = count_shapes(turned, turned, cells, r2, UNIFORM_4)
    assert np.count_nonzero(PX) > 500
    assert np.array_equal(PPr, XX) and np.array_equal(XXr, PP) and np.array_equal(PXr, -PX) and np.array_equal(Wr, W)


# --------------------------------------------------------------------------- 4. the sign convention
def isolated_pairs(n_pairs=6, seed=17):
    """``n_pairs`` pairs of shapes at d = 1000, the partners 0.4 .. 3 apart in radius and the pairs 50 apart: one segment,
    (ra, dec) and a handle without shear, objects 2 k and 2 k + 1 a pair."""
    rng = np.random.default_rng(seed)
    ra, dec = np.empty(2 * n_pairs), np.empty(2 * n_pairs)
    for k in range(n_pairs):
        ra[2 * k], dec[2 * k] = 0.5 + 0.05 * k, -0.6 + 0.25 * k
        ra[2 * k + 1:2 * k + 2], dec[2 * k + 1:2 * k + 2] = ring_around(rng, ra[2 * k], dec[2 * k], 1, 4e-4, 3e-3)
    h = one_segment(np.array(radec_to_xyz(ra, dec)), 1000.0, 50.0, w=rng.uniform(0.5, 1.5, 2 * n_pairs))
    return ra, dec, h


def test_shapes_elongated_along_the_line_that_joins_them_have_positive_PP():
    ra, dec, h = isolated_pairs()
    partner = np.arange(len(ra)) ^ 1
    g1, g2 = tangential_pattern(ra, dec, ra[partner], dec[partner], -0.1)  # radial about the partner: the tangential pattern of amplitude -0.1
    r2 = np.array([[0.3**2, 3.5**2]])
    ww = (h["w"][0::2] * h["w"][1::2]).sum()
    bound = RTOL_A * ww * 0.2 * 0.2  # A <= sum w_a w_b (|g1| + |g2|)^2, and |g1| + |g2| <= 0.1 sqrt(2) < 0.2
    along = dict(h, g1=g1, g2=g2)
    assert oracle.proj_shape_cells(along, along, DIAGONAL, r2, ONE_BIN)[5].sum() == len(ra) // 2  # the pairs, and nothing between them
    (PP, XX, PX, W), _ = count_shapes(along, along, DIAGONAL, r2, ONE_BIN)
    assert abs(W.sum() - ww) <= 1e-14 * ww
    assert abs(PP.sum() - 0.01 * ww) <= bound and abs(XX.sum()) <= bound and abs(PX.sum()) <= bound
    turned = dict(h, g1=-g2, g2=g1)  # both by 45 degrees
    (PP, XX, PX, W), _ = count_shapes(turned, turned, DIAGONAL, r2, ONE_BIN)
    assert abs(XX.sum() - 0.01 * ww) <= bound and abs(PP.sum()) <= bound and abs(PX.sum()) <= bound
    flip = np.where(np.arange(len(ra)) % 2 == 0, -1.0, 1.0)  # one of the two by 90 degrees
    across = dict(h, g1=flip * g1, g2=flip * g2)
    (PP, XX, PX, W), _ = count_shapes(across, across, DIAGONAL, r2, ONE_BIN)
    assert abs(PP.sum() + 0.01 * ww) <= bound and abs(XX.sum()) <= bound and abs(PX.sum()) <= bound
    print(f"isolated pairs: PP / W = {PP.sum() / W.sum():+.15f} with one of the two turned by 90 degrees")


# --------------------------------------------------------------------------- 5. long segments
@pytest.mark.parametrize("n_a, n_b", [(600, 600), (600, 300), (300, 600)])
def test_long_segments_on_either_side(n_a, n_b):
    """600 objects in one segment: three stages with a ragged last one (streamed), two full lane tiles and a padded one (in the
    lanes); ``d`` alternates by a factor 7 along the sort key, so the window follows the nearest object."""
    rng = np.random.default_rng(70 + n_a // 100 + n_b // 300)
    a, b = with_shear(long_segment(rng, n_a, 2), 8), with_shear(long_segment(rng, n_b, 2), 9)
    exp = oracle.proj_shape_cells(a, b, ACROSS, R2_LONG, UNIFORM_4)
    assert np.all(exp[5].sum(axis=(1, 2)) > 0) and np.count_nonzero(exp[5]) > 40
    planes, stats, W_pi, stats_pi = count_shapes(a, b, ACROSS, R2_LONG, UNIFORM_4, tie=True)
    assert np.array_equal(planes[3], exp[5]) and np.array_equal(planes[3], W_pi) and stats.candidate_pairs == n_a * n_b
    assert stats.evaluated_pairs == stats_pi.evaluated_pairs < stats.candidate_pairs
    check_planes(planes, exp)


@pytest.mark.parametrize("sort_axis", [0, 2])
def test_a_diagonal_cell_over_one_long_segment(sort_axis):
    """600 objects in ONE segment against itself: the first stage of every tile starts behind the tile's first lane and holds
    indices <= some lanes', which the index test drops; the evaluated pairs are the pi count's (``kept_work``)."""
    h = with_shear(long_segment(np.random.default_rng(5 + sort_axis), 600, sort_axis), 10)
    exp = oracle.proj_shape_cells(h, h, DIAGONAL, R2_LONG, UNIFORM_4)
    assert np.all(exp[5].sum(axis=(1, 2)) > 0) and np.count_nonzero(exp[5]) > 40
    planes, stats, W_pi, stats_pi = count_shapes(h, h, DIAGONAL, R2_LONG, UNIFORM_4, sort_axis, tie=True)
    assert np.array_equal(planes[3], exp[5]) and np.array_equal(planes[3], W_pi) and stats.candidate_pairs == 600 * 599 // 2
    assert stats.evaluated_pairs == stats_pi.evaluated_pairs <= stats.candidate_pairs  # (never more than the unordered pairs)
    check_planes(planes, exp)


# --------------------------------------------------------------------------- 6. edge cases
def test_empty_handles_a_single_object_the_pole_and_a_shared_position():
    rng = np.random.default_rng(31)
    r2 = np.array([[0.0, 1.0, 4.5**2]])  # from 0: only R2 == 0 itself is below the first bin
    some = with_shear(one_segment(box_xyz(rng, 40), 1000.0, rng.uniform(0.0, 60.0, 40)), 1)
    none = with_shear(one_segment(np.empty((3, 0)), 1000.0, 0.0), 1)
    one = with_shear(one_segment(np.array(radec_to_xyz(np.array([40.2 * np.pi / 180]), np.array([30.2 * np.pi / 180]))), 1000.0, 30.0), 2)
    for a, b in ((none, some), (some, none), (none, dict(none))):  # n = 0 on either side
        planes, stats = count_shapes(a, b, ACROSS, r2, UNIFORM_4)
        assert not any(p.any() for p in planes) and stats.candidate_pairs == 0 and stats.evaluated_pairs == 0
    for a, b in ((one, some), (some, one)):  # a one-object segment
        exp = oracle.proj_shape_cells(a, b, ACROSS, r2, UNIFORM_4)
        planes, stats = count_shapes(a, b, ACROSS, r2, UNIFORM_4)
        assert exp[5].sum() > 5 and np.array_equal(planes[3], exp[5]) and stats.candidate_pairs == 40
        check_planes(planes, exp)
    for h in (one, none):  # a one-object diagonal cell, and an empty one: all zero
        planes, stats = count_shapes(h, h, DIAGONAL, r2, UNIFORM_4)
        assert not any(p.any() for p in planes) and stats.candidate_pairs == 0 and stats.evaluated_pairs == 0
    # the pole guards: a shape ON the pole of the frame (its den == 0 for every partner) adds to W only, at either end
    ra, dec = ring_around(rng, 0.0, np.pi / 2, 50, 5e-4, 3e-3)
    around = with_shear(one_segment(np.array(radec_to_xyz(ra, dec)), 1000.0, 30.0), 4)
    pole = dict(one_segment(np.array([[0.0], [0.0], [1.0]]), 1000.0, 30.0), g1=np.array([0.3]), g2=np.array([-0.2]))
    off_pole = dict(pole, x=np.array([1e-9]))  # next to it the rotation is defined
    for a, b in ((around, pole), (pole, around)):
        (PP, XX, PX, W), _ = count_shapes(a, b, ACROSS, r2, ONE_BIN)
        assert W.sum() == 50 and not PP.any() and not XX.any() and not PX.any()
    for a, b in ((around, off_pole), (off_pole, around)):
        (PP, XX, PX, W), _ = count_shapes(a, b, ACROSS, r2, ONE_BIN)
        assert W.sum() == 50 and PP.any() and XX.any() and PX.any()
    # two objects at one position: R2 == 0, in no bin -- in a diagonal cell, and against a copy of the segment
    twice = {key: (np.concatenate([value, value[:1]]) if isinstance(value, np.ndarray) and key != "off" else value) for key, value in some.items()}
    twice["off"] = np.array([0, 41], dtype=np.int64)
    twice["c"][40] += 1.0  # (a partner of the others in its own right)
    exp = oracle.proj_shape_cells(twice, twice, DIAGONAL, r2, np.array([0.0, np.inf]))
    planes, stats = count_shapes(twice, twice, DIAGONAL, r2, np.array([0.0, np.inf]))
    assert stats.candidate_pairs == 41 * 40 // 2 and np.array_equal(planes[3], exp[5]) and 100 < exp[5].sum() <= 41 * 40 // 2 - 1
    check_planes(planes, exp)
    copy = {key: (value.copy() if isinstance(value, np.ndarray) else value) for key, value in some.items()}
    planes, stats = count_shapes(some, copy, ACROSS, r2, np.array([0.0, np.inf]))
    in_range = oracle.proj_shape_cells(some, some, DIAGONAL, r2, np.array([0.0, np.inf]))[5]
    assert stats.candidate_pairs == 1600 and planes[3].sum() == 2 * in_range.sum() <= 40 * 39 and in_range.sum() > 100


# --------------------------------------------------------------------------- 7. refusals
def test_wrong_kinds_cells_the_cap_and_the_reach_are_refused():
    ctx = engine.get_context(0)
    a_h, b_h = shape_scene(4, False)
    n_patches = 2 * len(scenes.SITES)
    cells, r2, pe = scenes.cells_two_handles(4), scenes.radius_edges(1, 4), UNIFORM_4
    a, b, plain = upload_shapes(ctx, a_h), upload_shapes(ctx, b_h), upload(ctx, a_h)
    others = [_lib.DsigmaLenses(ctx, a_h["x"], a_h["y"], a_h["z"], None, a_h["d"], a_h["c"], n_patches, 4, a_h["off"]),
              _lib.ShearSources(ctx, a_h["x"], a_h["y"], a_h["z"], None, a_h["d"], a_h["c"], n_patches, a_h["off"], n_bins=4)]
    try:
        # a projected, lens or source handle in either slot
        for wrong in (plain, *others):
            for first, second in ((wrong, b), (a, wrong)):
                with pytest.raises(_lib.YawhipError, match="a handle is not one of yawhip_proj_upload_shapes") as refusal:
                    _lib.proj_count_shapes(ctx, first, second, cells, r2, pe)
                assert "(status -5)" in str(refusal.value)  # YAWHIP_ERR_MISMATCH
        # the shape handle is still refused by the other counts
        empty_cells, empty_jobs = np.empty((0, 4), dtype=np.int32), np.empty((0, 2), dtype=np.int32)
        for call in (lambda: _lib.proj_count(ctx, a, b, empty_cells, r2, 40.0), lambda: _lib.proj_count_pi(ctx, a, a, empty_cells, r2, pe),
                     lambda: _lib.proj_count_smu(ctx, a, b, empty_cells, r2, np.array([0.0, 1.0])),
                     lambda: _lib.proj_count_shear(ctx, a, b, empty_cells, r2, pe), lambda: _lib.shear_auto_count(ctx, a, empty_jobs, r2),
                     lambda: _lib.shear_pair_count(ctx, a, b, np.empty((0, 5), dtype=np.int32), r2),
                     lambda: _lib.dsigma_count(ctx, a, b, empty_jobs, r2), lambda: _lib.dsigma_count_radial(ctx, a, b, empty_jobs, r2)):
            with pytest.raises(_lib.YawhipError) as refusal:
                call()
            assert "(status -5)" in str(refusal.value)
        # a wrong diagonal flag: set between two handles, set off the diagonal of one, missing on it
        own = scenes.cells_one_handle(4)
        for first, second, table, row in ((a, b, cells, 3), (a, a, own, len(own) - 1), (a, a, own, 0)):
            flagged = table.copy()
            flagged[row, 3] ^= 1
            with pytest.raises(_lib.YawhipError, match="diagonal") as refusal:
                _lib.proj_count_shapes(ctx, first, second, flagged, r2, pe)
            assert "(status -1)" in str(refusal.value)  # YAWHIP_ERR_INVALID
        # the pi edges and the reach: yawhip_proj_count_pi's
        with pytest.raises(_lib.YawhipError, match="first pi edge must be 0"):
            _lib.proj_count_shapes(ctx, a, b, cells, r2, np.array([1.0, 40.0]))
        with pytest.raises(_lib.YawhipError, match="strictly ascending"):
            _lib.proj_count_shapes(ctx, a, b, cells, r2, np.array([0.0, 20.0, 20.0]))
        with pytest.raises(_lib.YawhipError, match="an object is too close for the largest radius"):
            _lib.proj_count_shapes(ctx, a, b, cells, np.array([[0.0, 100.0**2]] * 4), pe)
        # not even one pi bin fits above 241 edges
        with pytest.raises(_lib.YawhipError, match="do not fit the LDS of a workgroup: not even 1 pi bin at n_edges=256, at most n_edges=241 at 1 pi bin") as refusal:
            _lib.proj_count_shapes(ctx, a, b, cells, scenes.radius_edges(255, 4), ONE_BIN)
        assert "(status -1)" in str(refusal.value)
        planes, _ = _lib.proj_count_shapes(ctx, a, b, np.empty((0, 4), dtype=np.int32), r2, pe)  # nothing to do
        assert all(p.shape == (4, 0, 1) for p in planes)
    finally:
        for handle in (a, b, plain, *others):
            handle.free()


@pytest.mark.parametrize("n_edges", sorted(CAPS))
def test_the_largest_n_pi_that_fits_runs_and_one_more_is_refused(n_edges):
    cap = CAPS[n_edges]
    a, b = shape_scene(1, False)
    cells, r2 = scenes.cells_two_handles(1), scenes.radius_edges(n_edges - 1, 1)
    pe = np.linspace(0.0, scenes.PMAX, cap + 1)
    exp = oracle.proj_shape_cells(a, b, cells, r2, pe)
    planes, _ = count_shapes(a, b, cells, r2, pe)
    assert np.all(exp[5].sum(axis=(1, 2)) > 0) and np.array_equal(planes[3], exp[5])
    check_planes(planes, exp)
    ctx = engine.get_context(0)
    made = [upload_shapes(ctx, a), upload_shapes(ctx, b)]
    try:
        with pytest.raises(_lib.YawhipError, match=f"do not fit the LDS of a workgroup: at most {cap} pi bins at n_edges={n_edges}"):
            _lib.proj_count_shapes(ctx, *made, cells, r2, np.linspace(0.0, scenes.PMAX, cap + 2))
    finally:
        for handle in made:
            handle.free()


# --------------------------------------------------------------------------- 8. the driver on the device
def test_the_driver_on_the_device_and_its_resident_handles(monkeypatch):
    """Eight patches, two redshift bins, shape randoms: the driver through the real library against the brute force of
    tests/test_shape_shape_host.py. The shape handle is the one a preceding ``crosscorrelate_alignment`` on the same catalogue
    left on the device, and a second call uploads nothing."""
    import test_alignment_host as align
    import test_shape_shape_host as host
    import yet_another_wizz_amd as yaw

    centres = tuple((0.30 + 0.0025 * i, 0.10 + 0.0025 * j) for j in range(2) for i in range(4))
    cols = dict(shapes=align.columns(3, 40, shear=True, centres=centres), shape_rand=align.columns(11, 50, weighted=False, centres=centres))
    cats = {name: align.catalog(c, centres) for name, c in cols.items()}
    density, density_rand = (align.catalog(align.columns(seed, n, centres=centres), centres) for seed, n in ((5, 35), (7, 60)))
    uploads = []
    for kind in ("ProjHandle", "ProjShapesHandle"):
        made = getattr(_lib, kind)
        monkeypatch.setattr(_lib, kind, lambda *args, made=made, kind=kind, **kwargs: uploads.append(kind) or made(*args, **kwargs))
    yaw.crosscorrelate_alignment(align.config(), cats["shapes"], density, density_rand, pi_max=align.PI_MAX, pi_bins=align.PI_EDGES)
    assert sorted(uploads) == ["ProjHandle", "ProjHandle", "ProjShapesHandle"]  # w_g+ uploads the shapes once ...
    first = host.check_driver(cols, centres, cats)
    assert uploads[3:] == ["ProjHandle"]  # ... and w_++ finds them there: only the shape randoms are new
    second = host.check_driver(cols, centres, cats)
    assert len(uploads) == 4 and first == second  # the handles are reused, and the counts are the same bits
    for cat in (*cats.values(), density, density_rand):
        cat.drop_layouts()
