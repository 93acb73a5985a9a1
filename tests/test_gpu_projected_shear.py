"""GPU: the projected position-shape count (``yawhip_proj_count_shear``) and ``crosscorrelate_alignment`` on the device,
against the numpy brute force of tests/proj_shear_oracle.py, on the scenes of tests/proj_scenes.py with seeded ``g1``,
``g2`` on the second handle, and against ``yawhip_proj_count_pi`` on the shapes' ``(x, y, z, w, d, c)``.

Membership is tested EXACTLY: with unit weights ``W`` is the integer number of pairs per pi bin, cell and fine bin and must
equal the oracle's with ``np.array_equal``. ``T`` and ``X`` are held to ``|ours - oracle| <= 1e-10 A`` per pi bin, cell and fine
bin, ``A = sum |w_a w_b| (|g1| + |g2|)`` over its member pairs: the project's rule for a signed sum."""
import functools

import numpy as np
import pytest

import proj_pi_oracle
import proj_scenes as scenes
import proj_shear_oracle as oracle
from proj_pi_oracle import UNEVEN, UNIFORM_4
from shear_oracle import tangential_pattern
from test_gpu_projected import ACROSS, box_xyz, long_segment, one_segment, scene, upload
from test_shear_host import ring_around
from yet_another_wizz_amd import _lib, engine
from yet_another_wizz_amd.catalog import radec_to_xyz

pytestmark = pytest.mark.gpu
RTOL_A = 1e-10  # the project's tolerance of a signed sum, relative to its cancellation-free magnitude A
ONE_BIN = np.array([0.0, scenes.PMAX])
EDGE_SETS = {"one": ONE_BIN, "uniform4": UNIFORM_4, "uneven": UNEVEN}
CAPS = {13: 35, 51: 8, 256: 1}  # include/yawhip.h: the largest n_pi whose carve-up fits 64 KiB of LDS


def with_shear(h, seed):
    """The oracle's shape handle: ``h`` with seeded ``g1``, ``g2``."""
    rng = np.random.default_rng(seed)
    n = len(h["x"])
    return dict(h, g1=rng.normal(0.01, 0.05, n), g2=rng.normal(-0.02, 0.05, n))


def upload_shapes(ctx, h, sort_axis=2):
    n_patches = (len(h["off"]) - 1) // h["nb"]
    return _lib.ProjShapesHandle(ctx, h["x"], h["y"], h["z"], h["w"], h["g1"], h["g2"], h["d"], h["c"], n_patches, h["nb"], h["off"],
                                 sort_axis=sort_axis)


def count_shear(dens, shapes, cells, r2, pe, axis_d=2, axis_s=None, tie=False):
    """``yawhip_proj_count_shear`` of the oracle's handles -> ((T, X, W), CountStats); ``tie``: also ``yawhip_proj_count_pi`` on
    the same density handle and the shapes' columns as a plain projected handle -> (..., W_pi, CountStats_pi)."""
    ctx = engine.get_context(0)
    made = [upload(ctx, dens, axis_d), upload_shapes(ctx, shapes, axis_d if axis_s is None else axis_s)]
    try:
        planes, stats = _lib.proj_count_shear(ctx, made[0], made[1], cells, r2, pe)
        extra = ()
        if tie:
            made.append(upload(ctx, shapes, axis_d if axis_s is None else axis_s))
            extra = _lib.proj_count_pi(ctx, made[0], made[2], cells, r2, pe)
    finally:
        for handle in made:
            handle.free()
    assert len(planes) == 3 and all(p.shape == (len(pe) - 1, len(cells), np.shape(r2)[1] - 1) for p in planes)
    assert stats.n_workgroups == len(cells) and stats.evaluated_pairs <= stats.candidate_pairs
    return (planes, stats, *extra)


@functools.lru_cache(maxsize=None)
def shape_scene(nb, weighted):
    a, b = scene(nb, weighted)
    return a, with_shear(b, 100 + nb)


@functools.lru_cache(maxsize=None)
def expected(nb, nf, weighted, edges):
    """The oracle's (T, X, W, A, N) of the scene: computed once per case, shared, never modified."""
    dens, shapes = shape_scene(nb, weighted)
    out = oracle.proj_shear_cells(dens, shapes, scenes.cells_two_handles(nb), scenes.radius_edges(nf, nb), EDGE_SETS[edges])
    for arr in out:
        arr.setflags(write=False)
    return out


def check_planes(got, exp, label=""):
    """T, X under the rule, cells without pairs exactly 0; returns the worst ``|ours - oracle| / A``."""
    (T, X, W), (exp_t, exp_x, _, exp_a, exp_n) = got, exp
    worst = 0.0
    for name, ours, theirs in (("T", T, exp_t), ("X", X, exp_x)):
        assert np.all(ours[exp_n == 0] == 0.0), (label, name)
        assert np.all(np.abs(ours - theirs) <= RTOL_A * exp_a), (label, name)
        if np.any(exp_a > 0):
            worst = max(worst, float(np.max(np.abs(ours - theirs)[exp_a > 0] / exp_a[exp_a > 0])))
    assert np.all(W[exp_n == 0] == 0.0), label
    return worst


# --------------------------------------------------------------------------- 1. against the oracle, and the tie to the pi count
@pytest.mark.parametrize("sort_axis", [0, 1, 2])
@pytest.mark.parametrize("edges", list(EDGE_SETS))
@pytest.mark.parametrize("nb, nf", [(1, 1), (1, 50), (4, 12)])
def test_unit_weights_membership_sums_and_the_walk_of_the_pi_count(nb, nf, edges, sort_axis):
    dens, shapes = shape_scene(nb, False)
    cells, r2, pe = scenes.cells_two_handles(nb), scenes.radius_edges(nf, nb), EDGE_SETS[edges]
    exp = expected(nb, nf, False, edges)
    assert np.all(exp[4].sum(axis=(1, 2)) > 0) and np.any(exp[4].sum(axis=(0, 2)) == 0) == (nb > 1)  # every pi bin; the empty segment
    planes, stats, W_pi, stats_pi = count_shear(dens, shapes, cells, r2, pe, sort_axis, tie=True)
    assert np.array_equal(planes[2], exp[4]) and np.array_equal(exp[2], exp[4])  # W: the oracle's integers
    assert np.array_equal(planes[2], W_pi)  # ... and the pi count's on the same columns
    assert (stats.candidate_pairs, stats.evaluated_pairs) == (stats_pi.candidate_pairs, stats_pi.evaluated_pairs)  # same walk, same window
    worst = check_planes(planes, exp)
    print(f"nb={nb} nf={nf} {edges} axis={sort_axis}: worst |ours - oracle| / A = {worst:.3e}")


@pytest.mark.parametrize("sort_axis", [0, 2])
@pytest.mark.parametrize("edges", ["uniform4", "uneven"])
@pytest.mark.parametrize("nb", [1, 4])
def test_weighted_sums_match_the_oracle(nb, edges, sort_axis):
    dens, shapes = shape_scene(nb, True)
    exp = expected(nb, 12, True, edges)
    planes, _ = count_shear(dens, shapes, scenes.cells_two_handles(nb), scenes.radius_edges(12, nb), EDGE_SETS[edges], sort_axis)
    worst = check_planes(planes, exp)
    np.testing.assert_allclose(planes[2], exp[2], rtol=RTOL_A, atol=0)
    print(f"weighted nb={nb} {edges} axis={sort_axis}: worst |ours - oracle| / A = {worst:.3e}")


def test_different_sort_axes_stream_the_whole_segment():
    dens, shapes = shape_scene(4, False)
    cells, r2 = scenes.cells_two_handles(4), scenes.radius_edges(12, 4)
    windowed, st_windowed = count_shear(dens, shapes, cells, r2, UNEVEN, 2, 2)
    whole, st_whole = count_shear(dens, shapes, cells, r2, UNEVEN, 2, 0)
    assert st_whole.evaluated_pairs == st_whole.candidate_pairs >= st_windowed.evaluated_pairs
    assert np.array_equal(whole[2], windowed[2]) and np.array_equal(whole[2], expected(4, 12, False, "uneven")[4])
    check_planes(whole, expected(4, 12, False, "uneven"))


# --------------------------------------------------------------------------- 2. bitwise properties
def test_no_shear_gives_exact_zeros_and_a_turn_by_45_degrees_swaps_the_planes_bit_for_bit():
    dens, shapes = shape_scene(4, True)
    cells, r2 = scenes.cells_two_handles(4), scenes.radius_edges(12, 4)
    (T, X, W), _ = count_shear(dens, shapes, cells, r2, UNIFORM_4)
    assert np.count_nonzero(T) > 500 and np.count_nonzero(X) > 500
    zero = np.zeros_like(shapes["g1"])
    (T0, X0, W0), _ = count_shear(dens, dict(shapes, g1=zero, g2=zero), cells, r2, UNIFORM_4)
    assert not T0.any() and not X0.any() and np.array_equal(W0, W)
    # (g1, g2) -> (-g2, g1): the products and the one sum of each term are sign-symmetric, the order of the adds is the walk's
    (Tr, Xr, Wr), _ = count_shear(dens, dict(shapes, g1=-shapes["g2"], g2=shapes["g1"]), cells, r2, UNIFORM_4)
    assert np.array_equal(Tr, -X) and np.array_equal(Xr, T) and np.array_equal(Wr, W)
    again, _ = count_shear(dens, shapes, cells, r2, UNIFORM_4)
    assert all(np.array_equal(one, two) for one, two in zip(again, (T, X, W)))  # two calls, the same bits


# --------------------------------------------------------------------------- 3. the sign convention
def test_shapes_that_point_at_the_density_object_have_negative_T():
    """One density object, a ring of 400 shapes of ellipticity 0.1 elongated TOWARDS it: the tangential ellipticity is -0.1,
    so ``-T / W = 0.1`` (the sign of ``w_g+``) and ``X / W = 0``."""
    rng = np.random.default_rng(3)
    ra_c, dec_c = 0.9, 0.4
    ra, dec = ring_around(rng, ra_c, dec_c, 400, 3e-4, 3e-3)
    g1, g2 = tangential_pattern(ra, dec, ra_c, dec_c, -0.1)  # radial: the tangential pattern of amplitude -0.1
    dens = one_segment(np.array(radec_to_xyz(np.array([ra_c]), np.array([dec_c]))), 1000.0, 50.0)
    shapes = dict(one_segment(np.array(radec_to_xyz(ra, dec)), 1000.0, rng.uniform(30.0, 70.0, 400), w=rng.uniform(0.5, 1.5, 400)), g1=g1, g2=g2)
    r2 = np.array([np.geomspace(0.25, 3.5, 5)]) ** 2
    exp = oracle.proj_shear_cells(dens, shapes, ACROSS, r2, ONE_BIN)
    (T, X, W), _ = count_shear(dens, shapes, ACROSS, r2, ONE_BIN)
    assert np.all(exp[4] > 20) and exp[4].sum() == 400
    assert np.all(np.abs(-T - 0.1 * W) <= RTOL_A * exp[3]) and np.all(np.abs(X) <= RTOL_A * exp[3]) and np.all(T < 0)
    print(f"ring: worst |-T / W - 0.1| = {np.max(np.abs(-T / W - 0.1)):.3e}, worst |X / W| = {np.max(np.abs(X / W)):.3e}")


# --------------------------------------------------------------------------- 4. long segments
R2_LONG = np.array([np.geomspace(0.1, 4.0, 13)]) ** 2


@pytest.mark.parametrize("n_dens, n_shapes", [(600, 600), (600, 300), (300, 600)])
def test_long_segments_on_either_side(n_dens, n_shapes):
    """600 objects in one segment: three stages with a ragged last one (streamed), two full lane tiles and a padded one (in the
    lanes); ``d`` alternates by a factor 7 along the sort key, so the window follows the nearest object."""
    rng = np.random.default_rng(70 + n_dens // 100 + n_shapes // 300)
    dens, shapes = long_segment(rng, n_dens, 2), with_shear(long_segment(rng, n_shapes, 2), 9)
    exp = oracle.proj_shear_cells(dens, shapes, ACROSS, R2_LONG, UNIFORM_4)
    assert np.all(exp[4].sum(axis=(1, 2)) > 0) and np.count_nonzero(exp[4]) > 40
    planes, stats, W_pi, stats_pi = count_shear(dens, shapes, ACROSS, R2_LONG, UNIFORM_4, tie=True)
    assert np.array_equal(planes[2], exp[4]) and np.array_equal(planes[2], W_pi) and stats.candidate_pairs == n_dens * n_shapes
    assert stats.evaluated_pairs == stats_pi.evaluated_pairs < stats.candidate_pairs
    check_planes(planes, exp)


# --------------------------------------------------------------------------- 5. edge cases
def test_empty_handles_a_single_object_the_pole_and_a_shared_position():
    rng = np.random.default_rng(31)
    r2 = np.array([[0.0, 1.0, 4.5**2]])  # from 0: only R2 == 0 itself is below the first bin
    some = one_segment(box_xyz(rng, 40), 1000.0, rng.uniform(0.0, 60.0, 40))
    none = one_segment(np.empty((3, 0)), 1000.0, 0.0)
    one = one_segment(np.array(radec_to_xyz(np.array([40.2 * np.pi / 180]), np.array([30.2 * np.pi / 180]))), 1000.0, 30.0)
    for dens, shapes in ((none, some), (some, none), (none, none)):  # n = 0 on either side
        planes, stats = count_shear(dens, with_shear(shapes, 1), ACROSS, r2, UNIFORM_4)
        assert not any(p.any() for p in planes) and stats.candidate_pairs == 0 and stats.evaluated_pairs == 0
    for dens, shapes in ((one, some), (some, one)):  # a one-object segment
        shapes = with_shear(shapes, 2)
        exp = oracle.proj_shear_cells(dens, shapes, ACROSS, r2, UNIFORM_4)
        planes, stats = count_shear(dens, shapes, ACROSS, r2, UNIFORM_4)
        assert exp[4].sum() > 5 and np.array_equal(planes[2], exp[4]) and stats.candidate_pairs == 40
        check_planes(planes, exp)
    # the pole guard: a shape ON the pole of the frame (den == 0 for every partner) adds to W only
    ra, dec = ring_around(rng, 0.0, np.pi / 2, 50, 5e-4, 3e-3)
    around = one_segment(np.array(radec_to_xyz(ra, dec)), 1000.0, 30.0)
    pole = dict(one_segment(np.array([[0.0], [0.0], [1.0]]), 1000.0, 30.0), g1=np.array([0.3]), g2=np.array([-0.2]))
    (T, X, W), _ = count_shear(around, pole, ACROSS, r2, ONE_BIN)
    assert W.sum() == 50 and not T.any() and not X.any()
    off_pole = dict(pole, x=np.array([1e-9]))  # next to it the rotation is defined
    (T, X, W), _ = count_shear(around, off_pole, ACROSS, r2, ONE_BIN)
    assert W.sum() == 50 and T.any() and X.any()
    # one sample on both sides: an object meets itself at R2 == 0, which is in no bin, and every other object once
    both = with_shear(some, 3)
    exp = oracle.proj_shear_cells(some, both, ACROSS, r2, np.array([0.0, np.inf]))
    planes, stats = count_shear(some, both, ACROSS, r2, np.array([0.0, np.inf]))
    assert stats.candidate_pairs == 1600 and np.array_equal(planes[2], exp[4])
    in_range = proj_pi_oracle.proj_pi_cells(some, some, np.array([[0, 0, 0, 1]]), r2, np.array([0.0, np.inf]))[2]
    assert planes[2].sum() == 2 * in_range.sum() <= 40 * 39 and in_range.sum() > 100
    check_planes(planes, exp)


# --------------------------------------------------------------------------- 6. refusals
def test_wrong_kinds_cells_the_cap_and_the_reach_are_refused():
    ctx = engine.get_context(0)
    dens_h, shapes_h = shape_scene(4, False)
    n_patches = 2 * len(scenes.SITES)
    cells, r2, pe = scenes.cells_two_handles(4), scenes.radius_edges(1, 4), UNIFORM_4
    dens, shapes = upload(ctx, dens_h), upload_shapes(ctx, shapes_h)
    a = dens_h
    others = [_lib.DsigmaLenses(ctx, a["x"], a["y"], a["z"], None, a["d"], a["c"], n_patches, 4, a["off"]),
              _lib.ShearSources(ctx, a["x"], a["y"], a["z"], None, a["d"], a["c"], n_patches, a["off"], n_bins=4)]
    try:
        # either handle of the wrong kind
        for first, second, what in ((shapes, shapes, "density handle is not one of yawhip_proj_upload"),
                                    (dens, dens, "shape handle is not one of yawhip_proj_upload_shapes"),
                                    (others[0], shapes, "density handle"), (others[1], shapes, "density handle"),
                                    (dens, others[0], "shape handle"), (dens, others[1], "shape handle")):
            with pytest.raises(_lib.YawhipError, match=what) as refusal:
                _lib.proj_count_shear(ctx, first, second, cells, r2, pe)
            assert "(status -5)" in str(refusal.value)  # YAWHIP_ERR_MISMATCH
        # the new kind given to the other counts
        empty_cells, empty_jobs = np.empty((0, 4), dtype=np.int32), np.empty((0, 2), dtype=np.int32)
        for call in (lambda: _lib.proj_count(ctx, dens, shapes, empty_cells, r2, 40.0), lambda: _lib.proj_count(ctx, shapes, dens, empty_cells, r2, 40.0),
                     lambda: _lib.proj_count_pi(ctx, dens, shapes, empty_cells, r2, pe), lambda: _lib.proj_count_pi(ctx, shapes, shapes, empty_cells, r2, pe),
                     lambda: _lib.proj_count_smu(ctx, dens, shapes, empty_cells, r2, np.array([0.0, 1.0])),
                     lambda: _lib.proj_count_smu(ctx, shapes, dens, empty_cells, r2, np.array([0.0, 1.0])),
                     lambda: _lib.shear_auto_count(ctx, shapes, empty_jobs, r2),
                     lambda: _lib.shear_pair_count(ctx, shapes, others[1], np.empty((0, 5), dtype=np.int32), r2),
                     lambda: _lib.shear_pair_count(ctx, others[1], shapes, np.empty((0, 5), dtype=np.int32), r2),
                     lambda: _lib.dsigma_count(ctx, others[0], shapes, empty_jobs, r2), lambda: _lib.dsigma_count(ctx, shapes, shapes, empty_jobs, r2),
                     lambda: _lib.dsigma_count_radial(ctx, shapes, shapes, empty_jobs, r2)):
            with pytest.raises(_lib.YawhipError) as refusal:
                call()
            assert "(status -5)" in str(refusal.value)
        # a diagonal flag
        flagged = cells.copy()
        flagged[3, 3] = 1
        with pytest.raises(_lib.YawhipError, match="diagonal") as refusal:
            _lib.proj_count_shear(ctx, dens, shapes, flagged, r2, pe)
        assert "(status -1)" in str(refusal.value)  # YAWHIP_ERR_INVALID
        # the pi edges and the reach: yawhip_proj_count_pi's
        with pytest.raises(_lib.YawhipError, match="first pi edge must be 0"):
            _lib.proj_count_shear(ctx, dens, shapes, cells, r2, np.array([1.0, 40.0]))
        with pytest.raises(_lib.YawhipError, match="strictly ascending"):
            _lib.proj_count_shear(ctx, dens, shapes, cells, r2, np.array([0.0, 20.0, 20.0]))
        with pytest.raises(_lib.YawhipError, match="an object is too close for the largest radius"):
            _lib.proj_count_shear(ctx, dens, shapes, cells, np.array([[0.0, 100.0**2]] * 4), pe)
        planes, _ = _lib.proj_count_shear(ctx, dens, shapes, np.empty((0, 4), dtype=np.int32), r2, pe)  # nothing to do
        assert all(p.shape == (4, 0, 1) for p in planes)
    finally:
        for handle in (dens, shapes, *others):
            handle.free()
    for bad in (dict(g1=np.where(np.arange(len(a["x"])) == 3, np.nan, 0.0)), dict(g2=np.where(np.arange(len(a["x"])) == 3, np.inf, 0.0)),
                dict(d=np.where(np.arange(len(a["x"])) == 3, 0.0, a["d"])), dict(c=np.where(np.arange(len(a["x"])) == 3, np.nan, a["c"]))):
        with pytest.raises(_lib.YawhipError, match=f"column {next(iter(bad))} has an entry"):
            upload_shapes(ctx, dict(shapes_h, **bad))


@pytest.mark.parametrize("n_edges", sorted(CAPS))
def test_the_largest_n_pi_that_fits_runs_and_one_more_is_refused(n_edges):
    cap = CAPS[n_edges]
    dens, shapes = shape_scene(1, False)
    cells, r2 = scenes.cells_two_handles(1), scenes.radius_edges(n_edges - 1, 1)
    pe = np.linspace(0.0, scenes.PMAX, cap + 1)
    exp = oracle.proj_shear_cells(dens, shapes, cells, r2, pe)
    planes, _ = count_shear(dens, shapes, cells, r2, pe)
    assert np.all(exp[4].sum(axis=(1, 2)) > 0) and np.array_equal(planes[2], exp[4])
    check_planes(planes, exp)
    ctx = engine.get_context(0)
    made = [upload(ctx, dens), upload_shapes(ctx, shapes)]
    try:
        with pytest.raises(_lib.YawhipError, match=f"do not fit the LDS of a workgroup: at most {cap} pi bins at n_edges={n_edges}"):
            _lib.proj_count_shear(ctx, *made, cells, r2, np.linspace(0.0, scenes.PMAX, cap + 2))
    finally:
        for handle in made:
            handle.free()


# --------------------------------------------------------------------------- 7. the driver on the device
def test_the_driver_on_the_device_and_its_resident_handles(monkeypatch):
    """Eight patches, two redshift bins, shape randoms: the driver through the real library against the brute force of
    tests/test_alignment_host.py; a second call uploads nothing."""
    import test_alignment_host as host

    centres = tuple((0.30 + 0.0025 * i, 0.10 + 0.0025 * j) for j in range(2) for i in range(4))
    cols = dict(shapes=host.columns(3, 40, shear=True, centres=centres), density=host.columns(5, 35, centres=centres),
                density_rand=host.columns(7, 60, weighted=False, centres=centres), shape_rand=host.columns(11, 50, weighted=False, centres=centres))
    cats = {name: host.catalog(c, centres) for name, c in cols.items()}
    first = host.check_driver(cols, centres, cats)
    uploads = []
    for kind in ("ProjHandle", "ProjShapesHandle"):
        made = getattr(_lib, kind)
        monkeypatch.setattr(_lib, kind, lambda *args, made=made, **kwargs: uploads.append(made) or made(*args, **kwargs))
    second = host.check_driver(cols, centres, cats)
    assert uploads == [] and first == second  # the handles are reused, and the counts are the same bits
    for cat in cats.values():
        cat.drop_layouts()
