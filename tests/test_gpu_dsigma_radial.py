"""GPU: the excess-surface-density count binned in each lens's own radius (``yawhip_dsigma_count_radial``) and the drivers with
``radius="lens"`` on the device, against the numpy brute force of tests/dsigma_radial_oracle.py, on the scene of
tests/test_gpu_dsigma.py (that of tests/test_gpu_shear.py with redshifts on both sides).

Membership is tested EXACTLY: with unit weights, ``f = 1``, ``c = 0`` and zero shear ``W`` is the integer number of pairs per
cell and must equal the oracle's with ``np.array_equal``. The signed sums of real columns follow the rule of
tests/shear_exact.py, ``|ours - oracle| <= K eps A_theta + 1e-13 A`` per cell with the ``K`` of its fixture."""
import functools

import numpy as np
import pytest

import dsigma_radial_oracle as oracle
import helpers
import shear_exact
from test_gpu_dsigma import dsigma_scene
from test_gpu_shear import DEG, JOBS, N_BINS
from yet_another_wizz_amd import _lib, engine
from yet_another_wizz_amd.catalog import radec_to_xyz

pytestmark = pytest.mark.gpu
RTOL_W = helpers.RTOL_W
COLUMNS_L = ("x", "y", "z", "w", "f", "c", "m")
COLUMNS_S = ("x", "y", "z", "w", "g1", "g2", "u")


def radii2(nf, n_bins=N_BINS, rmin=0.15, rmax=3.0):
    """f64[B, nf + 1]: squared log-spaced radius edges in Mpc^2, other limits in every bin. The lenses of the scene have
    ``700 < D_A < 1700`` Mpc: the angles run from 0.3 to 15 arcmin."""
    return np.array([np.geomspace(rmin * (1.0 + 0.1 * k), rmax * (1.0 - 0.05 * k), nf + 1) for k in range(n_bins)]) ** 2


@functools.lru_cache(maxsize=None)
def radial_scene(columns, nb=N_BINS):
    """The scene of tests/test_gpu_dsigma.py with ``m = D_A(z_l)^2``. ``columns="unit"``: no weights, ``f = 1``, ``c = 0``, zero
    shear (``W`` counts pairs); ``"real"``: everything as it comes. ``nb``: the lenses in 4 or 1 redshift bins."""
    lens, src = dsigma_scene()
    lens = dict(lens, m=lens["f"] * lens["f"])
    if columns == "unit":
        lens = dict(lens, w=None, f=np.ones_like(lens["f"]), c=np.zeros_like(lens["c"]))
        src = dict(src, w=None, g1=np.zeros_like(src["g1"]), g2=np.zeros_like(src["g2"]))
    if nb != N_BINS:
        lens = dict(lens, nb=nb, off=lens["off"][:: N_BINS // nb].copy())
    return lens, src


@functools.lru_cache(maxsize=None)
def expected(columns, nf, nb=N_BINS):
    """The oracle's (T, X, W, A, A_theta) of the scene: computed once per case, shared, never modified."""
    lens, src = radial_scene(columns, nb)
    out = oracle.radial_jobs(lens, src, JOBS, radii2(nf))
    for a in out:
        a.setflags(write=False)
    return out


def upload(ctx, lens, src, sort_axis=2, src_axis=None, radial=True):
    n_patches = len(src["off"]) - 1
    lenses = _lib.DsigmaLenses(ctx, lens["x"], lens["y"], lens["z"], lens["w"], lens["f"], lens["c"], n_patches, lens["nb"], lens["off"],
                               sort_axis=sort_axis, m=lens["m"] if radial else None)
    sources = _lib.ShearSources(ctx, src["x"], src["y"], src["z"], src["w"], src["g1"], src["g2"], n_patches, src["off"],
                                sort_axis=sort_axis if src_axis is None else src_axis, u=src["u"])
    return lenses, sources


def count(lens, src, jobs, r2, sort_axis=2, src_axis=None):
    ctx = engine.get_context(0)
    lenses, sources = upload(ctx, lens, src, sort_axis, src_axis)
    try:
        return _lib.dsigma_count_radial(ctx, lenses, sources, jobs, r2)
    finally:
        lenses.free(), sources.free()


def check_real_sums(key, got, exp):
    K = float(shear_exact.fixture()["K"])
    T_o, X_o, W_o, A, Ath = exp
    shear_exact.check(key, "TX", got[:2], got[2], ((T_o, X_o), W_o, A, Ath), K)


ONE_JOB = np.array([[0, 0]], dtype=np.int32)


def one_patch(lens_xyz, m, src_xyz):
    """Unit-column catalogues of one patch and one bin from coordinates [3, n]."""
    n_l, n_s = lens_xyz.shape[1], src_xyz.shape[1]
    lens = dict(zip("xyz", (c.copy() for c in lens_xyz)), w=None, f=np.ones(n_l), c=np.zeros(n_l), m=np.asarray(m, dtype=np.float64), nb=1,
                off=np.array([0, n_l], dtype=np.int64))
    src = dict(zip("xyz", (c.copy() for c in src_xyz)), w=None, g1=np.zeros(n_s), g2=np.zeros(n_s), u=np.zeros(n_s),
               off=np.array([0, n_s], dtype=np.int64))
    return lens, src


def box_xyz(rng, n, lo=40.0, hi=40.5):
    return np.array(radec_to_xyz(rng.uniform(lo, hi, n) * DEG, rng.uniform(30.0, 30.0 + hi - lo, n) * DEG))


# --------------------------------------------------------------------------- 1. exact membership
@pytest.mark.parametrize("sort_axis", [0, 1, 2])
@pytest.mark.parametrize("nf", [1, 12, 50])
def test_membership_is_the_oracles(nf, sort_axis):
    exp = expected("unit", nf)
    assert np.all(exp[2].sum(axis=(1, 2)) > 0) and np.any(exp[2] == 0)  # pairs in every job, and empty cells
    T, X, W, stats = count(*radial_scene("unit"), JOBS, radii2(nf), sort_axis)
    assert stats.n_workgroups == len(JOBS) * N_BINS and 0 < stats.evaluated_pairs <= stats.candidate_pairs
    assert np.array_equal(W, exp[2]) and np.all(W == np.rint(W))
    assert not np.any(T) and not np.any(X)


def test_lenses_in_one_bin_under_four_rows_of_radii():
    exp = expected("unit", 12, 1)
    assert np.count_nonzero(np.any(exp[2][:, 0] != exp[2][:, 1], axis=1)) >= 4  # the rows give other counts
    T, X, W, stats = count(*radial_scene("unit", 1), JOBS, radii2(12))
    assert stats.n_workgroups == len(JOBS) * N_BINS
    assert np.array_equal(W, exp[2])


@pytest.mark.parametrize("sort_axis", [0, 2])
def test_two_distances_alternating_inside_one_long_segment(sort_axis):
    """600 lenses in one segment (three stages, the last ragged), ``m`` alternating between two values a factor 49 apart in
    the order of the sort key, so that every stage mixes them; 300 sources: a full lane tile and a padded one."""
    rng = np.random.default_rng(5 + sort_axis)
    lens_xyz, src_xyz = box_xyz(rng, 600), box_xyz(rng, 300)
    m = np.empty(600)
    m[np.argsort(lens_xyz[sort_axis], kind="stable")] = np.where(np.arange(600) % 2 == 0, 900.0**2, 900.0**2 / 49.0)
    lens, src = one_patch(lens_xyz, m, src_xyz)
    r2 = np.array([np.geomspace(0.05, 0.6, 13)]) ** 2  # up to 2.3 arcmin around the far lenses, 16 around the near ones
    exp = oracle.radial_jobs(lens, src, ONE_JOB, r2)[2]
    near_only = oracle.radial_jobs(dict(lens, m=np.where(m < 1e5, m, 1e12)), src, ONE_JOB, r2)[2]
    assert near_only.sum() > 0 and (exp - near_only).sum() > 0 and np.all(exp[0, 0] > 0)  # both kinds of lens hold pairs
    T, X, W, stats = count(lens, src, ONE_JOB, r2, sort_axis)
    assert np.array_equal(W, exp)
    assert stats.evaluated_pairs <= stats.candidate_pairs == 600 * 300


@pytest.mark.parametrize("sort_axis", [0, 1, 2])
def test_partners_next_to_an_edge_and_on_it(sort_axis):
    """Sources displaced from a lens along the sort axis only, by the chord of the angle at which ``R^2`` is an inner / outer
    edge times ``(1 -/+ 1e-9)``, around the lenses that come first and last in their segment (the construction of
    tests/test_gpu_dsigma.py). The lenses' ``m`` are powers of two, so ``R2 = m th2`` is an exact product: two edges are then
    SET to the ``R2`` of one placed pair each, which must fall into the bin below its edge."""
    rng = np.random.default_rng(17 + sort_axis)
    lens_xyz = box_xyz(rng, 40)
    m = 2.0 ** rng.integers(18, 22, 40)  # D = 512 ... 1448
    r2 = np.array([[0.2, 0.9, 2.5]]) ** 2
    first, last = int(np.argmin(lens_xyz[sort_axis])), int(np.argmax(lens_xyz[sort_axis]))
    placed, owner = [], []
    for at in (first, last):
        for edge in (r2[0, 0], r2[0, 2]):
            for factor in (1.0 - 1e-9, 1.0, 1.0 + 1e-9):
                for sign in (-1.0, 1.0):
                    p = lens_xyz[:, at].copy()
                    p[sort_axis] += sign * 2.0 * np.sin(0.5 * np.sqrt(edge * factor / m[at]))
                    placed.append(p), owner.append((at, edge, factor))
    src_xyz = np.concatenate([np.array(placed).T, box_xyz(rng, 300)], axis=1)  # filler: two lane tiles
    lens, src = one_patch(lens_xyz, m, src_xyz)

    def pair_r2(i_lens, i_src):
        d = [src[c][i_src] - lens[c][i_lens] for c in "xyz"]
        return float(m[i_lens] * oracle.squared_angle((d[0] * d[0] + d[1] * d[1]) + d[2] * d[2]))

    # the pair placed at factor 1.0 below the first lens sets the inner edge, the one above the last lens the outer edge
    on_inner = next(i for i, (at, edge, factor) in enumerate(owner) if at == first and edge == r2[0, 0] and factor == 1.0)
    on_outer = next(i for i, (at, edge, factor) in enumerate(owner) if at == last and edge == r2[0, 2] and factor == 1.0) + 1
    r2[0, 0], r2[0, 2] = pair_r2(first, on_inner), pair_r2(last, on_outer)
    assert abs(r2[0, 0] / 0.04 - 1.0) < 1e-10 and abs(r2[0, 2] / 6.25 - 1.0) < 1e-10
    exp = oracle.radial_jobs(lens, src, ONE_JOB, r2)[2]
    only_placed = dict(src, **{c: src[c][: len(placed)] for c in COLUMNS_S if src[c] is not None}, off=np.array([0, len(placed)]))
    W_placed = oracle.radial_jobs(lens, only_placed, ONE_JOB, r2)[2]
    assert W_placed[0, 0, 0] > 0 and W_placed[0, 0, 1] > 0  # edge pairs on both sides of being counted
    # the pairs ON the two edges (the one that set it, and any that happens to share its bits): one ulp less of the inner edge
    # takes them into the first bin, one ulp less of the outer edge out of the last
    d = [only_placed[c][None, :] - lens[c][:, None] for c in "xyz"]
    R2 = m[:, None] * oracle.squared_angle((d[0] * d[0] + d[1] * d[1]) + d[2] * d[2])
    for column, which, sign in ((0, 0, 1), (2, 1, -1)):
        n_on = np.count_nonzero(R2 == r2[0, column])
        moved = r2.copy()
        moved[0, column] = np.nextafter(moved[0, column], 0.0)
        W_moved = oracle.radial_jobs(lens, only_placed, ONE_JOB, moved)[2]
        assert n_on >= 1 and W_moved[0, 0, which] == W_placed[0, 0, which] + sign * n_on
    T, X, W, _ = count(lens, src, ONE_JOB, r2, sort_axis)
    assert np.array_equal(W, exp)


@pytest.mark.parametrize("sort_axis", [0, 1, 2])
def test_the_window_follows_the_nearest_lens_of_the_bin(sort_axis):
    """One lens eight times nearer than the other 299 of its segment (``m`` 64 times smaller), with partners at the far end of
    ITS reach along the sort axis, eight window widths of the others away."""
    rng = np.random.default_rng(29 + sort_axis)
    lens_xyz = box_xyz(rng, 300, 40.0, 42.0)
    m = np.full(300, 1600.0**2)
    near = 123
    m[near] = 200.0**2
    r2 = np.array([np.geomspace(0.3, 2.0, 6)]) ** 2  # 2 Mpc: 4.3 arcmin at 1600 Mpc, 34 arcmin at 200 Mpc
    placed = []
    for factor in (0.7, 1.0 - 1e-6, 1.0 + 1e-6):
        for sign in (-1.0, 1.0):
            p = lens_xyz[:, near].copy()
            p[sort_axis] += sign * 2.0 * np.sin(0.5 * np.sqrt(r2[0, -1] * factor / m[near]))
            placed.append(p)
    src_xyz = np.concatenate([np.array(placed).T, box_xyz(rng, 400, 40.0, 42.0)], axis=1)
    lens, src = one_patch(lens_xyz, m, src_xyz)
    exp = oracle.radial_jobs(lens, src, ONE_JOB, r2)[2]
    alone = dict(lens, **{c: lens[c][near:near + 1] for c in COLUMNS_L if lens[c] is not None}, off=np.array([0, 1], dtype=np.int64))
    only_placed = dict(src, **{c: src[c][:6] for c in COLUMNS_S if src[c] is not None}, off=np.array([0, 6]))
    assert oracle.radial_jobs(alone, only_placed, ONE_JOB, r2)[2][0, 0, -1] == 4.0  # four of the six inside the last bin
    T, X, W, stats = count(lens, src, ONE_JOB, r2, sort_axis)
    assert np.array_equal(W, exp)
    assert 0 < stats.evaluated_pairs <= stats.candidate_pairs


def test_different_sort_axes_stream_the_whole_segment():
    lens, src = radial_scene("unit")
    r2 = radii2(12)
    windowed = count(lens, src, JOBS, r2, 2, 2)
    whole = count(lens, src, JOBS, r2, 2, 0)
    assert whole[3].evaluated_pairs == whole[3].candidate_pairs > windowed[3].evaluated_pairs
    assert np.array_equal(whole[2], windowed[2]) and np.array_equal(whole[2], expected("unit", 12)[2])


# --------------------------------------------------------------------------- 2. real sums
@pytest.mark.parametrize("sort_axis", [0, 2])
@pytest.mark.parametrize("nf", [12, 50])
def test_real_sums_match_the_oracle(nf, sort_axis):
    exp = expected("real", nf)
    T, X, W, _ = count(*radial_scene("real"), JOBS, radii2(nf), sort_axis)
    check_real_sums(f"radial nf={nf} axis={sort_axis}", (T, X, W), exp)


def test_real_sums_with_lenses_in_one_bin():
    T, X, W, _ = count(*radial_scene("real", 1), JOBS, radii2(12))
    check_real_sums("radial nb=1", (T, X, W), expected("real", 12, 1))


# --------------------------------------------------------------------------- 3. reproducibility, sources in front, the plain count
def test_two_calls_return_the_same_bits():
    ctx = engine.get_context(0)
    lenses, sources = upload(ctx, *radial_scene("real"))
    try:
        one = _lib.dsigma_count_radial(ctx, lenses, sources, JOBS, radii2(50))[:3]
        two = _lib.dsigma_count_radial(ctx, lenses, sources, JOBS, radii2(50))[:3]
    finally:
        lenses.free(), sources.free()
    assert np.count_nonzero(one[0]) > 100
    for a, b in zip(one, two):
        assert np.array_equal(a, b)


def test_sources_that_all_lie_in_front_give_zero_planes():
    lens, src = radial_scene("real")
    src = dict(src, u=np.full_like(src["u"], 2.0 / lens["c"].min()))  # c u >= 2 for every pair
    T, X, W, stats = count(lens, src, JOBS, radii2(12))
    assert stats.evaluated_pairs > 0
    for plane in (T, X, W):
        assert np.all(plane == 0.0) and not np.any(np.signbit(plane))


def test_the_plain_count_ignores_m():
    """``yawhip_dsigma_count`` on a radial handle returns the bits of the same call on a plain lens handle."""
    from test_gpu_shear import thresholds

    ctx = engine.get_context(0)
    lens, src = radial_scene("real")
    radial, sources = upload(ctx, lens, src)
    plain, _unused = upload(ctx, lens, src, radial=False)
    try:
        a = _lib.dsigma_count(ctx, radial, sources, JOBS, thresholds(50))
        b = _lib.dsigma_count(ctx, plain, sources, JOBS, thresholds(50))
    finally:
        for h in (radial, sources, plain, _unused):
            h.free()
    assert np.count_nonzero(a[0]) > 100
    for x, y in zip(a[:3], b[:3]):
        assert np.array_equal(x, y)
    assert a[3].evaluated_pairs == b[3].evaluated_pairs


# --------------------------------------------------------------------------- 4. refusals
def test_uploads_refuse_a_column_m_out_of_range():
    ctx = engine.get_context(0)
    lens, src = radial_scene("unit")
    for value in (0.0, -1.0, np.nan, np.inf):
        m = lens["m"].copy()
        m[17] = value
        with pytest.raises(_lib.YawhipError, match="column m"):
            _lib.DsigmaLenses(ctx, lens["x"], lens["y"], lens["z"], None, lens["f"], lens["c"], 3, N_BINS, lens["off"], m=m)
    for column, value in (("f", -1.0), ("c", np.nan)):  # the checks of the plain upload stay
        bad = dict(lens, **{column: lens[column].copy()})
        bad[column][17] = value
        with pytest.raises(_lib.YawhipError, match=f"column {column}"):
            _lib.DsigmaLenses(ctx, bad["x"], bad["y"], bad["z"], None, bad["f"], bad["c"], 3, N_BINS, bad["off"], m=lens["m"])


def test_mismatched_handles_and_reaches_are_refused():
    ctx = engine.get_context(0)
    other = _lib.Context(0)
    lens, src = radial_scene("unit")
    r2 = radii2(1)
    lenses, sources = upload(ctx, lens, src)
    plain, _unused = upload(ctx, lens, src, radial=False)
    foreign_lenses, foreign_sources = upload(other, lens, src)
    no_u = _lib.ShearSources(ctx, src["x"], src["y"], src["z"], None, src["g1"], src["g2"], 3, src["off"])
    binned = _lib.ShearSources(ctx, lens["x"], lens["y"], lens["z"], None, lens["f"], lens["c"], 3, lens["off"], n_bins=N_BINS)
    catalog = _lib.DeviceCatalog(ctx, lens["x"], lens["y"], lens["z"], None, 3, N_BINS, lens["off"])
    cells = np.array([[0, 0, 0, 0, 0]], dtype=np.int32)
    try:
        with pytest.raises(_lib.YawhipError, match="not a handle of yawhip_dsigma_upload_lenses_radial"):
            _lib.dsigma_count_radial(ctx, plain, sources, JOBS, r2)  # a lens handle without m
        with pytest.raises(_lib.YawhipError, match="sources are not a handle of yawhip_dsigma_upload_sources"):
            _lib.dsigma_count_radial(ctx, lenses, lenses, JOBS, r2)  # a lens handle as sources
        with pytest.raises(_lib.YawhipError, match="sources are not a handle of yawhip_dsigma_upload_sources"):
            _lib.dsigma_count_radial(ctx, lenses, no_u, JOBS, r2)
        with pytest.raises(_lib.YawhipError, match="lenses are not a handle of yawhip_dsigma_upload_lenses"):
            _lib.dsigma_count_radial(ctx, sources, sources, JOBS, r2)
        with pytest.raises(_lib.YawhipError, match="another context"):
            _lib.dsigma_count_radial(ctx, foreign_lenses, sources, JOBS, r2)
        with pytest.raises(_lib.YawhipError, match="another context"):
            _lib.dsigma_count_radial(ctx, lenses, foreign_sources, JOBS, r2)
        # the cap: the nearest lens of the scene is ~700 Mpc away, 0.01 is a chord of 0.1: 70 Mpc is too much in any bin ...
        with pytest.raises(_lib.YawhipError, match="a lens is too close for the largest radius"):
            _lib.dsigma_count_radial(ctx, lenses, sources, JOBS, radii2(1, rmax=100.0))
        # ... and exactly at the cap, per bin: the first radius beyond smax = 0.01 of bin 2 alone
        per_bin = [np.concatenate([lens["m"][lens["off"][p * N_BINS + k]:lens["off"][p * N_BINS + k + 1]] for p in range(3)]).min()
                   for k in range(N_BINS)]
        fits = np.array([[0.0, 0.0099 * per_bin[k]] for k in range(N_BINS)])
        _lib.dsigma_count_radial(ctx, lenses, sources, JOBS, fits)
        beyond = fits.copy()
        beyond[2, 1] = 0.0101 * per_bin[2]
        with pytest.raises(_lib.YawhipError, match="a lens is too close for the largest radius"):
            _lib.dsigma_count_radial(ctx, lenses, sources, JOBS, beyond)
        with pytest.raises(_lib.YawhipError, match="not finite|not ascending"):
            _lib.dsigma_count_radial(ctx, lenses, sources, JOBS, np.array([[0.0, np.inf]] * N_BINS))
        with pytest.raises(_lib.YawhipError, match="not ascending"):
            _lib.dsigma_count_radial(ctx, lenses, sources, JOBS, r2[:, ::-1].copy())
        with pytest.raises(_lib.YawhipError, match="bad sizes"):
            _lib.dsigma_count_radial(ctx, lenses, sources, JOBS, radii2(256))  # 257 edges
        # a radial lens handle is a lens handle: the three shear counts refuse it
        with pytest.raises(_lib.YawhipError, match="not a shear catalogue"):
            _lib.shear_count(ctx, catalog, lenses, JOBS, r2)
        with pytest.raises(_lib.YawhipError, match="not a shear catalogue"):
            _lib.shear_auto_count(ctx, lenses, np.array([[0, 0]], dtype=np.int32), r2)
        with pytest.raises(_lib.YawhipError, match="not a shear catalogue"):
            _lib.shear_pair_count(ctx, lenses, binned, cells, r2)
        T, X, W, _ = _lib.dsigma_count_radial(ctx, lenses, sources, np.empty((0, 2), dtype=np.int32), r2)  # nothing to do
        assert T.shape == (0, N_BINS, 1)
    finally:
        for h in (lenses, sources, plain, _unused, foreign_lenses, foreign_sources, no_u, binned, catalog):
            h.free()
        other.close()


# --------------------------------------------------------------------------- 5. end to end
def test_both_drivers_end_to_end(monkeypatch):
    """The scenarios of the CPU driver tests through the real library (both entry points, ``ref_rand`` and ``boost``), held to
    the oracle with the device tolerances, and to the drivers on the stand-in with the same bounds."""
    from test_dsigma_radial_host import check_radial_scenario, check_shear_scenario

    on_device, bounds = check_radial_scenario("kpc", device=True)
    shear_on_device = check_shear_scenario(device=True)
    monkeypatch.setattr(engine, "count_dsigma_radial_fine", oracle.count_dsigma_radial_fine)
    stand_in, _ = check_radial_scenario("kpc", device=False)
    shear_stand_in = check_shear_scenario(device=False)
    for ours, theirs, bound in zip(on_device, stand_in, bounds):
        dd_ours, dd_theirs = (cf[0].dd.sample_patch_sum().data for cf in (ours, theirs))
        assert np.all(np.abs(dd_ours - dd_theirs) <= bound)
        np.testing.assert_allclose(ours[2].sample().data + 1.0, theirs[2].sample().data + 1.0, rtol=1e-11 + 2.0 * RTOL_W * (1.0 + 1e-9), atol=0)
        np.testing.assert_allclose(ours[2].dd.counts.counts, theirs[2].dd.counts.counts, rtol=RTOL_W, atol=0)
    for ours, theirs in zip(shear_on_device, shear_stand_in):
        np.testing.assert_allclose(ours[0].dd.number_counts.counts, theirs[0].dd.number_counts.counts, rtol=RTOL_W, atol=0)
        np.testing.assert_allclose(ours[0].dr.number_counts.counts, theirs[0].dr.number_counts.counts, rtol=RTOL_W, atol=0)
