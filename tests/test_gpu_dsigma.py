"""GPU: the excess-surface-density count (``yawhip_dsigma_count``) and ``crosscorrelate_delta_sigma`` on the device, against
the numpy brute force of tests/dsigma_oracle.py, on the scene of tests/test_gpu_shear.py with redshifts on both sides.

The rule for the signed sums is that of the shear count: per (job, bin, fine bin) cell ``|T - T_o| <= 1e-10 * A`` and the same
for ``X``, with ``A = sum |w_l w_s| s (|g1| + |g2|)`` over the cell's pairs with the source behind its lens (the factor ``s`` is one
more float64 product per pair: ~1e-16 relative, and no test of this file goes below 0.5 arcmin -- tests/test_gpu_shear_exact.py does --, where the projection's error is ~1e-12);
a cell without such pairs must be exactly 0. ``W`` is held to ``helpers.RTOL_W``. Every test prints its worst ``|delta| / A``."""
import functools
import types

import numpy as np
import pytest

import dsigma_oracle
import helpers
from conftest import ARCMIN
from test_gpu_shear import DEG, JOBS, N_BINS, scene, thresholds
from yet_another_wizz_amd import _lib, cosmology, engine
from yet_another_wizz_amd.catalog import radec_to_xyz

pytestmark = pytest.mark.gpu
RTOL_W = helpers.RTOL_W


@functools.lru_cache(maxsize=None)
def dsigma_scene():
    """The shear scene (source patches of 1, 257 and 1500; an empty lens segment; a knot of 700 lenses inside 2 arcmin) with
    redshifts drawn from one distribution on both sides, so that about half the pairs have the source in front of the lens;
    the three columns are those of the driver: ``D_A(z_l)``, ``chi_l`` and ``1 / chi_s`` in Mpc."""
    lens, src = scene()
    rng = np.random.default_rng(99)
    z_l, z_s = rng.uniform(0.2, 0.9, len(lens["x"])), rng.uniform(0.2, 0.9, len(src["x"]))
    lens_z, src_z = (types.SimpleNamespace(redshifts=z) for z in (z_l, z_s))
    f, c, u = engine.dsigma_columns(lens_z, src_z, cosmology.Planck15)
    return dict(lens, f=f, c=c), dict(src, u=u)


def weighted_scene(weights, nb=N_BINS):
    """The scene with both weight columns ("both") or neither ("none"), and the lenses in ``nb`` = 4, 2 or 1 redshift bins
    (neighbouring bins merged: the objects of a patch stay together)."""
    lens, src = dsigma_scene()
    if weights == "none":
        lens, src = dict(lens, w=None), dict(src, w=None)
    if nb != N_BINS:
        lens = dict(lens, nb=nb, off=lens["off"][:: N_BINS // nb].copy())
    return lens, src


@functools.lru_cache(maxsize=None)
def expected(weights, nf, nb=N_BINS):
    """The oracle's (T, X, W, A) of the scene: computed once per case, shared, never modified."""
    lens, src = weighted_scene(weights, nb)
    out = dsigma_oracle.dsigma_jobs(lens, src, JOBS, thresholds(nf, n_bins=N_BINS if nb == N_BINS else 2))
    for a in out:
        a.setflags(write=False)
    return out


def upload(ctx, lens, src, sort_axis=2, src_axis=None):
    n_patches = len(src["off"]) - 1
    lenses = _lib.DsigmaLenses(ctx, lens["x"], lens["y"], lens["z"], lens["w"], lens["f"], lens["c"], n_patches, lens["nb"], lens["off"],
                               sort_axis=sort_axis)
    sources = _lib.ShearSources(ctx, src["x"], src["y"], src["z"], src["w"], src["g1"], src["g2"], n_patches, src["off"],
                                sort_axis=sort_axis if src_axis is None else src_axis, u=src["u"])
    return lenses, sources


def count(lens, src, jobs, t, sort_axis=2, src_axis=None):
    ctx = engine.get_context(0)
    lenses, sources = upload(ctx, lens, src, sort_axis, src_axis)
    try:
        return _lib.dsigma_count(ctx, lenses, sources, jobs, t)
    finally:
        lenses.free(), sources.free()


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
def test_the_scene_has_half_its_pairs_in_front():
    lens, src = dsigma_scene()
    behind = 1.0 - lens["c"][:600, None] * src["u"][None, :] > 0.0
    assert 0.4 < behind.mean() < 0.6


@pytest.mark.parametrize("sort_axis", [0, 1, 2])
@pytest.mark.parametrize("nf", [1, 12, 50])
@pytest.mark.parametrize("weights", ["both", "none"])
def test_fine_sums_match_the_oracle(weights, nf, sort_axis):
    exp = expected(weights, nf)
    assert np.all(exp[3].sum(axis=(1, 2)) > 0) and np.any(exp[3] == 0)  # cells with pairs in every job, and empty ones
    T, X, W, stats = count(*weighted_scene(weights), JOBS, thresholds(nf), sort_axis)
    assert stats.n_workgroups == len(JOBS) * N_BINS and 0 < stats.evaluated_pairs <= stats.candidate_pairs
    check_against_oracle(f"{weights} nf={nf} axis={sort_axis}", (T, X, W), exp)


@pytest.mark.parametrize("nb", [1, 2])
@pytest.mark.parametrize("weights", ["both", "none"])
def test_lenses_in_one_or_two_bins_under_two_rows_of_thresholds(weights, nb):
    """``nb = 1``: both cells of a job stream the one lens segment of its patch, each with the edges of its own row; ``nb = 2``:
    each its own segment."""
    exp = expected(weights, 12, nb)
    # every job holds pairs, and the two rows of thresholds give other sums (but for the jobs of the one-source patch)
    assert np.all(exp[3].sum(axis=(1, 2)) > 0) and np.count_nonzero(np.any(exp[2][:, 0] != exp[2][:, 1], axis=1)) >= 4
    T, X, W, stats = count(*weighted_scene(weights, nb), JOBS, thresholds(12, n_bins=2))
    assert stats.n_workgroups == len(JOBS) * 2 and 0 < stats.evaluated_pairs <= stats.candidate_pairs
    check_against_oracle(f"{weights} nb={nb}", (T, X, W), exp)


# --------------------------------------------------------------------------- 2. the shear count inside
@pytest.mark.parametrize("weights", ["both", "none"])
def test_unit_columns_return_the_bits_of_the_shear_count(weights):
    """``f = 1, c = 0`` and any ``u``: the planes and the evaluated separations of ``yawhip_shear_count`` on a plain upload of
    the same columns; with the real columns the evaluated separations stay: the window knows nothing of redshifts."""
    ctx = engine.get_context(0)
    lens, src = weighted_scene(weights)
    unit = dict(lens, f=np.ones_like(lens["f"]), c=np.zeros_like(lens["c"]))
    t = thresholds(50)
    plain_lenses = _lib.DeviceCatalog(ctx, lens["x"], lens["y"], lens["z"], lens["w"], 3, N_BINS, lens["off"], sort_axis=2)
    plain_sources = _lib.ShearSources(ctx, src["x"], src["y"], src["z"], src["w"], src["g1"], src["g2"], 3, src["off"], sort_axis=2)
    unit_lenses, sources = upload(ctx, unit, src)
    real_lenses, _unused = upload(ctx, lens, src)
    try:
        shear = _lib.shear_count(ctx, plain_lenses, plain_sources, JOBS, t)
        ignoring_u = _lib.shear_count(ctx, plain_lenses, sources, JOBS, t)  # a handle with u is a shear handle too
        got = _lib.dsigma_count(ctx, unit_lenses, sources, JOBS, t)
        real = _lib.dsigma_count(ctx, real_lenses, sources, JOBS, t)
    finally:
        for h in (plain_lenses, plain_sources, unit_lenses, sources, real_lenses, _unused):
            h.free()
    assert np.count_nonzero(shear[0]) > 100
    for a, b, c in zip(got[:3], shear[:3], ignoring_u[:3]):
        assert np.array_equal(a, b) and np.array_equal(c, b)
    for stats in (got[3], real[3], ignoring_u[3]):
        assert stats.evaluated_pairs == shear[3].evaluated_pairs and stats.candidate_pairs == shear[3].candidate_pairs
    assert 0 < np.count_nonzero(real[2]) <= np.count_nonzero(shear[2])


# --------------------------------------------------------------------------- 3. the clip
def clip_scene():
    """Eight lenses inside 1 arcmin, sources 3 - 6 arcmin around them: every source pairs with every lens. Per lens a group of
    sources has ``u`` at ``1 / c`` rounded, its two neighbours on either side, and every neighbour within 4 ulp whose product
    with ``c`` rounds to exactly 1.0; three lenses have ``c`` a power of two, whose ``1 / c`` gives exactly 1.0."""
    rng = np.random.default_rng(41)
    ra0, dec0 = 50.0 * DEG, 20.0 * DEG
    n_l = 8
    lra, ldec = ra0 + rng.uniform(-0.5, 0.5, n_l) * ARCMIN, dec0 + rng.uniform(-0.5, 0.5, n_l) * ARCMIN
    c = np.concatenate([[512.0, 1024.0, 2048.0], rng.uniform(600.0, 2500.0, n_l - 3)])
    f = c / rng.uniform(1.2, 1.9, n_l)
    u = []
    for ck in c:
        mid = 1.0 / ck
        steps = [mid]
        for direction in (0.0, np.inf):
            v = mid
            for _ in range(4):
                v = np.nextafter(v, direction)
                steps.append(v)
        u += steps
    u = np.array(u + [0.0, 1.0 / 9000.0, 1.0 / 300.0])
    exact = np.array([[ck * uk == 1.0 for uk in u] for ck in c])
    assert exact.any(axis=1).all() and (1.0 - c[:, None] * u[None, :] > 0).any() and (1.0 - c[:, None] * u[None, :] < 0).any()
    n_s = len(u)
    r, theta = rng.uniform(3.0, 6.0, n_s) * ARCMIN, rng.uniform(0, 2 * np.pi, n_s)
    sra, sdec = ra0 + r * np.cos(theta) / np.cos(dec0), dec0 + r * np.sin(theta)
    lens = dict(zip("xyz", radec_to_xyz(lra, ldec)), w=rng.uniform(0.5, 2.0, n_l), f=f, c=c, nb=1, off=np.array([0, n_l], dtype=np.int64))
    src = dict(zip("xyz", radec_to_xyz(sra, sdec)), w=rng.uniform(0.5, 2.0, n_s), g1=rng.normal(0, 0.3, n_s), g2=rng.normal(0, 0.3, n_s),
               u=u, off=np.array([0, n_s], dtype=np.int64))
    return lens, src


def test_the_clip_is_the_oracles_to_the_last_bit_of_c_times_u():
    lens, src = clip_scene()
    jobs = np.array([[0, 0]], dtype=np.int32)
    t = (2.0 * np.sin(0.5 * np.array([[1.5, 4.5, 8.0]]) * ARCMIN)) ** 2
    # per (lens, source) pair alone: a pair on the wrong side of the clip shows as a cell that should be exactly zero, or is not
    T, X, W, _ = count(lens, src, jobs, t)
    exp = dsigma_oracle.dsigma_jobs(lens, src, jobs, t)
    assert np.all(exp[2] > 0)
    check_against_oracle("clip", (T, X, W), exp)
    for k in range(len(lens["c"])):  # lens by lens, source group by source group: the cells are sums of nine sources at most
        one = dict(lens, **{col: lens[col][k:k + 1] for col in ("x", "y", "z", "w", "f", "c")}, off=np.array([0, 1], dtype=np.int64))
        group = slice(9 * k, 9 * k + 9)
        near = dict(src, **{col: src[col][group] for col in ("x", "y", "z", "w", "g1", "g2", "u")}, off=np.array([0, 9], dtype=np.int64))
        got = count(one, near, jobs, t)[:3]
        ref = dsigma_oracle.dsigma_jobs(one, near, jobs, t)
        assert 0 < np.count_nonzero(1.0 - one["c"] * near["u"] > 0) < 9
        check_against_oracle(f"clip lens {k}", got, ref)
        for j in range(9):  # and pair by pair
            single = dict(near, **{col: near[col][j:j + 1] for col in ("x", "y", "z", "w", "g1", "g2", "u")}, off=np.array([0, 1], dtype=np.int64))
            got = count(one, single, jobs, t)[:3]
            ref = dsigma_oracle.dsigma_jobs(one, single, jobs, t)
            assert np.array_equal(got[2] != 0, ref[2] != 0), (k, j)
            check_against_oracle(f"clip lens {k} source {j}", got, ref)


def test_sources_that_all_lie_in_front_give_zero_planes():
    lens, src = weighted_scene("both")
    src = dict(src, u=np.full_like(src["u"], 2.0 / lens["c"].min()))  # c u >= 2 for every pair
    T, X, W, stats = count(lens, src, JOBS, thresholds(12))
    assert stats.evaluated_pairs > 0
    for plane in (T, X, W):
        assert np.all(plane == 0.0) and not np.any(np.signbit(plane))


# --------------------------------------------------------------------------- 4. sort axes and window edges
def test_different_sort_axes_stream_the_whole_segment():
    lens, src = weighted_scene("both")
    t = thresholds(12)
    windowed = count(lens, src, JOBS, t, 2, 2)
    whole = count(lens, src, JOBS, t, 2, 0)
    assert whole[3].evaluated_pairs == whole[3].candidate_pairs > windowed[3].evaluated_pairs
    assert np.all(whole[2][windowed[2] == 0] == 0.0)
    np.testing.assert_allclose(whole[2], windowed[2], rtol=RTOL_W, atol=0)
    check_against_oracle("lens z, sources x", whole[:3], expected("both", 12))


@pytest.mark.parametrize("sort_axis", [0, 1, 2])
def test_window_edges(sort_axis):
    """Sources displaced from a lens along the sort axis only, by the chord of an inner / outer bin edge times (1 -/+ 1e-9),
    around the lenses that come first and last in their segment (the construction of tests/test_gpu_shear.py): with unit
    columns ``W`` is the exact pair count, with real ones (every source behind every lens) it is the oracle's."""
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
    jobs = np.array([[0, 0]], dtype=np.int32)
    src = dict(x=src_xyz[0].copy(), y=src_xyz[1].copy(), z=src_xyz[2].copy(), w=None, g1=rng.normal(0, 0.3, n), g2=rng.normal(0, 0.3, n),
               u=rng.uniform(0.0, 1.0 / 2000.0, n), off=np.array([0, n], dtype=np.int64))
    base = dict(x=lens_xyz[0].copy(), y=lens_xyz[1].copy(), z=lens_xyz[2].copy(), w=None, nb=1, off=np.array([0, 40], dtype=np.int64))
    for name, f, c in (("unit", np.ones(40), np.zeros(40)), ("real", rng.uniform(500.0, 1200.0, 40), rng.uniform(600.0, 1900.0, 40))):
        lens = dict(base, f=f, c=c)
        exp = dsigma_oracle.dsigma_jobs(lens, src, jobs, t)
        only_placed = dict(src, **{col: src[col][:len(placed)] for col in ("x", "y", "z", "g1", "g2", "u")}, off=np.array([0, len(placed)]))
        W_placed = dsigma_oracle.dsigma_jobs(lens, only_placed, jobs, t)[2]
        assert W_placed[0, 0, 0] > 0 and W_placed[0, 0, 1] > 0  # edge pairs on both sides of being counted
        T, X, W, _ = count(lens, src, jobs, t, sort_axis)
        if name == "unit":
            assert np.array_equal(W, exp[2])
        check_against_oracle(f"edges axis={sort_axis} {name}", (T, X, W), exp)


# --------------------------------------------------------------------------- 5. reproducibility, pole
def test_two_calls_return_the_same_bits():
    ctx = engine.get_context(0)
    lenses, sources = upload(ctx, *weighted_scene("both"))
    try:
        one = _lib.dsigma_count(ctx, lenses, sources, JOBS, thresholds(50))[:3]
        two = _lib.dsigma_count(ctx, lenses, sources, JOBS, thresholds(50))[:3]
    finally:
        lenses.free(), sources.free()
    assert np.count_nonzero(one[0]) > 100
    for a, b in zip(one, two):
        assert np.array_equal(a, b)


def test_a_source_on_the_pole_adds_to_w_only():
    (lx,), (ly,), (lz,) = radec_to_xyz(np.array([1.0]), np.array([0.5 * np.pi - 3.0 * ARCMIN]))
    (ox,), (oy,), (oz,) = radec_to_xyz(np.array([1.3]), np.array([0.5 * np.pi - 5.0 * ARCMIN]))
    t = (2.0 * np.sin(0.5 * np.array([[0.5, 12.0]]) * ARCMIN)) ** 2
    jobs = np.array([[0, 0]], dtype=np.int32)
    lens = dict(x=np.array([lx]), y=np.array([ly]), z=np.array([lz]), w=np.array([1.5]), f=np.array([800.0]), c=np.array([1000.0]), nb=1,
                off=np.array([0, 1], dtype=np.int64))
    with_pole = dict(x=np.array([0.0, ox]), y=np.array([0.0, oy]), z=np.array([1.0, oz]), w=np.array([0.75, 1.25]),
                     g1=np.array([0.5, 0.1]), g2=np.array([0.3, -0.2]), u=np.array([0.0005, 0.00025]), off=np.array([0, 2], dtype=np.int64))
    without = dict(with_pole, **{col: with_pole[col][1:] for col in ("x", "y", "z", "w", "g1", "g2", "u")}, off=np.array([0, 1], dtype=np.int64))
    (T, X, W), (T1, X1, W1) = (count(lens, src, jobs, t)[:3] for src in (with_pole, without))
    assert np.all(np.isfinite(T)) and np.all(np.isfinite(X))
    assert T1[0, 0, 0] != 0.0 and np.array_equal(T, T1) and np.array_equal(X, X1)  # nothing from the source on the pole ...
    s_pole, s_other = 800.0 * (1.0 - 1000.0 * 0.0005), 800.0 * (1.0 - 1000.0 * 0.00025)
    assert W1[0, 0, 0] == ((1.5 * s_other) * s_other) * 1.25                        # ... but W includes it
    assert W[0, 0, 0] == W1[0, 0, 0] + ((1.5 * s_pole) * s_pole) * 0.75
    check_against_oracle("pole", (T, X, W), dsigma_oracle.dsigma_jobs(lens, with_pole, jobs, t))


# --------------------------------------------------------------------------- 6. end to end
def test_crosscorrelate_delta_sigma_end_to_end(monkeypatch):
    """The scenarios of the CPU driver tests through the real library, held to the oracle with the device tolerances, and to
    the driver on the stand-in with the same bounds."""
    from test_dsigma_host import check_dsigma_scenario, check_sis_scenario

    on_device, bounds = check_dsigma_scenario(device=True)
    check_sis_scenario()
    monkeypatch.setattr(engine, "count_dsigma_fine", dsigma_oracle.count_dsigma_fine)
    stand_in, _ = check_dsigma_scenario(device=False)
    for ours, theirs, bound in zip(on_device, stand_in, bounds):
        # DD of the tangential part within its bound; the randoms' ratio is checked against the oracle inside the scenario
        dd_ours, dd_theirs = (cf[0].dd.sample_patch_sum().data for cf in (ours, theirs))
        assert np.all(np.abs(dd_ours - dd_theirs) <= bound)
        np.testing.assert_allclose(ours[2].sample().data + 1.0, theirs[2].sample().data + 1.0, rtol=1e-11 + 2.0 * RTOL_W * (1.0 + 1e-9), atol=0)
        np.testing.assert_allclose(ours[2].dd.counts.counts, theirs[2].dd.counts.counts, rtol=RTOL_W, atol=0)


# --------------------------------------------------------------------------- 7. error paths
def test_mismatched_handles_are_refused():
    ctx = engine.get_context(0)
    other = _lib.Context(0)
    lens, src = weighted_scene("none")
    t = thresholds(1)
    lenses, sources = upload(ctx, lens, src)
    foreign_lenses, foreign_sources = upload(other, lens, src)
    plain = _lib.ShearSources(ctx, src["x"], src["y"], src["z"], None, src["g1"], src["g2"], 3, src["off"])
    binned = _lib.ShearSources(ctx, lens["x"], lens["y"], lens["z"], None, lens["f"], lens["c"], 3, lens["off"], n_bins=N_BINS)
    catalog = _lib.DeviceCatalog(ctx, lens["x"], lens["y"], lens["z"], None, 3, N_BINS, lens["off"])
    two_patches = _lib.ShearSources(ctx, src["x"], src["y"], src["z"], None, src["g1"], src["g2"], 2,
                                    np.array([0, 258, len(src["x"])], dtype=np.int64), u=src["u"])
    cells = np.array([[0, 0, 0, 0, 0]], dtype=np.int32)
    try:
        with pytest.raises(_lib.YawhipError, match="another context"):
            _lib.dsigma_count(ctx, foreign_lenses, sources, JOBS, t)
        with pytest.raises(_lib.YawhipError, match="another context"):
            _lib.dsigma_count(ctx, lenses, foreign_sources, JOBS, t)
        with pytest.raises(_lib.YawhipError, match="another context"):
            _lib.dsigma_count(other, foreign_lenses, sources, JOBS, t)
        with pytest.raises(_lib.YawhipError, match="sources are not a handle of yawhip_dsigma_upload_sources"):
            _lib.dsigma_count(ctx, lenses, lenses, JOBS, t)  # a lens handle as sources
        with pytest.raises(_lib.YawhipError, match="sources are not a handle of yawhip_dsigma_upload_sources"):
            _lib.dsigma_count(ctx, lenses, plain, JOBS, t)  # a source handle without u
        with pytest.raises(_lib.YawhipError, match="lenses are not a handle of yawhip_dsigma_upload_lenses"):
            _lib.dsigma_count(ctx, binned, sources, JOBS, t)  # a plain shear handle as lenses
        with pytest.raises(_lib.YawhipError, match="lenses are not a handle of yawhip_dsigma_upload_lenses"):
            _lib.dsigma_count(ctx, sources, sources, JOBS, t)
        # a lens handle is no shear catalogue: the three shear counts refuse it
        with pytest.raises(_lib.YawhipError, match="not a shear catalogue"):
            _lib.shear_count(ctx, catalog, lenses, JOBS, t)
        with pytest.raises(_lib.YawhipError, match="not a shear catalogue"):
            _lib.shear_auto_count(ctx, lenses, np.array([[0, 0]], dtype=np.int32), t)
        with pytest.raises(_lib.YawhipError, match="not a shear catalogue"):
            _lib.shear_pair_count(ctx, lenses, binned, cells, t)
        with pytest.raises(_lib.YawhipError, match="not a shear catalogue"):
            _lib.shear_pair_count(ctx, binned, lenses, cells, t)
        # the checks of the shear count
        with pytest.raises(_lib.YawhipError, match="patch counts differ"):
            _lib.dsigma_count(ctx, lenses, two_patches, JOBS, t)
        with pytest.raises(_lib.YawhipError, match="not ascending"):
            _lib.dsigma_count(ctx, lenses, sources, JOBS, t[:, ::-1].copy())
        with pytest.raises(_lib.YawhipError, match="does not fit"):
            _lib.dsigma_count(ctx, lenses, sources, JOBS, thresholds(1, n_bins=3))
        with pytest.raises(_lib.YawhipError, match="patch id outside"):
            _lib.dsigma_count(ctx, lenses, sources, np.array([[0, 3]], dtype=np.int32), t)
        with pytest.raises(_lib.YawhipError, match="bad sizes"):
            _lib.dsigma_count(ctx, lenses, sources, JOBS, thresholds(256))  # 257 edges
        T, X, W, _ = _lib.dsigma_count(ctx, lenses, sources, np.empty((0, 2), dtype=np.int32), t)  # nothing to do
        assert T.shape == (0, N_BINS, 1)
    finally:
        for h in (lenses, sources, foreign_lenses, foreign_sources, plain, binned, catalog, two_patches):
            h.free()
        other.close()


def test_uploads_refuse_columns_out_of_range():
    ctx = engine.get_context(0)
    lens, src = weighted_scene("none")
    for column, value in (("f", -1.0), ("c", np.nan), ("f", np.inf), ("c", -0.0 - 1e-300)):
        bad = dict(lens, **{column: lens[column].copy()})
        bad[column][17] = value
        with pytest.raises(_lib.YawhipError, match=f"column {column}"):
            _lib.DsigmaLenses(ctx, bad["x"], bad["y"], bad["z"], None, bad["f"], bad["c"], 3, N_BINS, bad["off"])
    for value in (-1e-9, np.nan, np.inf):
        u = src["u"].copy()
        u[5] = value
        with pytest.raises(_lib.YawhipError, match="column u"):
            _lib.ShearSources(ctx, src["x"], src["y"], src["z"], None, src["g1"], src["g2"], 3, src["off"], u=u)
    with pytest.raises(ValueError, match="unbinned"):
        _lib.ShearSources(ctx, lens["x"], lens["y"], lens["z"], None, lens["f"], lens["c"], 3, lens["off"], n_bins=N_BINS, u=lens["c"])
