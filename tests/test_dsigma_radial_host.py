"""CPU: lensing profiles binned in each lens's own radius (``radius="lens"`` of ``crosscorrelate_delta_sigma`` and
``crosscorrelate_shear``) above the device seam -- the C ABI's new names, the series of the squared angle against mpmath, the
radial plan, and the drivers with ``engine.count_dsigma_radial_fine`` replaced by the numpy brute force of
tests/dsigma_radial_oracle.py."""
import ctypes
import os
import re

import numpy as np
import pytest

import dsigma_oracle
import dsigma_radial_oracle as radial_oracle
import shear_oracle
import yet_another_wizz_amd as yaw
from conftest import ARCMIN, ROOT
from test_dsigma_host import CENTERS, K, ZEDGES, dsigma_scenario, jackknife, ratio_bound
from test_shear_host import ring_around
from yet_another_wizz_amd import _lib, angular_bins, cosmology, engine, measurements

COSMO = cosmology.Planck15
SYMBOLS = ("yawhip_dsigma_upload_lenses_radial", "yawhip_dsigma_count_radial")


@pytest.fixture
def stand_in(monkeypatch):
    monkeypatch.setattr(engine, "count_dsigma_radial_fine", radial_oracle.count_dsigma_radial_fine)
    monkeypatch.setattr(engine, "count_dsigma_fine", dsigma_oracle.count_dsigma_fine)


# --------------------------------------------------------------------------- 1. ABI
def test_new_symbols_are_declared_bound_and_built_at_abi_6():
    text = open(os.path.join(ROOT, "include", "yawhip.h")).read()
    code = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    lib = ctypes.CDLL(_lib.LIB_PATH)
    for name in SYMBOLS:
        assert name in _lib.ABI_SYMBOLS, name
        assert re.search(rf"\bint {name}\s*\(", code), name
        assert hasattr(lib, name), name
    assert re.search(r"#define YAWHIP_ABI_VERSION 6\b", text)


# --------------------------------------------------------------------------- 2. the series
def test_the_series_is_the_squared_angle_to_two_ulp():
    import mpmath

    mpmath.mp.dps = 50
    s2 = np.concatenate([np.geomspace(1e-14, 0.01, 397), [0.01, np.nextafter(0.01, 0.0), 0.005]])
    ours = radial_oracle.squared_angle(s2)
    worst = 0.0
    for s, got in zip(s2, ours):
        exact = (2 * mpmath.asin(mpmath.sqrt(mpmath.mpf(float(s))) / 2)) ** 2
        worst = max(worst, float(abs(mpmath.mpf(float(got)) - exact) / exact))
    print(f"worst relative error of the series over {len(s2)} points: {worst / 2.0**-53:.3f} * 2^-53")
    assert worst <= 2.0 * 2.0**-53
    assert np.all(ours >= s2)  # q >= 1 after rounding: what the kernel's outer test rests on
    assert radial_oracle.squared_angle(0.0) == 0.0


# --------------------------------------------------------------------------- 3. the plan
@pytest.mark.parametrize("rweight, resolution", [(None, None), (-0.8, 12), (0.5, None)])
@pytest.mark.parametrize("z", [0.15, 0.55, 0.9])
def test_the_radial_plan_is_the_angular_one_at_any_redshift(z, rweight, resolution):
    config = yaw.Configuration.create(rmin=[100.0, 300.0, 150.0], rmax=[2000.0, 1000.0, 160.0], unit="kpc", rweight=rweight,
                                      resolution=resolution, edges=np.linspace(0.1, 1.0, 5))
    plans = measurements.radial_plans(config)
    assert len(plans) == 4 and all(p is plans[0] for p in plans) and type(plans[0]) is angular_bins.RadialBinPlan
    radial = plans[0]
    angular = angular_bins.plan_for_limits(*config.scales.scales.get_angle_radian(z, cosmology=COSMO), rweight, resolution)
    assert radial._slices == angular._slices and radial.num_edges == angular.num_edges
    assert np.array_equal(radial.thresholds, radial.ang_bins * radial.ang_bins)
    d_a = float(COSMO.angular_diameter_distance(z))
    np.testing.assert_allclose(radial.ang_bins, angular.ang_bins * d_a, rtol=1e-13)  # radii in Mpc
    np.testing.assert_allclose(radial.limits, np.column_stack([[0.1, 0.3, 0.15], [2.0, 1.0, 0.16]]), rtol=1e-15)
    if rweight is None:
        assert radial._scale_factor is None and angular._scale_factor is None
    else:
        np.testing.assert_allclose(radial._scale_factor, angular._scale_factor, rtol=1e-12)
    fine = np.random.default_rng(1).uniform(0, 1, (5, radial.num_edges - 1))
    np.testing.assert_allclose(radial.combine(fine), angular.combine(fine), rtol=1e-12)


def test_radial_limits_are_checked():
    with pytest.raises(ValueError):
        angular_bins.radial_plan_for_limits([1.0], [0.5])
    with pytest.raises(ValueError):
        angular_bins.radial_plan_for_limits([0.0], [0.5])
    plan = angular_bins.radial_plan_for_limits([5.0], [50.0])  # radii beyond pi are fine
    assert plan.thresholds[-1] == pytest.approx(2500.0, rel=1e-14)


# --------------------------------------------------------------------------- 4. the drivers on the oracle stand-in
def scenario_config(unit):
    if unit == "kpc":
        return yaw.Configuration.create(rmin=[100.0, 300.0], rmax=[2000.0, 1000.0], unit="kpc", rweight=-0.8, resolution=12, edges=ZEDGES)
    return yaw.Configuration.create(rmin=[0.12, 0.4], rmax=[2.4, 1.3], unit="Mpc/h", rweight=-0.8, resolution=12, edges=ZEDGES)


def by_hand(config, lenses, sources, shear_only=False):
    """``sum T``, ``sum W`` and the magnitude ``sum A`` per scale, bin and patch pair [S, B, P, P] from the oracle's fine planes
    and the radial plan, over all nine patch pairs."""
    plans = measurements.radial_plans(config)
    r2 = measurements.threshold_table(plans)
    lens_layout = lenses.build_trees(config.binning.edges, closed=config.binning.closed, with_redshifts=True)
    source_layout = sources.build_trees(None, with_redshifts=not shear_only)
    jobs = np.array([(p, q) for p in range(3) for q in range(3)])
    f, c, m, u = engine.dsigma_radial_columns(lens_layout, source_layout, config.cosmology, config.scales.scales.unit, unit_columns=shear_only)
    T, _, W, A, _ = radial_oracle.radial_jobs(radial_oracle.as_lens(lens_layout, f, c, m), radial_oracle.as_sources(source_layout, u), jobs, r2)
    combine = measurements.CombinePlan(plans)
    out = []
    for fine in (T, W, A):
        per_scale = combine(np.moveaxis(fine, 0, -1))  # [S, B, J]
        out.append(per_scale.reshape(per_scale.shape[0], per_scale.shape[1], 3, 3))
    return out, (lens_layout, source_layout)


def check_radial_scenario(unit="kpc", device=False):
    """The scenario of tests/test_dsigma_host.py (three patches, three bins, two scales, ``rweight``) with ``radius="lens"``,
    through both drivers, with ``ref_rand`` and ``boost``; ``engine.count_dsigma_radial_fine`` is whatever the caller left in
    place (the stand-in: held to the host's rounding; the library: to the device tolerances of ``ratio_bound``). Returns the
    results of ``crosscorrelate_delta_sigma`` and the bounds of ``Delta Sigma`` per scale."""
    _, reference, sources, ref_rand = dsigma_scenario(with_randoms=True)
    config = scenario_config(unit)
    rtol_w = 1e-10 if device else 1e-13
    with_dr = yaw.crosscorrelate_delta_sigma(config, reference, sources, ref_rand=ref_rand, boost=True, radius="lens")
    dd_only = yaw.crosscorrelate_delta_sigma(config, reference, sources, radius="lens")
    (T_dd, W_dd, A_dd), (lens_layout, source_layout) = by_hand(config, reference, sources)
    (T_dr, W_dr, A_dr), (rand_layout, _) = by_hand(config, ref_rand, sources)
    bounds = []
    assert len(with_dr) == 2 and len(dd_only) == 2
    for s, (cf_t, cf_x, cf_boost) in enumerate(with_dr):
        assert cf_t.dd == dd_only[s][0].dd and dd_only[s][0].dr is None
        sampled = cf_t.dd.sample_patch_sum()
        assert sampled.samples.shape == (3, 3) and np.all(W_dd[s].sum(axis=(1, 2)) > 0)
        (t_tot, t_jk), (w_tot, w_jk), (a_tot, a_jk) = jackknife(T_dd[s]), jackknife(W_dd[s]), jackknife(A_dd[s])
        bounds.append(ratio_bound(t_tot, w_tot, a_tot, device))
        err = np.abs(sampled.data - K * t_tot / w_tot)
        print(f"{unit} scale {s}: Delta Sigma = {sampled.data}, |ours - by hand| / bound = {err / bounds[-1]}")
        assert np.all(err <= bounds[-1])
        assert np.all(np.abs(sampled.samples - K * t_jk / w_jk) <= ratio_bound(t_jk, w_jk, a_jk, device))
        np.testing.assert_allclose(cf_t.dd.number_counts.counts, W_dd[s], rtol=rtol_w, atol=0)
        assert np.array_equal(cf_t.dd.number_counts.counts, cf_x.dd.number_counts.counts)
        assert np.all(sampled.data > 0)  # a tangential pattern around the lenses
        (r_tot, r_jk), (rw_tot, rw_jk), (ra_tot, ra_jk) = jackknife(T_dr[s]), jackknife(W_dr[s]), jackknife(A_dr[s])
        rand = cf_t.dr.sample_patch_sum()
        assert np.all(np.abs(rand.data - K * r_tot / rw_tot) <= ratio_bound(r_tot, rw_tot, ra_tot, device))
        assert np.all(np.abs(rand.samples - K * r_jk / rw_jk) <= ratio_bound(r_jk, rw_jk, ra_jk, device))
        assert np.array_equal(cf_t.sample().data, sampled.data - rand.data)
        # the boost factor: the W planes over (lens weight sums per (patch, bin)) x (source patch totals), DD / DR - 1
        assert type(cf_boost) is yaw.CorrFunc
        assert np.array_equal(cf_boost.dd.counts.counts, cf_t.dd.number_counts.counts)
        assert np.array_equal(cf_boost.dr.counts.counts, cf_t.dr.number_counts.counts)
        ratio = []
        for W, layout in ((W_dd[s], lens_layout), (W_dr[s], rand_layout)):
            lens_sums = np.array([[layout.w[lo:hi].sum() if layout.w is not None else float(hi - lo)
                                   for lo, hi in zip(layout.offsets[p * 3:p * 3 + 3], layout.offsets[p * 3 + 1:p * 3 + 4])]
                                  for p in range(3)]).T  # [B, P]
            source_sums = np.array([source_layout.w[lo:hi].sum() for lo, hi in zip(source_layout.offsets[:-1], source_layout.offsets[1:])])
            norm = lens_sums[:, :, None] * source_sums[None, None, :]  # [B, P, P]
            (c_tot, c_jk), (n_tot, n_jk) = jackknife(W), jackknife(norm)
            ratio.append((c_tot / n_tot, c_jk / n_jk))
        boost = cf_boost.sample()
        rtol_b = 1e-11 + (2.0 * 1e-10 * (1.0 + 1e-9) if device else 0.0)
        np.testing.assert_allclose(boost.data + 1.0, ratio[0][0] / ratio[1][0], rtol=rtol_b, atol=0)
        np.testing.assert_allclose(boost.samples + 1.0, ratio[0][1] / ratio[1][1], rtol=rtol_b, atol=0)
    return with_dr, bounds


def check_shear_scenario(device=False):
    """``crosscorrelate_shear(radius="lens")`` on sources WITHOUT redshifts: ``sum T / sum W`` of the count with ``f = 1``,
    ``c = 0``, ``u = 0``, by hand. On the device ``|T' - T| <= 1e-10 A`` and ``|W' / W - 1| <= 1e-10`` (``ratio_bound`` with
    the unit ``K`` divided out)."""
    _, reference, sources, ref_rand = dsigma_scenario(with_randoms=True, source_redshifts=False)
    config = scenario_config("kpc")
    result = yaw.crosscorrelate_shear(config, reference, sources, ref_rand=ref_rand, radius="lens")
    (T_dd, W_dd, A_dd), _ = by_hand(config, reference, sources, shear_only=True)
    (T_dr, W_dr, A_dr), _ = by_hand(config, ref_rand, sources, shear_only=True)
    for s, (cf_t, cf_x) in enumerate(result):
        for counts, (T, W, A) in ((cf_t.dd, (T_dd[s], W_dd[s], A_dd[s])), (cf_t.dr, (T_dr[s], W_dr[s], A_dr[s]))):
            (t_tot, t_jk), (w_tot, w_jk), (a_tot, a_jk) = jackknife(T), jackknife(W), jackknife(A)
            sampled = counts.sample_patch_sum()
            assert np.all(w_tot > 0)
            assert np.all(np.abs(sampled.data - t_tot / w_tot) <= ratio_bound(t_tot, w_tot, a_tot, device) / K)
            assert np.all(np.abs(sampled.samples - t_jk / w_jk) <= ratio_bound(t_jk, w_jk, a_jk, device) / K)
            np.testing.assert_allclose(counts.number_counts.counts, W, rtol=1e-10 if device else 1e-13, atol=0)
        assert np.all(cf_t.dd.sample_patch_sum().data > 0)
    return result


@pytest.mark.parametrize("unit", ["kpc", "Mpc/h"])
def test_delta_sigma_driver_on_the_oracle_stand_in(stand_in, unit):
    check_radial_scenario(unit)


def test_shear_driver_on_the_oracle_stand_in(stand_in):
    check_shear_scenario()


def test_comoving_units_use_the_comoving_distance():
    layout = type("L", (), dict(redshifts=np.array([0.2, 0.7])))()
    f, c, m, _ = engine.dsigma_radial_columns(layout, None, COSMO, "Mpc")
    assert np.array_equal(m, f * f)
    m_h = engine.dsigma_radial_columns(layout, None, COSMO, "kpc/h")[2]
    np.testing.assert_allclose(m_h, c * c, rtol=1e-15)  # D_A (1 + z) is the comoving distance of a flat cosmology
    ones, zeros, _, u = engine.dsigma_radial_columns(layout, type("S", (), dict(x=np.zeros(3), redshifts=None))(), COSMO, "Mpc", unit_columns=True)
    assert np.all(ones == 1.0) and np.all(zeros == 0.0) and np.array_equal(u, np.zeros(3))


# --------------------------------------------------------------------------- 5. what the feature is for
RING_R = 320.0  # kpc


def ring_scenario():
    """Two lenses at z = 0.15 and z = 0.9, the two ends of ONE redshift slice 0.1 < z < 1.0 (middle 0.55), 10 degrees apart
    in patches of their own, each with 200 sources on a ring of physical radius 320 kpc around it. Three scales: 100 - 300,
    300 - 600 and 600 - 1500 kpc."""
    rng = np.random.default_rng(5)
    config = yaw.Configuration.create(rmin=[100.0, 300.0, 600.0], rmax=[300.0, 600.0, 1500.0], unit="kpc", edges=np.array([0.1, 1.0]))
    centers = yaw.AngularCoordinates(np.array(CENTERS[:2]))
    lens_z = np.array([0.15, 0.9])
    ra, dec = [], []
    for (ra_c, dec_c), z in zip(CENTERS[:2], lens_z):
        theta = RING_R / 1000.0 / float(COSMO.angular_diameter_distance(z))
        r, d = ring_around(rng, ra_c, dec_c, 200, theta * (1.0 - 1e-3), theta * (1.0 + 1e-3))
        ra.append(r), dec.append(d)
    ra, dec = np.concatenate(ra), np.concatenate(dec)
    g1, g2 = shear_oracle.tangential_pattern(ra, dec, np.repeat([c[0] for c in CENTERS[:2]], 200), np.repeat([c[1] for c in CENTERS[:2]], 200), 0.02)
    kw = dict(patch_centers=centers, degrees=False)
    sources = yaw.Catalog.from_arrays(ra, dec, redshifts=np.full(len(ra), 1.5), g1=g1, g2=g2, **kw)
    reference = yaw.Catalog.from_arrays(np.array([c[0] for c in CENTERS[:2]]), np.array([c[1] for c in CENTERS[:2]]), redshifts=lens_z, **kw)
    return config, reference, sources


def test_both_rings_land_in_the_bin_that_names_their_radius(stand_in):
    """The feature: with ``radius="lens"`` the sources 320 kpc from their lens are all in the scale 300 - 600 kpc, whichever end
    of the slice the lens sits at. With ``radius="slice"`` the near lens's ring is counted at 783 kpc and the far one's at
    264 kpc: in two other bins, and none in the one that names its radius."""
    config, reference, sources = ring_scenario()
    per_lens = yaw.crosscorrelate_delta_sigma(config, reference, sources, radius="lens")
    per_slice = yaw.crosscorrelate_delta_sigma(config, reference, sources)  # radius="slice"
    pairs = lambda result: [np.count_nonzero(cf_t.dd.number_counts.counts, axis=0) for cf_t, _ in result]  # [S][P, P]
    assert [p.tolist() for p in pairs(per_lens)] == [[[0, 0], [0, 0]], [[1, 0], [0, 1]], [[0, 0], [0, 0]]]
    assert [p.tolist() for p in pairs(per_slice)] == [[[0, 0], [0, 1]], [[0, 0], [0, 0]], [[1, 0], [0, 0]]]
    # every source counts, once: W of the per-lens count is the sum over both rings, split over two bins by the other
    total = lambda result: sum(cf_t.dd.number_counts.counts.sum() for cf_t, _ in result)
    assert total(per_lens) == pytest.approx(total(per_slice), rel=1e-12)
    shear = yaw.crosscorrelate_shear(config, reference, sources, radius="lens")
    assert [cf_t.dd.number_counts.counts.sum() for cf_t, _ in shear] == [0.0, 400.0, 0.0]
    assert shear[1][0].dd.sample_patch_sum().data[0] == pytest.approx(0.02, rel=1e-9)


def test_lenses_at_the_middle_of_their_slice_give_the_same_in_both_modes(stand_in):
    """Every lens exactly at its slice's middle redshift: there the two modes name the same pairs, as long as no pair lies
    within 1e-9 (relative, in R^2) of an edge -- the two tables of edges differ by their rounding. The scene is checked
    with the oracle; the two modes then agree to 1e-12 per slot."""
    _, reference, sources, ref_rand = dsigma_scenario(with_randoms=True)
    config = scenario_config("kpc")
    mids = np.asarray(config.binning.binning.mids)
    rng = np.random.default_rng(3)
    ra, dec = [], []
    for ra_c, dec_c in CENTERS:
        r, d = ring_around(rng, ra_c, dec_c, 6, 0.05 * ARCMIN, 1.0 * ARCMIN)
        ra.append(r), dec.append(d)
    reference = yaw.Catalog.from_arrays(np.concatenate(ra), np.concatenate(dec), redshifts=np.tile(np.repeat(mids, 2), 3),
                                        weights=rng.uniform(0.5, 1.5, 18), patch_centers=yaw.AngularCoordinates(np.array(CENTERS)), degrees=False)
    lens_layout = reference.build_trees(config.binning.edges, closed=config.binning.closed, with_redshifts=True)
    source_layout = sources.build_trees(None, with_redshifts=True)
    assert np.array_equal(np.unique(lens_layout.redshifts), mids)
    jobs = np.array([(p, q) for p in range(3) for q in range(3)])
    f, c, m, u = engine.dsigma_radial_columns(lens_layout, source_layout, COSMO, "kpc")
    lens, src = radial_oracle.as_lens(lens_layout, f, c, m), radial_oracle.as_sources(source_layout, u)
    r2 = measurements.threshold_table(measurements.radial_plans(config))
    margin = radial_oracle.nearest_margin(lens, src, jobs, r2)
    # ... and the same pairs against the chord thresholds of the slice: no squared chord within 1e-9 of one
    t = measurements.threshold_table(measurements.angular_plans(config))
    # (with m = 1 the oracle's R2 is the squared angle, a monotone function of the squared chord: the edges go through it too)
    margin_t = radial_oracle.nearest_margin(dict(lens, m=np.ones_like(m)), src, jobs, radial_oracle.squared_angle(t))
    print(f"nearest pair to an edge: {margin:.3e} (radii), {margin_t:.3e} (chords)")
    assert margin > 1e-9 and margin_t > 1e-9
    per_lens = yaw.crosscorrelate_delta_sigma(config, reference, sources, ref_rand=None, radius="lens")
    per_slice = yaw.crosscorrelate_delta_sigma(config, reference, sources, ref_rand=None, radius="slice")
    for (lens_t, lens_x), (slice_t, slice_x) in zip(per_lens, per_slice):
        assert np.count_nonzero(lens_t.dd.number_counts.counts) >= 9
        for a, b in ((lens_t, slice_t), (lens_x, slice_x)):
            np.testing.assert_allclose(a.dd.number_counts.counts, b.dd.number_counts.counts, rtol=1e-12, atol=0)
            scale = np.abs(a.dd.kappa_counts.counts).max()
            np.testing.assert_allclose(a.dd.kappa_counts.counts, b.dd.kappa_counts.counts, rtol=1e-12, atol=1e-12 * scale)


# --------------------------------------------------------------------------- 6. error cases
def test_drivers_reject_what_they_cannot_use(stand_in):
    config, reference, sources, ref_rand = dsigma_scenario(with_randoms=True)
    angular = yaw.Configuration.create(rmin=[1.0], rmax=[5.0], unit="arcmin", edges=ZEDGES)
    for driver in (yaw.crosscorrelate_delta_sigma, yaw.crosscorrelate_shear):
        with pytest.raises(ValueError, match="physical or comoving unit"):
            driver(angular, reference, sources, radius="lens")
        with pytest.raises(ValueError, match="'slice' or 'lens'"):
            driver(config, reference, sources, radius="object")
    no_z = yaw.Catalog.from_arrays(np.array([c[0] for c in CENTERS]), np.array([c[1] for c in CENTERS]),
                                   patch_centers=yaw.AngularCoordinates(np.array(CENTERS)), degrees=False)
    with pytest.raises(ValueError, match="redshifts"):
        yaw.crosscorrelate_shear(config, no_z, sources, radius="lens")
    _, _, sources_no_z, _ = dsigma_scenario(source_redshifts=False)
    with pytest.raises(ValueError, match="redshifts"):
        yaw.crosscorrelate_delta_sigma(config, reference, sources_no_z, radius="lens")
    links = yaw.PatchLinkage.from_catalogs(config, reference, sources)
    reference.build_trees(config.binning.edges), sources.build_trees(None)  # layouts without redshifts
    with pytest.raises(ValueError, match="with_redshifts"):
        links.count_dsigma_radial_pairs(reference, sources)


def test_a_lens_too_close_for_the_largest_radius_is_named(stand_in):
    """2 Mpc around a lens at z = 0.002 (8.9 Mpc away) is 13 degrees: beyond the cap, and the error says which lens."""
    config, reference, sources, _ = dsigma_scenario()
    config = yaw.Configuration.create(rmin=[100.0], rmax=[2000.0], unit="kpc", edges=np.array([0.001, 0.35, 0.65]))
    near = yaw.Catalog.from_arrays(np.array([c[0] for c in CENTERS]), np.array([c[1] for c in CENTERS]), redshifts=np.array([0.3, 0.002, 0.5]),
                                   patch_centers=yaw.AngularCoordinates(np.array(CENTERS)), degrees=False)
    for driver in (yaw.crosscorrelate_delta_sigma, yaw.crosscorrelate_shear):
        with pytest.raises(ValueError, match=r"too close for the largest radius.*bin 0 at z = 0\.002 .*R = 2 Mpc"):
            driver(config, near, sources, radius="lens")
    yaw.crosscorrelate_delta_sigma(config, near, sources)  # the slices' own angles are no such problem
    # the randoms count too
    far = yaw.Catalog.from_arrays(np.array([c[0] for c in CENTERS]), np.array([c[1] for c in CENTERS]), redshifts=np.array([0.3, 0.4, 0.5]),
                                  patch_centers=yaw.AngularCoordinates(np.array(CENTERS)), degrees=False)
    with pytest.raises(ValueError, match="too close for the largest radius"):
        yaw.crosscorrelate_delta_sigma(config, far, sources, ref_rand=near, radius="lens")
    # the seam itself refuses as the library does
    layout = near.build_trees(config.binning.edges, with_redshifts=True)
    m = engine.dsigma_radial_columns(layout, None, COSMO, "kpc")[2]
    with pytest.raises(ValueError, match="too close"):
        engine.check_radial_reach(layout, m, np.array([[0.01, 4.0]] * 2))
    smax = engine.check_radial_reach(layout, m, np.array([[0.01, 0.04]] * 2))
    assert smax[0] == pytest.approx(0.04 / m.min(), rel=1e-11) and smax[1] == pytest.approx(0.04 / np.sort(m)[2], rel=1e-11)


def test_the_linkage_reaches_as_far_as_the_nearest_lens(stand_in):
    config, reference, sources, ref_rand = dsigma_scenario(with_randoms=True)
    lens_layout = reference.build_trees(config.binning.edges, with_redshifts=True)
    rand_layout = ref_rand.build_trees(config.binning.edges, with_redshifts=True)
    angle = measurements.radial_max_angle(config, lens_layout, rand_layout)
    d_near = float(COSMO.angular_diameter_distance(0.22))  # the nearest lens; the randoms start at 0.25
    assert angle == pytest.approx(2.0 / d_near, rel=1e-6)
    assert measurements.radial_max_angle(config, rand_layout) < angle
    wide = yaw.PatchLinkage.from_catalogs(config, reference, sources, max_angle=0.5)  # 28 degrees: everything is linked
    assert wide.num_links == 9 and yaw.PatchLinkage.from_catalogs(config, reference, sources).num_links == 3


def test_several_ranks_are_refused(stand_in, monkeypatch):
    from yet_another_wizz_amd import parallel

    monkeypatch.setattr(parallel, "world", lambda: (0, 2))
    config, reference, sources, _ = dsigma_scenario()
    for driver in (yaw.crosscorrelate_delta_sigma, yaw.crosscorrelate_shear):
        with pytest.raises(NotImplementedError):
            driver(config, reference, sources, radius="lens")
