"""CPU: excess surface density around reference slices (``crosscorrelate_delta_sigma``) above the device seam -- the C ABI's
new names, the pair term of the contract on one pair and against the shear oracle, the layouts with redshifts, and the driver
with ``engine.count_dsigma_fine`` replaced by the numpy brute force of tests/dsigma_oracle.py."""
import ctypes
import os
import re
import types

import numpy as np
import pytest

import dsigma_oracle
import shear_oracle
import yet_another_wizz_amd as yaw
from conftest import ARCMIN, ROOT
from test_shear_host import ring_around
from yet_another_wizz_amd import _lib, cosmology, engine, measurements
from yet_another_wizz_amd.catalog import radec_to_xyz

COSMO = cosmology.Planck15
K = cosmology.DELTA_SIGMA_UNIT
SYMBOLS = ("yawhip_dsigma_upload_lenses", "yawhip_dsigma_upload_sources", "yawhip_dsigma_count")


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
    assert "crosscorrelate_delta_sigma" in yaw.__all__


def test_the_unit_constant():
    c, mpc, gm_sun = 299792458.0, 3.085677581491367e22, 1.32712440018e20
    assert K == pytest.approx(c * c * mpc / (4.0 * np.pi * gm_sun) * 1e-12, rel=1e-15)
    assert K == pytest.approx(1.6629e6, rel=1e-4)


# --------------------------------------------------------------------------- 2. one pair
def one_pair(z_l, z_s, gamma=0.01, w_l=1.7, w_s=0.6):
    """One lens on the equator and one source 3 arcmin due east of it with ``g1 = -gamma`` (a stretch along north-south:
    tangential to the lens): the oracle's planes, with the three columns made by the engine's helper."""
    ra_l = 0.7
    lens_xyz = radec_to_xyz(np.array([ra_l]), np.array([0.0]))
    src_xyz = radec_to_xyz(np.array([ra_l + 3.0 * ARCMIN]), np.array([0.0]))
    layouts = [types.SimpleNamespace(redshifts=np.array([z])) for z in (z_l, z_s)]
    f, c, u = engine.dsigma_columns(*layouts, COSMO)
    lens = dict(zip("xyz", lens_xyz), w=np.array([w_l]), f=f, c=c, nb=1, off=np.array([0, 1]))
    src = dict(zip("xyz", src_xyz), w=np.array([w_s]), g1=np.array([-gamma]), g2=np.array([0.0]), u=u, off=np.array([0, 1]))
    t = (2.0 * np.sin(0.5 * np.array([[1.0, 5.0]]) * ARCMIN)) ** 2
    return dsigma_oracle.dsigma_jobs(lens, src, [[0, 0]], t)[:3]


@pytest.mark.parametrize("z_l, z_s", [(0.3, 0.8), (0.05, 3.0), (0.6, 0.61)])
def test_one_pair_gives_gamma_times_sigma_crit(z_l, z_s):
    gamma = 0.01
    T, X, W = one_pair(z_l, z_s, gamma)
    expected = gamma * dsigma_oracle.sigma_crit(COSMO, z_l, z_s)
    assert W[0, 0, 0] > 0 and np.isfinite(expected)
    assert K * T[0, 0, 0] / W[0, 0, 0] == pytest.approx(expected, rel=1e-12)
    assert abs(X[0, 0, 0]) <= 1e-12 * abs(T[0, 0, 0])


@pytest.mark.parametrize("z_l, z_s", [(0.8, 0.3), (0.5, 0.5)], ids=["in front", "same redshift"])
def test_a_source_not_behind_its_lens_adds_nothing(z_l, z_s):
    for plane in one_pair(z_l, z_s):
        assert np.all(plane == 0.0)


# --------------------------------------------------------------------------- 3. reduction to the shear count
@pytest.mark.parametrize("source_weights", ["none", "powers of two"])
def test_unit_columns_reduce_to_the_shear_oracle(source_weights):
    """``f = 1, c = 0`` and any ``u``: the planes of tests/shear_oracle.py, bit for bit. The shear oracle multiplies the shear
    by ``w_l * w_s`` where the contract (and this oracle) multiply ``w_s * g`` by ``w_l``: the two round alike where ``w_s``
    is a power of two or absent, which is what this test draws; the lens weights are arbitrary."""
    rng = np.random.default_rng(3)
    n_l, n_s = 90, 400
    ra_l, dec_l = rng.uniform(0.30, 0.303, n_l), rng.uniform(0.1, 0.103, n_l)
    ra_s, dec_s = rng.uniform(0.30, 0.303, n_s), rng.uniform(0.1, 0.103, n_s)
    lens = dict(zip("xyz", radec_to_xyz(ra_l, dec_l)), w=rng.uniform(0.5, 2.0, n_l), nb=3, off=np.array([0, 20, 50, 50, 60, 90, 90]))
    sw = None if source_weights == "none" else 2.0 ** rng.integers(-2, 3, n_s)
    src = dict(zip("xyz", radec_to_xyz(ra_s, dec_s)), w=sw, g1=rng.normal(0, 0.3, n_s), g2=rng.normal(0, 0.3, n_s),
               off=np.array([0, 150, n_s]))
    t = (2.0 * np.sin(0.5 * np.array([np.geomspace(0.5 + 0.1 * k, 9.0, 8) for k in range(3)]) * ARCMIN)) ** 2
    jobs = [[0, 0], [0, 1], [1, 0], [1, 1]]
    exp = shear_oracle.shear_jobs(lens, src, jobs, t)
    got = dsigma_oracle.dsigma_jobs(dict(lens, f=np.ones(n_l), c=np.zeros(n_l)), dict(src, u=rng.uniform(0.0, 5.0, n_s)), jobs, t)
    assert np.count_nonzero(exp[2]) > 40
    for a, b in zip(got, exp):
        assert np.array_equal(a, b)


# --------------------------------------------------------------------------- 4. layouts with redshifts
def test_layouts_carry_the_redshifts_in_their_order():
    rng = np.random.default_rng(8)
    n = 500
    ra, dec = rng.uniform(0.1, 0.3, n), rng.uniform(-0.1, 0.1, n)
    z = 0.1 + 0.9 * (ra - 0.1) / 0.2 + 0.01 * dec  # a function of the position: alignment is checkable per object
    cat = yaw.Catalog.from_arrays(ra, dec, redshifts=z, g1=ra, g2=dec, patch_ids=rng.integers(0, 4, n), degrees=False)
    edges = np.array([0.2, 0.5, 0.7, 0.95])
    plain_binned, plain_unbinned = cat.build_trees(edges), cat.build_trees(None)
    for bins, plain in ((edges, plain_binned), (None, plain_unbinned)):
        layout = cat.build_trees(bins, with_redshifts=True)
        assert layout is not plain and plain.redshifts is None
        assert cat.build_trees(bins) is plain and cat.build_trees(bins, with_redshifts=True) is layout  # both stay cached
        ra_of = np.arctan2(layout.y, layout.x)
        dec_of = np.arcsin(layout.z)
        np.testing.assert_allclose(layout.redshifts, 0.1 + 0.9 * (ra_of - 0.1) / 0.2 + 0.01 * dec_of, rtol=0, atol=1e-12)
        assert np.array_equal(layout.offsets, plain.offsets) and np.array_equal(layout.x, plain.x)
        if bins is not None:
            k = np.repeat(np.tile(np.arange(3), 4), np.diff(layout.offsets))
            assert np.all(layout.redshifts > edges[k]) and np.all(layout.redshifts <= edges[k + 1])
            assert layout.g1 is None
        else:
            assert np.array_equal(layout.g1, plain.g1)
    without = yaw.Catalog.from_arrays(ra, dec, patch_ids=np.zeros(n, dtype=int), degrees=False)
    with pytest.raises(ValueError, match="redshifts"):
        without.build_trees(None, with_redshifts=True)


def test_distance_column_calls_the_cosmology_in_chunks():
    z = np.linspace(0.0, 2.0, 1001)
    chi = cosmology.distance_column(COSMO, z, chunksize=64)
    assert np.array_equal(chi, COSMO.comoving_distance(z)) and chi[0] == 0.0
    assert np.array_equal(cosmology.distance_column(COSMO, z, kind="angular", chunksize=1000), COSMO.angular_diameter_distance(z))

    class Custom(cosmology.CustomCosmology):  # used as given
        calls = 0

        def comoving_distance(self, z):
            Custom.calls += 1
            return 3000.0 * np.asarray(z)

        def angular_diameter_distance(self, z):
            return self.comoving_distance(z) / (1.0 + np.asarray(z))

    assert np.array_equal(cosmology.distance_column(Custom(), z, chunksize=100), 3000.0 * z) and Custom.calls == 11


# --------------------------------------------------------------------------- 5. the driver on the oracle stand-in
CENTERS = ((0.30, 0.10), (0.30 + np.deg2rad(10.0), 0.12), (0.30 + np.deg2rad(20.0), 0.08))  # three patches 10 degrees apart
ZEDGES = np.array([0.2, 0.35, 0.5, 0.65])


def dsigma_scenario(with_randoms=False, shear=True, source_redshifts=True):
    """Three patches, three redshift bins. Per patch six lenses within 1 arcmin of its centre, two per bin, and 300 sources
    at 0.2' - 14' around it with redshifts 0.1 - 1.2 (about a third in front of a lens at 0.5), a tangential pattern around
    the centre plus noise. Scales in kpc: every bin has its own angles. ``(config, reference, sources, ref_rand | None)``."""
    rng = np.random.default_rng(17)
    centers = yaw.AngularCoordinates(np.array(CENTERS))
    kw = dict(patch_centers=centers, degrees=False)
    ra, dec, g1, g2, lra, ldec, rra, rdec = ([] for _ in range(8))
    for ra_c, dec_c in CENTERS:
        r, d = ring_around(rng, ra_c, dec_c, 300, 0.2 * ARCMIN, 14.0 * ARCMIN)
        a, b = shear_oracle.tangential_pattern(r, d, ra_c, dec_c, 0.03)
        ra.append(r), dec.append(d), g1.append(a + rng.normal(0, 0.02, 300)), g2.append(b + rng.normal(0, 0.02, 300))
        r, d = ring_around(rng, ra_c, dec_c, 6, 0.05 * ARCMIN, 1.0 * ARCMIN)
        lra.append(r), ldec.append(d)
        r, d = ring_around(rng, ra_c, dec_c, 9, 0.5 * ARCMIN, 4.0 * ARCMIN)
        rra.append(r), rdec.append(d)
    ra, dec, g1, g2, lra, ldec, rra, rdec = (np.concatenate(c) for c in (ra, dec, g1, g2, lra, ldec, rra, rdec))
    extra = dict(g1=g1, g2=g2) if shear else {}
    if source_redshifts:
        extra["redshifts"] = rng.uniform(0.1, 1.2, len(ra))
    sources = yaw.Catalog.from_arrays(ra, dec, weights=rng.uniform(0.5, 1.5, len(ra)), **extra, **kw)
    lens_z = np.tile([0.22, 0.33, 0.38, 0.47, 0.55, 0.64], 3)
    reference = yaw.Catalog.from_arrays(lra, ldec, redshifts=lens_z, weights=rng.uniform(0.5, 1.5, len(lra)), **kw)
    ref_rand = yaw.Catalog.from_arrays(rra, rdec, redshifts=np.tile([0.25, 0.4, 0.6], 9), **kw) if with_randoms else None
    config = yaw.Configuration.create(rmin=[100.0, 300.0], rmax=[2000.0, 1000.0], unit="kpc", rweight=-0.8, resolution=12,
                                      edges=ZEDGES)
    return config, reference, sources, ref_rand


def by_hand(config, lenses, sources):
    """``sum T``, ``sum W`` and the magnitude ``sum A`` per scale, bin and patch pair [S, B, P, P] from the oracle's fine planes
    and a ``CombinePlan`` (its separation weights are positive: the combined ``A`` bounds the combined ``T`` as before)."""
    plans = measurements.angular_plans(config)
    thresholds = measurements.threshold_table(plans)
    lens_layout = lenses.build_trees(config.binning.edges, closed=config.binning.closed, with_redshifts=True)
    source_layout = sources.build_trees(None, with_redshifts=True)
    jobs = np.array([(p, q) for p in range(3) for q in range(3)])
    f, c, u = engine.dsigma_columns(lens_layout, source_layout, config.cosmology)
    T, _, W, A = dsigma_oracle.dsigma_jobs(dsigma_oracle.as_lens(lens_layout, f, c), dsigma_oracle.as_sources(source_layout, u), jobs,
                                           thresholds)
    combine = measurements.CombinePlan(plans)
    out = []
    for fine in (T, W, A):
        per_scale = combine(np.moveaxis(fine, 0, -1))  # [S, B, J]
        out.append(per_scale.reshape(per_scale.shape[0], per_scale.shape[1], 3, 3))
    return out, (lens_layout, source_layout)


def jackknife(arr):
    """[B, P, P] -> the total [B] and the leave-one-patch-out sums [P, B], written out."""
    total = arr.sum(axis=(1, 2))
    samples = np.array([arr[:, keep][:, :, keep].sum(axis=(1, 2))
                        for keep in (np.flatnonzero(np.arange(arr.shape[1]) != i) for i in range(arr.shape[1]))])
    return total, samples


DEVICE_RTOL_W = 1e-10  # tests/helpers.RTOL_W: the project's tolerance of a weighted pair count
DEVICE_RTOL_A = 1e-10  # ... and of a signed sum, relative to its cancellation-free magnitude A


def ratio_bound(T, W, A, device):
    """How far ``K T' / W'`` may lie from the oracle's ``K T / W``. On the stand-in the sums are the oracle's and only the host's
    few roundings differ (1e-12 relative). On the device ``|T' - T| <= 1e-10 A`` and ``|W' / W - 1| <= 1e-10``, the project's
    tolerances, so the ratio moves by at most ``(1e-10 A + 1e-10 |T|) / W`` to first order (1e-9 of that for the second)."""
    host = 1e-12 * np.abs(K * T / W)
    return host + (K * (DEVICE_RTOL_A * A + DEVICE_RTOL_W * np.abs(T)) / W * (1.0 + 1e-9) if device else 0.0)


def check_dsigma_scenario(device=False):
    """The assertions of the scenario; ``engine.count_dsigma_fine`` is whatever the caller left in place: the stand-in
    (``device=False``: the oracle's sums, held to the host's rounding) or the library (``device=True``: the project's device
    tolerances, ``ratio_bound``). Returns the driver's results and the bounds of ``Delta Sigma`` per scale."""
    config, reference, sources, ref_rand = dsigma_scenario(with_randoms=True)
    dd_only = yaw.crosscorrelate_delta_sigma(config, reference, sources)
    (T_dd, W_dd, A_dd), (lens_layout, source_layout) = by_hand(config, reference, sources)
    rtol_w = DEVICE_RTOL_W if device else 1e-13
    bounds = []
    assert len(dd_only) == 2
    for s, (cf_t, cf_x) in enumerate(dd_only):
        assert type(cf_t) is yaw.ScalarCorrFunc and type(cf_x) is yaw.ScalarCorrFunc and cf_t.dr is None and cf_x.dr is None
        sampled = cf_t.sample()
        assert sampled.samples.shape == (3, 3) and np.all(W_dd[s].sum(axis=(1, 2)) > 0)
        (t_tot, t_jk), (w_tot, w_jk), (a_tot, a_jk) = jackknife(T_dd[s]), jackknife(W_dd[s]), jackknife(A_dd[s])
        bounds.append(ratio_bound(t_tot, w_tot, a_tot, device))
        err = np.abs(sampled.data - K * t_tot / w_tot)
        print(f"scale {s}: Delta Sigma = {sampled.data}, |ours - by hand| / bound = {err / bounds[-1]}")
        assert np.all(err <= bounds[-1])
        assert np.all(np.abs(sampled.samples - K * t_jk / w_jk) <= ratio_bound(t_jk, w_jk, a_jk, device))
        np.testing.assert_allclose(cf_t.dd.number_counts.counts, W_dd[s], rtol=rtol_w, atol=0)
        assert np.array_equal(cf_t.dd.number_counts.counts, cf_x.dd.number_counts.counts)
        assert np.all(sampled.data > 0)  # a tangential pattern around the lenses

    with_dr = yaw.crosscorrelate_delta_sigma(config, reference, sources, ref_rand=ref_rand, boost=True)
    (T_dr, W_dr, A_dr), (rand_layout, _) = by_hand(config, ref_rand, sources)
    for s, (cf_t, cf_x, cf_boost) in enumerate(with_dr):
        assert cf_t.dd == dd_only[s][0].dd and cf_x.dd == dd_only[s][1].dd
        for cf in (cf_t, cf_x):
            assert np.array_equal(cf.sample().data, cf.dd.sample_patch_sum().data - cf.dr.sample_patch_sum().data)
        t_tot, w_tot, a_tot = (plane[s].sum(axis=(1, 2)) for plane in (T_dr, W_dr, A_dr))
        assert np.all(np.abs(cf_t.dr.sample_patch_sum().data - K * t_tot / w_tot) <= ratio_bound(t_tot, w_tot, a_tot, device))
        # the boost factor: the W planes over (lens weight sums per (patch, bin)) x (source patch totals), DD / DR - 1
        assert type(cf_boost) is yaw.CorrFunc and cf_boost.rr is None and cf_boost.rd is None
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
        rtol_b = 1e-11 + (2.0 * DEVICE_RTOL_W * (1.0 + 1e-9) if device else 0.0)  # DD / DR: each within rtol_w
        np.testing.assert_allclose(boost.data + 1.0, ratio[0][0] / ratio[1][0], rtol=rtol_b, atol=0)
        np.testing.assert_allclose(boost.samples + 1.0, ratio[0][1] / ratio[1][1], rtol=rtol_b, atol=0)
        assert np.all(np.isfinite(boost.data))
    plain = yaw.crosscorrelate_delta_sigma(config, reference, sources, ref_rand=ref_rand)
    assert all(len(item) == 2 for item in plain) and plain[0][0] == with_dr[0][0]
    return with_dr, bounds


def test_driver_on_the_oracle_stand_in(monkeypatch):
    monkeypatch.setattr(engine, "count_dsigma_fine", dsigma_oracle.count_dsigma_fine)
    check_dsigma_scenario()


# --------------------------------------------------------------------------- 6. a singular isothermal sphere
SIS_SIGMA_V = 250.0  # km / s
SIS_RMIN, SIS_RMAX = (100.0, 400.0), (1500.0, 800.0)  # kpc


def sis_scenario():
    """One lens at the middle of the one redshift bin; 4000 sources at 0.1 - 3 Mpc from it and redshifts 0.05 - 1.5, each
    with the tangential shear ``Delta Sigma_SIS(R) / Sigma_c(z_l, z_s)`` of its own distance and redshift; the sources in front
    of the lens carry a shear of 0.5 that must not be seen."""
    rng = np.random.default_rng(23)
    config = yaw.Configuration.create(rmin=list(SIS_RMIN), rmax=list(SIS_RMAX), unit="kpc", edges=np.array([0.2, 0.4]))
    z_l = float(config.binning.binning.mids[0])
    d_l = float(COSMO.angular_diameter_distance(z_l))  # Mpc
    ra_l, dec_l = 1.1, -0.4
    ra, dec = ring_around(rng, ra_l, dec_l, 4000, 0.1 / d_l, 3.0 / d_l)
    z_s = rng.uniform(0.05, 1.5, len(ra))
    (lx,), (ly,), (lz,) = radec_to_xyz(np.array([ra_l]), np.array([dec_l]))
    sx, sy, sz = radec_to_xyz(ra, dec)
    theta = 2.0 * np.arcsin(0.5 * np.sqrt((sx - lx) ** 2 + (sy - ly) ** 2 + (sz - lz) ** 2))
    behind = z_s > z_l
    with np.errstate(divide="ignore"):
        gamma_t = np.where(behind, dsigma_oracle.sis_delta_sigma(SIS_SIGMA_V, theta * d_l) / dsigma_oracle.sigma_crit(COSMO, z_l, z_s), 0.5)
    assert 0.2 < behind.mean() < 0.9 and np.all(gamma_t[behind] < 0.5)
    g1, g2 = shear_oracle.tangential_pattern(ra, dec, ra_l, dec_l, gamma_t)
    kw = dict(patch_ids=np.zeros(len(ra), dtype=int), degrees=False)
    sources = yaw.Catalog.from_arrays(ra, dec, redshifts=z_s, g1=g1, g2=g2, weights=rng.uniform(0.5, 1.5, len(ra)), **kw)
    reference = yaw.Catalog.from_arrays(np.array([ra_l]), np.array([dec_l]), redshifts=np.array([z_l]), patch_ids=np.zeros(1, dtype=int),
                                        degrees=False)
    return config, reference, sources, z_l


def check_sis_scenario():
    config, reference, sources, z_l = sis_scenario()
    d_l = float(COSMO.angular_diameter_distance(z_l))
    theta_min, theta_max = config.scales.scales.get_angle_radian(z_l, cosmology=config.cosmology)
    for s, (cf_t, cf_x) in enumerate(yaw.crosscorrelate_delta_sigma(config, reference, sources)):
        estimate = cf_t.sample().data[0]
        lo, hi = (dsigma_oracle.sis_delta_sigma(SIS_SIGMA_V, theta * d_l) for theta in (theta_max[s], theta_min[s]))
        print(f"scale {s}: Delta Sigma = {estimate:.4f} M_sun/pc^2 inside [{lo:.4f}, {hi:.4f}]")
        assert lo <= estimate <= hi
        assert abs(cf_x.sample().data[0]) <= 1e-9 * estimate
        assert np.count_nonzero(cf_t.dd.number_counts.counts) == 1


def test_a_singular_isothermal_sphere_is_recovered(monkeypatch):
    monkeypatch.setattr(engine, "count_dsigma_fine", dsigma_oracle.count_dsigma_fine)
    check_sis_scenario()


# --------------------------------------------------------------------------- 7. error cases
def test_driver_rejects_what_it_cannot_use(monkeypatch):
    monkeypatch.setattr(engine, "count_dsigma_fine", dsigma_oracle.count_dsigma_fine)
    config, reference, sources, ref_rand = dsigma_scenario(with_randoms=True, shear=False)
    with pytest.raises(ValueError, match="catalog has no 'g1'/'g2' attached"):
        yaw.crosscorrelate_delta_sigma(config, reference, sources)
    config, reference, sources, ref_rand = dsigma_scenario(with_randoms=True, source_redshifts=False)
    with pytest.raises(ValueError, match="redshifts"):
        yaw.crosscorrelate_delta_sigma(config, reference, sources)
    config, reference, sources, ref_rand = dsigma_scenario(with_randoms=True)
    with pytest.raises(ValueError, match="ref_rand"):
        yaw.crosscorrelate_delta_sigma(config, reference, sources, boost=True)
    with pytest.raises(ValueError, match="separate Catalog instance"):
        yaw.crosscorrelate_delta_sigma(config, reference, reference)
    with pytest.raises(ValueError, match="separate Catalog instance"):
        yaw.crosscorrelate_delta_sigma(config, reference, sources, ref_rand=sources)
    links = yaw.PatchLinkage.from_catalogs(config, reference, sources)
    reference.build_trees(config.binning.edges), sources.build_trees(None)  # layouts without redshifts
    with pytest.raises(ValueError, match="with_redshifts"):
        links.count_dsigma_pairs(reference, sources)


def test_several_ranks_are_refused(monkeypatch):
    from yet_another_wizz_amd import parallel

    monkeypatch.setattr(engine, "count_dsigma_fine", dsigma_oracle.count_dsigma_fine)
    monkeypatch.setattr(parallel, "world", lambda: (0, 2))
    config, reference, sources, _ = dsigma_scenario()
    with pytest.raises(NotImplementedError):
        yaw.crosscorrelate_delta_sigma(config, reference, sources)


def test_columns_refuse_redshifts_and_distances_out_of_range():
    good = types.SimpleNamespace(redshifts=np.array([0.2, 0.5]))
    f, c, u = engine.dsigma_columns(good, good, COSMO)
    np.testing.assert_allclose(f * (1.0 + good.redshifts), c, rtol=1e-15)
    np.testing.assert_allclose(u * c, 1.0, rtol=1e-15)
    assert engine.dsigma_columns(types.SimpleNamespace(redshifts=np.array([0.0])), None, COSMO)[:2] == (0.0, 0.0)  # a lens at z = 0 is fine
    for bad in (np.array([0.2, -0.1]), np.array([np.nan, 0.3]), np.array([0.3, np.inf])):
        layout = types.SimpleNamespace(redshifts=bad)
        with pytest.raises(ValueError, match="finite and >= 0"):
            engine.dsigma_columns(layout, None, COSMO)
        with pytest.raises(ValueError, match="finite and >= 0"):
            engine.dsigma_columns(None, layout, COSMO)
    with pytest.raises(ValueError, match="comoving distance > 0"):
        engine.dsigma_columns(None, types.SimpleNamespace(redshifts=np.array([0.4, 0.0])), COSMO)
    with pytest.raises(ValueError, match="with_redshifts"):
        engine.dsigma_columns(types.SimpleNamespace(redshifts=None), None, COSMO)
