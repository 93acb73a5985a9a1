"""CPU: tangential shear in redshift slices (``crosscorrelate_shear``) above the device seam -- the projection of the
contract against spherical trigonometry, the shear columns of a catalogue, and the driver with ``engine.count_shear_fine``
replaced by the numpy brute force of tests/shear_oracle.py."""
import numpy as np
import pytest

import shear_oracle
import yet_another_wizz_amd as yaw
from conftest import ARCMIN
from yet_another_wizz_amd import catalog as catalog_module
from yet_another_wizz_amd import engine
from yet_another_wizz_amd.catalog import radec_to_xyz


def ring_around(rng, ra_l, dec_l, n, rmin, rmax, log_uniform=False):
    """``n`` points (ra, dec, radian) at separations rmin .. rmax (radian; uniform, or uniform in the logarithm) and any
    direction around (ra_l, dec_l)."""
    r = np.exp(rng.uniform(np.log(rmin), np.log(rmax), n)) if log_uniform else rng.uniform(rmin, rmax, n)
    theta = rng.uniform(0.0, 2.0 * np.pi, n)
    lens = np.array([np.cos(dec_l) * np.cos(ra_l), np.cos(dec_l) * np.sin(ra_l), np.sin(dec_l)])
    east = np.array([-np.sin(ra_l), np.cos(ra_l), 0.0])
    north = np.cross(lens, east)
    xyz = (np.cos(r)[:, None] * lens + np.sin(r)[:, None] * (np.cos(theta)[:, None] * east + np.sin(theta)[:, None] * north))
    return np.arctan2(xyz[:, 1], xyz[:, 0]) % (2.0 * np.pi), np.arcsin(np.clip(xyz[:, 2], -1.0, 1.0))


# --------------------------------------------------------------------------- 1. the projection
ARCSEC = ARCMIN / 60.0
DEC_EXTREME = 89.99 * np.pi / 180.0
RA_WRAP = 2.0 * np.pi - 1e-7  # partners on both sides of the wrap


def rotation_bound(x, y, z, lx, ly, lz):
    """The per-pair bound ``K * eps / theta`` on ``c2`` and ``s2p`` (``K`` and ``eps`` are those of
    tests/shear_exact.py, measured by tools/make_golden_shear_exact.py), ``theta`` the pair's separation in radian."""
    import shear_exact

    theta = 2.0 * np.arcsin(0.5 * np.sqrt((x - lx) ** 2 + (y - ly) ** 2 + (z - lz) ** 2))
    return float(shear_exact.fixture()["K"]) * shear_exact.EPS / theta


def reference_angle(ra, dec, ra_l, dec_l):
    """``shear_oracle.position_angle`` in extended precision where the platform has it: at arcseconds the float64 bearing
    has an error of the size of the one it is to measure (its ``north`` cancels to ``theta``)."""
    return shear_oracle.position_angle(*(np.asarray(v, dtype=np.longdouble) for v in (ra, dec, ra_l, dec_l)))


def check_projection(rng, ra_l, dec_l, rmin, rmax, log_uniform):
    """``c2`` and ``s2p`` of 5000 sources ``rmin .. rmax`` around the lens against the spherical position angle, pair by pair
    within ``rotation_bound`` -> the sources and the lens."""
    ra, dec = ring_around(rng, ra_l, dec_l, 5000, rmin, rmax, log_uniform=log_uniform)
    x, y, z = radec_to_xyz(ra, dec)
    (lx,), (ly,), (lz,) = radec_to_xyz(np.array([ra_l]), np.array([dec_l]))
    c2, s2p, den = shear_oracle.projection(x, y, z, lx, ly, lz)
    phi = reference_angle(ra, dec, ra_l, dec_l)
    bound = rotation_bound(x, y, z, lx, ly, lz)
    assert np.all(den > 0) and bound.max() < 1e-9  # (tighter than the flat 1e-9 this test had, which went down to 0.5 arcmin)
    assert np.all(np.abs(c2 - np.cos(2 * phi)) <= bound)
    assert np.all(np.abs(s2p - np.sin(2 * phi)) <= bound)
    return ra, dec, x, y, z, lx, ly, lz


@pytest.mark.parametrize("dec_l", [0.0, 0.9, -1.4, DEC_EXTREME, -DEC_EXTREME])
def test_projection_matches_the_spherical_position_angle(dec_l):
    rng = np.random.default_rng(11)
    ra_l, amplitude = 2.1, 0.03
    ra, dec, x, y, z, lx, ly, lz = check_projection(rng, ra_l, dec_l, 0.5 * ARCMIN, 30.0 * ARCMIN, False)
    # down to 0.5 arcsec, also just below the wrap of the right ascension and with partners on both sides of it
    for ra_other in (ra_l, 6.2831, RA_WRAP):
        ra_s = check_projection(np.random.default_rng(12), ra_other, dec_l, 0.5 * ARCSEC, 30.0 * ARCSEC, True)[0]
        assert ra_other != RA_WRAP or 1000 < np.count_nonzero(ra_s < np.pi) < 4000
    # a pure tangential pattern comes back as gamma_t = A, gamma_x = 0
    g1, g2 = shear_oracle.tangential_pattern(ra, dec, ra_l, dec_l, amplitude)
    w = rng.uniform(0.5, 2.0, len(ra))
    lens = dict(x=np.array([lx]), y=np.array([ly]), z=np.array([lz]), w=np.array([1.7]), nb=1, off=np.array([0, 1]))
    src = dict(x=x, y=y, z=z, w=w, g1=g1, g2=g2, off=np.array([0, len(x)]))
    t = (2.0 * np.sin(0.5 * np.array([[0.4, 5.0, 31.0]]) * ARCMIN)) ** 2
    T, X, W, A = shear_oracle.shear_jobs(lens, src, [[0, 0]], t)
    assert np.all(W > 0) and W.sum() == pytest.approx(1.7 * w.sum(), rel=1e-12)
    np.testing.assert_allclose(T / W, amplitude, rtol=1e-10)
    assert np.all(np.abs(X / W) <= 1e-10 * amplitude)
    np.testing.assert_allclose(A.sum(), (1.7 * w * (np.abs(g1) + np.abs(g2))).sum(), rtol=1e-12)


# --------------------------------------------------------------------------- 2. catalogue plumbing
def _shear_columns(ra, dec):
    return 0.5 * ra + dec, ra - 2.0 * dec  # functions of the position: alignment is checkable per object


@pytest.mark.parametrize("n", [300, catalog_module.HOST_GROUP_MIN + 1000], ids=["numpy", "group_columns"])
def test_shear_columns_follow_the_objects_through_patch_assignment(n):
    rng = np.random.default_rng(n)
    ra, dec = rng.uniform(0.1, 0.3, n), rng.uniform(-0.1, 0.1, n)
    g1, g2 = _shear_columns(ra, dec)
    cat = yaw.Catalog.from_arrays(ra, dec, g1=g1, g2=g2, weights=rng.uniform(1, 2, n), patch_ids=rng.integers(0, 5, n),
                                  degrees=False)
    assert cat.has_shear
    seen = 0
    for patch in cat.values():
        pra, pdec = patch.coords.ra, patch.coords.dec
        e1, e2 = _shear_columns(pra, pdec)
        assert np.array_equal(patch.g1, e1) and np.array_equal(patch.g2, e2)
        seen += len(patch)
    assert seen == n
    layout = cat.build_trees(None)
    assert np.array_equal(layout.g1, np.concatenate([p.g1 for p in cat.values()]))
    assert np.array_equal(layout.g2, np.concatenate([p.g2 for p in cat.values()]))
    plain = yaw.Catalog.from_arrays(ra, dec, patch_ids=np.zeros(n, dtype=int), degrees=False)
    assert not plain.has_shear and plain[0].g1 is None and plain[0].g2 is None
    assert plain.build_trees(None).g1 is None


def test_flip_g2_negates_g2_only():
    ra, dec = np.linspace(10, 11, 50), np.linspace(-1, 1, 50)
    g1, g2 = np.linspace(-0.1, 0.1, 50), np.linspace(0.2, -0.3, 50)
    kw = dict(patch_ids=np.zeros(50, dtype=int))
    same = yaw.Catalog.from_arrays(ra, dec, g1=g1, g2=g2, **kw)
    flipped = yaw.Catalog.from_arrays(ra, dec, g1=g1, g2=g2, flip_g2=True, **kw)
    assert np.array_equal(same[0].g1, g1) and np.array_equal(same[0].g2, g2)
    assert np.array_equal(flipped[0].g1, g1) and np.array_equal(flipped[0].g2, -g2)
    frame = dict(ra=ra, dec=dec, e1=g1, e2=g2, patch=np.zeros(50, dtype=int))
    framed = yaw.Catalog.from_dataframe(None, frame, ra_name="ra", dec_name="dec", patch_name="patch", g1_name="e1", g2_name="e2")
    assert np.array_equal(framed[0].g1, g1) and np.array_equal(framed[0].g2, g2)


def test_shear_column_errors_and_layouts(tmp_path):
    ra, dec = np.linspace(10, 11, 20), np.linspace(-1, 1, 20)
    g = np.full(20, 0.01)
    kw = dict(patch_ids=np.zeros(20, dtype=int))
    with pytest.raises(ValueError, match="both"):
        yaw.Catalog.from_arrays(ra, dec, g1=g, **kw)
    with pytest.raises(ValueError, match="both"):
        yaw.Catalog.from_arrays(ra, dec, g2=g, **kw)
    bad = g.copy()
    bad[3] = np.nan
    with pytest.raises(ValueError):
        yaw.Catalog.from_arrays(ra, dec, g1=bad, g2=g, **kw)
    bad[3] = np.inf
    with pytest.raises(ValueError):
        yaw.Catalog.from_arrays(ra, dec, g1=g, g2=bad, **kw)
    with pytest.raises(ValueError, match="length"):
        yaw.Catalog.from_arrays(ra, dec, g1=g[:-1], g2=g[:-1], **kw)
    cat = yaw.Catalog.from_arrays(ra, dec, g1=g, g2=g, redshifts=np.linspace(0.2, 0.8, 20), **kw)
    with pytest.raises(ValueError, match="cache"):
        cat.to_cache(tmp_path / "cache")
    assert not (tmp_path / "cache").exists()
    binned = cat.build_trees(np.array([0.1, 0.5, 0.9]))
    assert binned.g1 is None and binned.g2 is None  # a binned layout does not carry the shear
    unbinned = cat.build_trees(None)
    assert np.array_equal(unbinned.g1, g) and np.array_equal(unbinned.g2, g)


# --------------------------------------------------------------------------- 3. the driver on the oracle stand-in
AMPLITUDES = (0.02, 0.05)
LENSES = ((0.30, 0.10), (0.30 + np.deg2rad(10.0), 0.12))  # (ra, dec) radian, two patches 10 degrees apart
ZEDGES = np.array([0.1, 0.5, 0.9])


def shear_scenario(with_randoms=False, shear=True):
    """One lens per patch, in different redshift bins; 500 sources in a 1'-8' annulus around each, carrying the tangential
    pattern of their lens with its own amplitude. Returns ``(config, reference, sources, ref_rand | None)``."""
    rng = np.random.default_rng(5)
    centers = yaw.AngularCoordinates(np.array(LENSES))
    ra, dec, g1, g2 = [], [], [], []
    for (ra_l, dec_l), amplitude in zip(LENSES, AMPLITUDES):
        r, d = ring_around(rng, ra_l, dec_l, 500, 1.0 * ARCMIN, 8.0 * ARCMIN)
        a, b = shear_oracle.tangential_pattern(r, d, ra_l, dec_l, amplitude)
        ra.append(r), dec.append(d), g1.append(a), g2.append(b)
    ra, dec, g1, g2 = (np.concatenate(c) for c in (ra, dec, g1, g2))
    kw = dict(patch_centers=centers, degrees=False)
    shear_kw = dict(g1=g1, g2=g2) if shear else {}
    sources = yaw.Catalog.from_arrays(ra, dec, weights=rng.uniform(0.5, 1.5, len(ra)), **shear_kw, **kw)
    lens_ra, lens_dec = np.array([l[0] for l in LENSES]), np.array([l[1] for l in LENSES])
    reference = yaw.Catalog.from_arrays(lens_ra, lens_dec, redshifts=np.array([0.3, 0.7]), weights=np.array([1.3, 0.8]), **kw)
    ref_rand = None
    if with_randoms:  # three random lenses per patch and bin, a few arcmin off the real ones
        rr = np.concatenate([ring_around(rng, ra_l, dec_l, 6, 2.0 * ARCMIN, 4.0 * ARCMIN) for ra_l, dec_l in LENSES], axis=1)
        ref_rand = yaw.Catalog.from_arrays(rr[0], rr[1], redshifts=np.tile([0.3, 0.7], 6), **kw)
    config = yaw.Configuration.create(rmin=[0.9, 2.0], rmax=[8.1, 6.0], unit="arcmin", rweight=-0.8, resolution=12, edges=ZEDGES)
    return config, reference, sources, ref_rand


def check_shear_scenario(with_randoms):
    """The assertions of the scenario; ``engine.count_shear_fine`` is whatever the caller left in place."""
    config, reference, sources, ref_rand = shear_scenario(with_randoms)
    dd_only = yaw.crosscorrelate_shear(config, reference, sources)
    assert len(dd_only) == 2
    for cf_t, cf_x in dd_only:
        assert type(cf_t) is yaw.ScalarCorrFunc and type(cf_x) is yaw.ScalarCorrFunc
        assert cf_t.dr is None and cf_x.dr is None
        sampled_t, sampled_x = cf_t.sample(), cf_x.sample()
        for k, amplitude in enumerate(AMPLITUDES):  # lens k sits in patch k and redshift bin k
            assert sampled_t.data[k] == pytest.approx(amplitude, rel=1e-10)
            assert abs(sampled_x.data[k]) <= 1e-10 * amplitude
        assert sampled_t.samples.shape == (2, 2) and sampled_x.samples.shape == (2, 2)  # [P, B]
        assert np.array_equal(cf_t.dd.number_counts.counts, cf_x.dd.number_counts.counts)
        assert np.count_nonzero(cf_t.dd.number_counts.counts) == 2  # slots [0, 0, 0] and [1, 1, 1] only
    if not with_randoms:
        return
    with_dr = yaw.crosscorrelate_shear(config, reference, sources, ref_rand=ref_rand)
    links = yaw.PatchLinkage.from_catalogs(config, reference, sources, ref_rand)
    dr_alone = links.count_shear_pairs(ref_rand, sources)
    for (cf_t, cf_x), (dd_t, dd_x), (dr_t, dr_x) in zip(with_dr, dd_only, dr_alone):
        assert cf_t.dd == dd_t.dd and cf_x.dd == dd_x.dd
        assert cf_t.dr == dr_t and cf_x.dr == dr_x
        assert np.any(dr_t.kappa_counts.counts != 0) and np.all(dr_t.number_counts.counts[[0, 1], [0, 1], [0, 1]] > 0)
        for cf, dd, dr in ((cf_t, dd_t, dr_t), (cf_x, dd_x, dr_x)):
            assert np.array_equal(cf.sample().data, dd.sample().data - dr.sample_patch_sum().data)


@pytest.mark.parametrize("with_randoms", [False, True], ids=["dd", "dd-dr"])
def test_driver_on_the_oracle_stand_in(monkeypatch, with_randoms):
    monkeypatch.setattr(engine, "count_shear_fine", shear_oracle.count_shear_fine)
    check_shear_scenario(with_randoms)


def test_driver_rejects_sources_without_shear_and_shared_catalogues(monkeypatch):
    monkeypatch.setattr(engine, "count_shear_fine", shear_oracle.count_shear_fine)
    config, reference, sources, _ = shear_scenario(shear=False)
    with pytest.raises(ValueError, match="catalog has no 'g1'/'g2' attached"):
        yaw.crosscorrelate_shear(config, reference, sources)
    config, reference, sources, _ = shear_scenario()
    with pytest.raises(ValueError, match="separate Catalog instance"):
        yaw.crosscorrelate_shear(config, reference, reference)
    with pytest.raises(ValueError, match="separate Catalog instance"):
        yaw.crosscorrelate_shear(config, reference, sources, ref_rand=reference)


def test_several_ranks_are_refused(monkeypatch):
    from yet_another_wizz_amd import parallel

    monkeypatch.setattr(engine, "count_shear_fine", shear_oracle.count_shear_fine)
    monkeypatch.setattr(parallel, "world", lambda: (0, 2))
    config, reference, sources, _ = shear_scenario()
    with pytest.raises(NotImplementedError):
        yaw.crosscorrelate_shear(config, reference, sources)
