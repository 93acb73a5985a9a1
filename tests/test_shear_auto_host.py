"""CPU: shear-shear correlations in redshift bins (``autocorrelate_shear``) above the device seam -- known answers of the
contract, the oracle's rotations against spherical trigonometry, the binned layout with shear columns, and the driver with
``engine.count_shear_auto_fine`` replaced by the numpy brute force of tests/shear_auto_oracle.py."""
import os
import re

import numpy as np
import pytest

import shear_auto_oracle
import shear_oracle
import yet_another_wizz_amd as yaw
from conftest import ARCMIN, ROOT
from test_shear_host import ARCSEC, reference_angle, ring_around, rotation_bound
from yet_another_wizz_amd import catalog as catalog_module
from yet_another_wizz_amd import engine, measurements
from yet_another_wizz_amd.catalog import radec_to_xyz

G = 0.03
DEG = np.pi / 180.0


def two_objects(ra, dec, shears):
    """One patch, one bin, two objects with unit weights -> the oracle's (P, M, C, W) of the one pair, 3 arcmin apart."""
    x, y, z = radec_to_xyz(np.asarray(ra, dtype=float), np.asarray(dec, dtype=float))
    cat = dict(x=x, y=y, z=z, w=None, g1=np.array([s[0] for s in shears], dtype=float), g2=np.array([s[1] for s in shears], dtype=float),
               nb=1, off=np.array([0, 2], dtype=np.int64))
    t = (2.0 * np.sin(0.5 * np.array([[1.0, 5.0]]) * ARCMIN)) ** 2
    P, M, C, W, _ = shear_auto_oracle.shear_auto_jobs(cat, [[0, 0]], t)
    assert W[0, 0, 0] == 1.0
    return P[0, 0, 0], M[0, 0, 0], C[0, 0, 0]


# --------------------------------------------------------------------------- 1. known answers
@pytest.mark.parametrize("where", ["equator", "meridian"])
def test_known_answers_from_two_objects(where):
    """The signs of the contract, independent of any kernel: a pair along RA on the equator (position angles 0 and pi) and a
    pair on one meridian (position angles +-pi/2)."""
    ra, dec = ([0.7, 0.7 + 3.0 * ARCMIN], [0.0, 0.0]) if where == "equator" else ([0.0, 0.0], [0.0, 3.0 * ARCMIN])
    g2 = G * G
    expected = [(((G, 0.0), (G, 0.0)), (g2, g2, 0.0)), (((0.0, G), (0.0, G)), (g2, -g2, 0.0))]
    if where == "equator":
        expected.append((((G, 0.0), (0.0, G)), (0.0, 0.0, g2)))
    for shears, want in expected:
        got = two_objects(ra, dec, shears)
        for value, ref in zip(got, want):
            assert abs(value - ref) <= 1e-14 * g2, (where, shears, got)


# --------------------------------------------------------------------------- 2. the rotations
@pytest.mark.parametrize("dec_deg", [0.0, 40.0, 80.0, 89.99, -89.99])
def test_rotations_match_the_spherical_position_angles(dec_deg):
    """cos / sin of twice the position angle at EACH end, from tests/shear_oracle.position_angle taken from that end, pair by
    pair within ``K eps / theta`` (test_shear_host.rotation_bound): partners 0.5' .. 30' away, then 0.5" .. 30" (uniform in the
    logarithm), the last 20 objects within 2" of the wrap of the right ascension."""
    rng = np.random.default_rng(int(abs(dec_deg)) + 3)
    ra_a = rng.uniform(0.0, 2.0 * np.pi, 200)
    dec_a = np.full(200, dec_deg * DEG)
    for rmin, rmax, log_uniform in ((0.5 * ARCMIN, 30.0 * ARCMIN, False), (0.5 * ARCSEC, 30.0 * ARCSEC, True)):
        if log_uniform:
            ra_a[-20:] = rng.uniform(-2.0, 2.0, 20) * ARCSEC % (2.0 * np.pi)
        ra_b, dec_b = np.empty(200), np.empty(200)
        for i in range(200):  # one partner in any direction
            (ra_b[i],), (dec_b[i],) = ring_around(rng, ra_a[i], dec_a[i], 1, rmin, rmax, log_uniform=log_uniform)
        assert not log_uniform or np.count_nonzero(np.abs(ra_a - ra_b) > 6.0) >= 3  # pairs across the wrap
        xyz_a, xyz_b = radec_to_xyz(ra_a, dec_a), radec_to_xyz(ra_b, dec_b)
        c_a, s_a, c_b, s_b, den_a, den_b = shear_auto_oracle.rotations(*xyz_a, *xyz_b)
        assert np.all(den_a > 0) and np.all(den_b > 0)
        phi_a = reference_angle(ra_a, dec_a, ra_b, dec_b)  # b seen from a
        phi_b = reference_angle(ra_b, dec_b, ra_a, dec_a)  # a seen from b
        bound = rotation_bound(*xyz_a, *xyz_b)
        assert bound.max() < 1e-9  # (tighter than the flat 1e-9 this test had, which went down to 0.5 arcmin)
        for ours, ref in ((c_a, np.cos(2 * phi_a)), (s_a, np.sin(2 * phi_a)), (c_b, np.cos(2 * phi_b)), (s_b, np.sin(2 * phi_b))):
            assert np.all(np.abs(ours - ref) <= bound)


# --------------------------------------------------------------------------- 3. the binned layout with shear
def _shear_columns(ra, dec):
    return 0.5 * ra + dec, ra - 2.0 * dec  # functions of the position: alignment is checkable per object


@pytest.mark.parametrize("n", [300, catalog_module.HOST_GROUP_MIN + 1000], ids=["numpy", "group_columns"])
def test_build_trees_with_shear_groups_the_columns(n):
    rng = np.random.default_rng(n)
    ra, dec = rng.uniform(0.1, 0.3, n), rng.uniform(-0.1, 0.1, n)
    g1, g2 = _shear_columns(ra, dec)
    redshifts = rng.uniform(0.0, 1.0, n)  # about 20 % fall outside the binning
    patch_ids = rng.integers(0, 3, n)
    weights = rng.uniform(1.0, 2.0, n)
    cat = yaw.Catalog.from_arrays(ra, dec, g1=g1, g2=g2, redshifts=redshifts, weights=weights, patch_ids=patch_ids, degrees=False)
    edges = np.array([0.1, 0.4, 0.9])
    layout = cat.build_trees(edges, with_shear=True)
    # a plain numpy regrouping: stable by (patch, bin), objects outside the binning dropped
    bin_idx = np.searchsorted(edges, redshifts, side="left") - 1  # closed="right": edges[k] < z <= edges[k+1]
    keep = np.flatnonzero((redshifts > edges[0]) & (redshifts <= edges[-1]))
    order = keep[np.argsort(patch_ids[keep] * 2 + bin_idx[keep], kind="stable")]
    assert len(order) < n and layout.num_records == len(order) and layout.num_bins == 2
    x, y, z = radec_to_xyz(ra, dec)
    for ours, ref in ((layout.x, x), (layout.y, y), (layout.z, z), (layout.w, weights), (layout.g1, g1), (layout.g2, g2)):
        assert np.array_equal(ours, ref[order])
    assert np.array_equal(np.diff(layout.offsets), np.bincount(patch_ids[keep] * 2 + bin_idx[keep], minlength=6))
    plain = cat.build_trees(edges)
    assert plain.g1 is None and plain.g2 is None and plain is not layout  # the default call: its own cache entry
    assert cat.build_trees(edges, with_shear=True) is layout and cat.build_trees(edges) is plain
    assert cat._active_layout is plain
    cat.drop_layouts()
    assert cat._active_layout is None and cat.build_trees(edges, with_shear=True) is not layout


def test_build_trees_with_shear_needs_shear_and_redshifts():
    ra, dec = np.linspace(10, 11, 20), np.linspace(-1, 1, 20)
    g = np.full(20, 0.01)
    kw = dict(patch_ids=np.zeros(20, dtype=int))
    edges = np.array([0.1, 0.5, 0.9])
    with pytest.raises(ValueError, match="g1"):
        yaw.Catalog.from_arrays(ra, dec, redshifts=np.linspace(0.2, 0.8, 20), **kw).build_trees(edges, with_shear=True)
    with pytest.raises(ValueError, match="redshifts"):
        yaw.Catalog.from_arrays(ra, dec, g1=g, g2=g, **kw).build_trees(edges, with_shear=True)


# --------------------------------------------------------------------------- 4. the driver on the oracle stand-in
def test_constant_field_gives_xi_plus_g_squared(monkeypatch):
    """g1 = g, g2 = 0 everywhere near the equator: xi_plus = g^2 (the frames at the two ends of a pair differ by at most
    theta tan(dec) ~ 1e-5 rad, an effect of 2e-10); xi_minus and xi_cross carry cos / sin of FOUR times the direction of the
    pair, which only averages out."""
    monkeypatch.setattr(engine, "count_shear_auto_fine", shear_auto_oracle.count_shear_auto_fine)
    rng = np.random.default_rng(17)
    n = 400
    ra, dec = rng.uniform(20.0, 20.4, n), rng.uniform(-0.2, 0.2, n)
    centers = yaw.AngularCoordinates(np.deg2rad([[20.1, 0.0], [20.3, 0.0]]))
    cat = yaw.Catalog.from_arrays(ra, dec, g1=np.full(n, G), g2=np.zeros(n), redshifts=rng.uniform(0.2, 0.8, n), patch_centers=centers)
    config = yaw.Configuration.create(rmin=1.0, rmax=10.0, unit="arcmin", zmin=0.1, zmax=0.9, num_bins=1)
    ((cf_plus, cf_minus, cf_cross),) = yaw.autocorrelate_shear(config, cat)
    assert cf_plus.dd.number_counts.counts.sum() > 1000
    assert abs(cf_plus.sample().data[0] - G * G) <= 1e-8 * G * G
    assert abs(cf_minus.sample().data[0]) < 0.2 * G * G and abs(cf_cross.sample().data[0]) < 0.2 * G * G


ZEDGES = np.array([0.1, 0.5, 0.9])


def auto_scenario(shear=True, redshifts=True):
    """1200 weighted sources in two patches 12 arcmin apart and two redshift bins, a coherent shear plus noise."""
    rng = np.random.default_rng(23)
    n = 1200
    centre_ra = np.array([0.30, 0.30 + 12.0 * ARCMIN])
    centers = yaw.AngularCoordinates(np.stack([centre_ra, [0.10, 0.10]], axis=1))
    which = rng.integers(0, 2, n)
    ra = centre_ra[which] + rng.uniform(-6.0, 6.0, n) * ARCMIN
    dec = 0.10 + rng.uniform(-6.0, 6.0, n) * ARCMIN
    columns = dict(weights=rng.uniform(0.5, 1.5, n))
    if shear:
        columns.update(g1=0.05 + rng.normal(0, 0.02, n), g2=-0.02 + rng.normal(0, 0.02, n))
    if redshifts:
        columns.update(redshifts=rng.uniform(0.1, 0.9, n))
    sources = yaw.Catalog.from_arrays(ra, dec, patch_centers=centers, degrees=False, **columns)
    config = yaw.Configuration.create(rmin=[0.9, 2.0], rmax=[8.1, 6.0], unit="arcmin", rweight=-0.8, resolution=12, edges=ZEDGES)
    return config, sources


def check_auto_scenario():
    """The assertions of the scenario; ``engine.count_shear_auto_fine`` is whatever the caller left in place."""
    config, sources = auto_scenario()
    result = yaw.autocorrelate_shear(config, sources)
    assert isinstance(result, list) and len(result) == 2
    # the same numbers from the oracle's fine bins, combined with the same plan
    layout = sources.build_trees(ZEDGES, with_shear=True)
    links = yaw.PatchLinkage.from_catalogs(config, sources)
    jobs = links.get_patch_pairs(sources)
    assert [tuple(j) for j in jobs] == [(0, 0), (1, 1), (0, 1)]
    plans, thresholds = links._angular_setup()
    fine = shear_auto_oracle.shear_auto_jobs(shear_auto_oracle.as_catalogue(layout), jobs, thresholds)
    combine = measurements.CombinePlan(plans)
    P, M, C, W = (combine(np.moveaxis(f, 0, -1)).sum(axis=2) for f in fine[:4])  # [S, B]
    for s, triple in enumerate(result):
        assert len(triple) == 3
        for cf in triple:
            assert type(cf) is yaw.ScalarCorrFunc and cf.dr is None
            assert cf.dd.kappa_counts.auto and cf.dd.number_counts.auto
            assert cf.sample().samples.shape == (2, 2)  # [P, B]
        cf_plus, cf_minus, cf_cross = triple
        assert np.array_equal(cf_plus.dd.number_counts.counts, cf_minus.dd.number_counts.counts)
        assert np.array_equal(cf_plus.dd.number_counts.counts, cf_cross.dd.number_counts.counts)
        assert np.all(cf_plus.dd.number_counts.counts[:, [0, 0, 1], [0, 1, 1]] > 0)  # the upper triangle is filled ...
        assert np.all(cf_plus.dd.number_counts.counts[:, 1, 0] == 0)                 # ... and only it
        np.testing.assert_allclose(cf_plus.sample().data, P[s] / W[s], rtol=1e-10)
        np.testing.assert_allclose(cf_minus.sample().data, M[s] / W[s], rtol=1e-8, atol=1e-12)
        np.testing.assert_allclose(cf_cross.sample().data, C[s] / W[s], rtol=1e-8, atol=1e-12)
        assert np.all(cf_plus.sample().data > 0.05 ** 2)  # the coherent part: (0.05^2 + 0.02^2) and the noise on top


def test_driver_on_the_oracle_stand_in(monkeypatch):
    monkeypatch.setattr(engine, "count_shear_auto_fine", shear_auto_oracle.count_shear_auto_fine)
    check_auto_scenario()


def test_driver_rejects_catalogues_without_shear_or_redshifts(monkeypatch):
    monkeypatch.setattr(engine, "count_shear_auto_fine", shear_auto_oracle.count_shear_auto_fine)
    config, sources = auto_scenario(shear=False)
    with pytest.raises(ValueError, match="catalog has no 'g1'/'g2' attached"):
        yaw.autocorrelate_shear(config, sources)
    config, sources = auto_scenario(redshifts=False)
    with pytest.raises(ValueError, match="redshifts"):
        yaw.autocorrelate_shear(config, sources)


def test_several_ranks_are_refused(monkeypatch):
    from yet_another_wizz_amd import parallel

    monkeypatch.setattr(engine, "count_shear_auto_fine", shear_auto_oracle.count_shear_auto_fine)
    monkeypatch.setattr(parallel, "world", lambda: (0, 2))
    config, sources = auto_scenario()
    with pytest.raises(NotImplementedError):
        yaw.autocorrelate_shear(config, sources)


# --------------------------------------------------------------------------- 5. ABI
def test_new_symbols_are_declared_and_bound_at_abi_6():
    from yet_another_wizz_amd import _lib

    text = open(os.path.join(ROOT, "include", "yawhip.h")).read()
    code = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    for name in ("yawhip_shear_upload_binned", "yawhip_shear_auto_count"):
        assert name in _lib.ABI_SYMBOLS
        assert re.search(rf"\bint {name}\s*\(", code)
    assert re.search(r"#define YAWHIP_ABI_VERSION 6\b", text)
    assert "autocorrelate_shear" in yaw.__all__
