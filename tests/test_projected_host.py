"""CPU: projected clustering in each pair's own radius (``autocorrelate_projected``) above the device seam -- the C ABI's new
names, the columns, what the feature is for, the driver with ``engine.count_projected_fine`` replaced by the numpy brute force
of tests/proj_oracle.py, the oracle's symmetry, the error cases, and the oracle's membership against mpmath on the scene that
the device tests use (tests/proj_scenes.py)."""
import ctypes
import os
import re

import numpy as np
import pytest

import proj_oracle
import proj_scenes
import yet_another_wizz_amd as yaw
from conftest import ROOT
from helpers import use_oracle_engine
from test_dsigma_host import CENTERS, jackknife
from test_shear_host import ring_around
from yet_another_wizz_amd import _lib, cosmology, engine, measurements

COSMO = cosmology.Planck15
SYMBOLS = ("yawhip_proj_upload", "yawhip_proj_count")
EPS = 2.0**-53


@pytest.fixture
def stand_in(monkeypatch):
    monkeypatch.setattr(engine, "count_projected_fine", proj_oracle.count_projected_fine)
    use_oracle_engine(monkeypatch)  # count_pairs, for the comparison with the angular count


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
    assert "autocorrelate_projected" in yaw.__all__ and "autocorrelate_projected" in measurements.__all__
    assert callable(_lib.proj_count) and issubclass(_lib.ProjHandle, _lib.ShearSources)
    _lib.load_library()
    assert _lib.load_library().yawhip_proj_count.argtypes[8] is ctypes.c_double  # pmax


# --------------------------------------------------------------------------- 2. the columns
@pytest.mark.parametrize("unit", ["kpc", "Mpc", "kpc/h", "Mpc/h"])
def test_the_columns_are_the_cosmologys_distances(unit):
    z = np.array([0.05, 0.2, 0.7, 1.4])
    layout = type("L", (), dict(redshifts=z))()
    d, c = engine.proj_columns(layout, COSMO, unit)
    d_a = cosmology.distance_column(COSMO, z, kind="angular")
    chi = cosmology.distance_column(COSMO, z, kind="comoving")
    assert np.array_equal(c, chi)
    if unit in ("kpc", "Mpc"):
        assert np.array_equal(d, d_a)
    else:
        assert np.array_equal(d, d_a * (1.0 + z))
        np.testing.assert_allclose(d, chi, rtol=1e-14)  # a flat cosmology: D_A (1 + z) is the comoving distance
    # the radii of the plan are in the same Mpc: a scale of 500 kpc (or kpc/h) at z = 0.7 is the angle Scales gives it
    config = yaw.Configuration.create(rmin=100.0 if "kpc" in unit else 0.1, rmax=500.0 if "kpc" in unit else 0.5, unit=unit, edges=np.array([0.1, 1.0]))
    theta = config.scales.scales.get_angle_radian(0.7, cosmology=COSMO)[1][0]
    radius = np.sqrt(measurements.threshold_table(measurements.radial_plans(config))[0, -1])
    assert radius / d[2] == pytest.approx(theta, rel=1e-13)


# --------------------------------------------------------------------------- 3. what the feature is for
def redshift_at(chi):
    """The redshift at the comoving distance ``chi`` (Mpc), by bisection on the cosmology."""
    lo, hi = 0.0, 3.0
    for _ in range(200):
        mid = 0.5 * (lo + hi)
        lo, hi = (mid, hi) if float(COSMO.comoving_distance(mid)) < chi else (lo, mid)
    return 0.5 * (lo + hi)


GROUP_SIZE = 12  # quadruples per group


def two_groups():
    """Two compact groups in ONE slice 0.1 < z < 1.0, one at z = 0.15 and one at z = 0.9, in patches of their own 10 degrees
    apart. A group is 12 quadruples 0.3 degrees apart; a quadruple is two sky positions an angle ``theta`` apart (320 kpc at
    the group's redshift) with two objects each: A (first position, chi0), B (second, chi0 + 0.5 Mpc), C (first, chi0 + 80 Mpc)
    and D (second, chi0 + 80.5 Mpc). Every object has ONE partner at ``theta`` with |delta chi| = 0.5 Mpc (A-B, C-D) and ONE
    at the same angle with |delta chi| = 79.5 or 80.5 Mpc (A-D, B-C); the other two pairs (A-C, B-D) are at angle 0."""
    ra, dec, z = [], [], []
    for (ra_c, dec_c), z0 in zip(CENTERS[:2], (0.15, 0.9)):
        theta = 0.320 / float(COSMO.angular_diameter_distance(z0))
        chi0 = float(COSMO.comoving_distance(z0))
        zs = [z0] + [redshift_at(chi0 + more) for more in (0.5, 80.0, 80.5)]
        for n in range(GROUP_SIZE):
            base = ra_c + np.deg2rad(0.3) * (n - 0.5 * GROUP_SIZE)
            ra += [base, base + theta / np.cos(dec_c), base, base + theta / np.cos(dec_c)]
            dec += [dec_c] * 4
            z += zs
    config = yaw.Configuration.create(rmin=[100.0, 300.0, 600.0], rmax=[300.0, 600.0, 1500.0], unit="kpc", edges=np.array([0.1, 1.0]))
    catalog = yaw.Catalog.from_arrays(np.array(ra), np.array(dec), redshifts=np.array(z), patch_centers=yaw.AngularCoordinates(np.array(CENTERS[:2])), degrees=False)
    return config, catalog


def test_both_groups_pairs_land_in_the_bin_that_names_their_radius(stand_in):
    """The feature: the partners 320 kpc apart are all in the scale 300 - 600 kpc, whichever end of the slice their group sits
    at, and the line-of-sight cut keeps those 0.5 Mpc apart and drops those 80 Mpc apart. ``count_pairs`` on the same
    catalogue bins by the angle at the slice's middle (z = 0.55) and knows no line of sight: it puts the near group's pairs
    at 790 kpc and the far group's at 264 kpc -- in two other scales, none in the one that names the radius, and the far
    partners with the close ones."""
    config, catalog = two_groups()
    layout = catalog.build_trees(config.binning.edges, closed=config.binning.closed, with_redshifts=True)
    chi = cosmology.distance_column(COSMO, layout.redshifts, kind="comoving")
    for p in range(2):  # the scene is what the docstring says
        seg = chi[layout.offsets[p]:layout.offsets[p + 1]]
        steps = np.sort(seg) - seg.min()
        assert np.all(np.abs(steps.reshape(4, GROUP_SIZE).mean(axis=1) - [0.0, 0.5, 80.0, 80.5]) < 1e-6)
    links = yaw.PatchLinkage.from_catalogs(config, catalog, max_angle=measurements.radial_max_angle(config, layout))
    pairs = lambda result: [nc.counts.counts[0].tolist() for nc in result]  # [S][P][P]
    near_cut = links.count_projected_pairs(catalog, pi_max=40.0)
    assert pairs(near_cut) == [[[0, 0], [0, 0]], [[2.0 * GROUP_SIZE, 0], [0, 2.0 * GROUP_SIZE]], [[0, 0], [0, 0]]]
    far_cut = links.count_projected_pairs(catalog, pi_max=200.0)
    assert pairs(far_cut) == [[[0, 0], [0, 0]], [[4.0 * GROUP_SIZE, 0], [0, 4.0 * GROUP_SIZE]], [[0, 0], [0, 0]]]
    assert all(type(nc) is yaw.NormalisedCounts and nc.auto for nc in near_cut)
    catalog.build_trees(config.binning.edges, closed=config.binning.closed)
    angular = yaw.PatchLinkage.from_catalogs(config, catalog).count_pairs(catalog)
    assert pairs(angular) == [[[0, 0], [0, 4.0 * GROUP_SIZE]], [[0, 0], [0, 0]], [[4.0 * GROUP_SIZE, 0], [0, 0]]]


# --------------------------------------------------------------------------- 4. the driver on the oracle stand-in
ZEDGES = np.array([0.2, 0.4, 0.6])
NEIGHBOURS = ((0.30, 0.10), (0.3025, 0.10), (0.3050, 0.1005))  # three patches side by side: pairs across their borders


def driver_scenario():
    """Three patches 8.6 arcmin apart, two redshift bins: 90 weighted data objects and 150 randoms around every centre, within
    6 arcmin of it (an object belongs to the nearest centre), redshifts 0.22 .. 0.58."""
    rng = np.random.default_rng(23)
    kw = dict(patch_centers=yaw.AngularCoordinates(np.array(NEIGHBOURS)), degrees=False)
    cats = []
    for n, weighted in ((90, True), (150, False)):
        ra, dec = (np.concatenate(c) for c in zip(*(ring_around(rng, ra_c, dec_c, n, 1e-5, 1.8e-3) for ra_c, dec_c in NEIGHBOURS)))
        cats.append(yaw.Catalog.from_arrays(ra, dec, redshifts=rng.uniform(0.22, 0.58, len(ra)),
                                            weights=rng.uniform(0.5, 1.5, len(ra)) if weighted else None, **kw))
    return cats


def driver_config(unit):
    if unit == "kpc":
        return yaw.Configuration.create(rmin=[100.0, 300.0], rmax=[2000.0, 1000.0], unit="kpc", rweight=-0.8, resolution=12, edges=ZEDGES)
    return yaw.Configuration.create(rmin=[0.15, 0.4], rmax=[2.8, 1.5], unit="Mpc/h", rweight=-0.8, resolution=12, edges=ZEDGES)


def by_hand(config, cat1, cat2, pi_max):
    """The count [S, B, P, P] from the oracle's fine sums and the radial plan over all nine patch pairs (the upper triangle of
    an auto count), and its normalisation [B, P, P]."""
    auto = cat2 is None
    plans = measurements.radial_plans(config)
    r2 = measurements.threshold_table(plans)
    unit = config.scales.scales.unit
    layouts = [cat.build_trees(config.binning.edges, closed=config.binning.closed, with_redshifts=True) for cat in ((cat1,) if auto else (cat1, cat2))]
    handles = [proj_oracle.as_handle(layout, *engine.proj_columns(layout, config.cosmology, unit)) for layout in layouts]
    jobs = [(p, q) for p in range(3) for q in range(p if auto else 0, 3)]
    cells = np.array([(p * 2 + k, q * 2 + k, k, auto and p == q) for p, q in jobs for k in range(2)])
    W, _, _ = proj_oracle.proj_cells(handles[0], handles[-1], cells, r2, pi_max)
    per_scale = measurements.CombinePlan(plans)(np.moveaxis(W.reshape(len(jobs), 2, -1), 0, -1))  # [S, B, J]
    counts = np.zeros((per_scale.shape[0], 2, 3, 3))
    for n, (p, q) in enumerate(jobs):
        counts[:, :, p, q] = per_scale[:, :, n]
    sums = [np.array([[(layout.w[lo:hi].sum() if layout.w is not None else float(hi - lo))
                       for lo, hi in zip(layout.offsets[p * 2:p * 2 + 2], layout.offsets[p * 2 + 1:p * 2 + 3])] for p in range(3)]).T
            for layout in layouts]  # [B, P]
    norm = sums[0][:, :, None] * sums[-1][:, None, :]
    if auto:
        norm = np.triu(norm)
        norm[:, np.arange(3), np.arange(3)] *= 0.5
    return counts, norm


def check_driver(unit, count_rr, rtol=1e-12):
    """``autocorrelate_projected`` against Landy-Szalay (Davis-Peebles without RR) recombined by hand from the oracle's fine
    sums; ``engine.count_projected_fine`` is whatever the caller left in place."""
    data, random = driver_scenario()
    config = driver_config(unit)
    pi_max = 60.0
    result = yaw.autocorrelate_projected(config, data, random, pi_max=pi_max, count_rr=count_rr)
    assert len(result) == 2
    hand = dict(dd=by_hand(config, data, None, pi_max), dr=by_hand(config, data, random, pi_max))
    if count_rr:
        hand["rr"] = by_hand(config, random, None, pi_max)
    for s, cf in enumerate(result):
        assert type(cf) is yaw.CorrFunc and cf.rd is None and (cf.rr is not None) == count_rr
        assert cf.dd.auto and not cf.dr.auto
        ratio = {}
        for kind, (counts, norm) in hand.items():
            got = getattr(cf, kind)
            assert np.count_nonzero(counts[s]) >= (2 * 5 if got.auto else 2 * 7)  # pairs across the patch borders too
            np.testing.assert_allclose(got.counts.counts, counts[s], rtol=rtol, atol=0, err_msg=kind)
            (c_tot, c_jk), (n_tot, n_jk) = jackknife(counts[s]), jackknife(norm)  # (of an auto count: its upper triangle)
            ratio[kind] = (c_tot / n_tot, c_jk / n_jk)
            sampled = got.sample_patch_sum()
            np.testing.assert_allclose(sampled.data, ratio[kind][0], rtol=rtol, atol=0)
            np.testing.assert_allclose(sampled.samples, ratio[kind][1], rtol=rtol, atol=0)
        sample = cf.sample()
        for got, part in ((sample.data, 0), (sample.samples, 1)):
            dd, dr = ratio["dd"][part], ratio["dr"][part]
            if count_rr:  # the three ratios are held to rtol each: the estimator moves by that of their magnitudes over RR
                rr = ratio["rr"][part]
                expected, bound = ((dd - dr) + (rr - dr)) / rr, 4.0 * rtol * (np.abs(dd) + 2.0 * np.abs(dr) + np.abs(rr)) / np.abs(rr)
            else:
                expected, bound = (dd - dr) / dr, 4.0 * rtol * np.abs(dd / dr)
            assert np.all(np.abs(got - expected) <= bound)
        assert sample.samples.shape == (3, 2) and np.all(np.isfinite(sample.data))
    return result


@pytest.mark.parametrize("count_rr", [True, False], ids=["LS", "DP"])
@pytest.mark.parametrize("unit", ["kpc", "Mpc/h"])
def test_the_driver_on_the_oracle_stand_in(stand_in, unit, count_rr):
    check_driver(unit, count_rr)


# --------------------------------------------------------------------------- 4b. the linkage at wide angles
WIDE_GRID, WIDE_STEP = 5, np.deg2rad(3.0)  # 25 patches of 3 x 3 degrees over a field of 15 degrees


def wide_scenario():
    """A nearby sample in ONE redshift bin: 300 objects and 400 randoms of unit weight over a field of 15 x 15 degrees around
    dec 8 degrees, in 25 patches, at 0.0055 <= z < 0.02 with the nearest at z = 0.0055 (24 Mpc: the largest radius of 2 Mpc
    spans 4.7 degrees there, a patch and a half, and 1.3 degrees at the far end)."""
    rng = np.random.default_rng(31)
    grid = (np.arange(WIDE_GRID) + 0.5) * WIDE_STEP
    centers = np.array([(0.5 + x, np.deg2rad(0.5) + y) for y in grid for x in grid])
    cats = []
    for n in (300, 400):
        ra = 0.5 + rng.uniform(0.0, WIDE_GRID * WIDE_STEP, n)
        dec = np.deg2rad(0.5) + rng.uniform(0.0, WIDE_GRID * WIDE_STEP, n)
        z = np.concatenate([[0.0055], rng.uniform(0.0055, 0.02, n - 1)])
        cats.append(yaw.Catalog.from_arrays(ra, dec, redshifts=z, patch_centers=yaw.AngularCoordinates(centers), degrees=False))
    config = yaw.Configuration.create(rmin=0.1, rmax=2.0, unit="Mpc", edges=np.array([0.004, 0.03]))
    return config, cats[0], cats[1]


def check_wide_linkage(pi_max=19.0):
    """``autocorrelate_projected`` on the nearby sample, whose linkage must reach past neighbouring patches
    (``radial_max_angle`` between 4 and 5.7 degrees): DD, DR and RR summed over all patch pairs, the diagonal as the driver
    stores it, are the patch-free brute force of tests/proj_oracle.py over the whole catalogues as integers -- a linkage too
    short would lose pairs without a word. Then with four pi bins: the planes sum to the same totals.
    ``engine.count_projected_fine`` and ``engine.count_projected_pi_fine`` are whatever the caller left in place."""
    config, data, random = wide_scenario()
    edges, closed = config.binning.edges, config.binning.closed
    layouts = [cat.build_trees(edges, closed=closed, with_redshifts=True) for cat in (data, random)]
    reach = measurements.radial_max_angle(config, *layouts)
    assert np.deg2rad(4.0) < reach < np.deg2rad(5.7) and WIDE_GRID * WIDE_STEP >= 3.0 * reach and len(data) == WIDE_GRID**2 >= 12
    r2 = measurements.threshold_table(measurements.radial_plans(config))
    assert r2.shape == (1, 2)
    whole = []
    for layout in layouts:  # the whole catalogue as one segment: no patches
        assert layout.w is None and 200 < len(layout.x) < 500
        h = proj_oracle.as_handle(layout, *engine.proj_columns(layout, config.cosmology, "Mpc"))
        whole.append(dict(h, nb=1, off=np.array([0, len(layout.x)], dtype=np.int64)))
    diagonal, across = np.array([[0, 0, 0, 1]]), np.array([[0, 0, 0, 0]])
    expected, uncut = {}, {}
    for kind, (a, b, cell) in dict(dd=(whole[0], whole[0], diagonal), dr=(whole[0], whole[1], across), rr=(whole[1], whole[1], diagonal)).items():
        expected[kind] = proj_oracle.proj_cells(a, b, cell, r2, pi_max)[2].sum()
        uncut[kind] = proj_oracle.proj_cells(a, b, cell, r2, float("inf"))[2].sum()
        assert min(proj_oracle.nearest_margin(a, b, cell, r2, pi_max)) > 1e-9
        assert expected[kind] > 100 and 0.3 < expected[kind] / uncut[kind] < 0.7  # pi_max cuts roughly half the pairs
    (cf,) = yaw.autocorrelate_projected(config, data, random, pi_max=pi_max)
    row, col = np.divmod(np.arange(WIDE_GRID**2), WIDE_GRID)
    apart = np.maximum(np.abs(row[:, None] - row[None, :]), np.abs(col[:, None] - col[None, :]))  # in patches, along either axis
    for kind in ("dd", "dr", "rr"):
        counts = getattr(cf, kind).counts.counts
        assert counts.shape == (1, WIDE_GRID**2, WIDE_GRID**2) and np.all(counts == np.rint(counts))
        assert counts.sum() == expected[kind], (kind, counts.sum(), expected[kind])
        assert counts[0][apart > 0].sum() >= 0.1 * counts.sum()  # a tenth of the member pairs between different patches
        assert counts[0][apart >= 2].sum() > 0  # ... and some between patches that share no boundary
        print(f"{kind}: {counts.sum():.0f} pairs, {counts[0][apart > 0].sum():.0f} between patches, {counts[0][apart >= 2].sum():.0f} past a neighbour")
    (planes,) = yaw.autocorrelate_projected(config, data, random, pi_max=pi_max, pi_bins=4)
    assert len(planes.pi_bins) == 4
    for kind in ("dd", "dr", "rr"):
        per_plane = [getattr(plane, kind).counts.counts for plane in planes.pi_bins]
        assert all(plane.sum() > 0 for plane in per_plane) and np.array_equal(sum(per_plane), getattr(cf, kind).counts.counts)
        assert sum(plane.sum() for plane in per_plane) == expected[kind]
    for cat in (data, random):
        cat.drop_layouts()
    return cf


def test_the_linkage_reaches_past_neighbouring_patches(stand_in, monkeypatch):
    import proj_pi_oracle

    monkeypatch.setattr(engine, "count_projected_pi_fine", proj_pi_oracle.count_projected_pi_fine)
    check_wide_linkage()


# --------------------------------------------------------------------------- 5. symmetry
def test_the_oracle_is_bit_symmetric_under_swapping_the_sides():
    a, b = proj_scenes.handle(proj_scenes.SEED_A, 4, 24), proj_scenes.handle(proj_scenes.SEED_B, 4, 24)
    r2 = proj_scenes.radius_edges(12, 4)
    cells = proj_scenes.cells_two_handles(4)
    forward = proj_oracle.proj_cells(a, b, cells, r2, proj_scenes.PMAX)
    swapped = proj_oracle.proj_cells(b, a, cells[:, [1, 0, 2, 3]], r2, proj_scenes.PMAX)
    assert forward[2].sum() > 1000
    # the same member pairs with the same terms; a cell's sum runs over them in another order, so W is compared pair by pair
    assert np.array_equal(forward[2], swapped[2])
    i, j = np.arange(len(a["x"]))[:, None], np.arange(len(b["x"]))[None, :]
    for one, other in zip(proj_oracle.pair_terms(a, b, i, j), proj_oracle.pair_terms(b, a, j.T, i.T)):
        assert np.array_equal(np.broadcast_to(one, (i.size, j.size)), np.broadcast_to(other, (j.size, i.size)).T)


# --------------------------------------------------------------------------- 6. error cases
def test_drivers_reject_what_they_cannot_use(stand_in, monkeypatch):
    data, random = driver_scenario()
    config = driver_config("kpc")
    angular = yaw.Configuration.create(rmin=[1.0], rmax=[5.0], unit="arcmin", edges=ZEDGES)
    with pytest.raises(ValueError, match="physical or comoving unit"):
        yaw.autocorrelate_projected(angular, data, random, pi_max=40.0)
    for bad in (0.0, -1.0, float("nan"), float("inf")):
        with pytest.raises(ValueError, match="pi_max"):
            yaw.autocorrelate_projected(config, data, random, pi_max=bad)
    with pytest.raises(TypeError):
        yaw.autocorrelate_projected(config, data, random)  # pi_max has no default
    kw = dict(patch_centers=yaw.AngularCoordinates(np.array(CENTERS)), degrees=False)
    ra, dec = np.array([c[0] for c in CENTERS]), np.array([c[1] for c in CENTERS])
    no_z = yaw.Catalog.from_arrays(ra, dec, **kw)
    with pytest.raises(ValueError, match="redshift"):
        yaw.autocorrelate_projected(config, no_z, random, pi_max=40.0)
    with pytest.raises(ValueError, match="redshift"):
        yaw.autocorrelate_projected(config, data, no_z, pi_max=40.0)
    wide = yaw.Configuration.create(rmin=[100.0], rmax=[1000.0], unit="kpc", edges=np.array([-0.1, 0.4, 0.6]), closed="left")
    at_zero = yaw.Catalog.from_arrays(ra, dec, redshifts=np.array([0.3, 0.0, 0.5]), **kw)
    with pytest.raises(ValueError, match="finite and > 0"):
        yaw.autocorrelate_projected(wide, at_zero, random, pi_max=40.0)
    # layouts without redshifts, or unbinned
    links = yaw.PatchLinkage.from_catalogs(config, data, random)
    data.build_trees(config.binning.edges)
    with pytest.raises(ValueError, match="with_redshifts"):
        links.count_projected_pairs(data, pi_max=40.0)
    data.build_trees(None, with_redshifts=True)
    with pytest.raises(ValueError, match="with_redshifts"):
        links.count_projected_pairs(data, pi_max=40.0)
    from yet_another_wizz_amd import parallel

    monkeypatch.setattr(parallel, "world", lambda: (0, 2))
    with pytest.raises(NotImplementedError):
        yaw.autocorrelate_projected(config, data, random, pi_max=40.0)
    with pytest.raises(NotImplementedError):
        links.count_projected_pairs(data, pi_max=40.0)


def test_an_object_too_close_for_the_largest_radius_is_named(stand_in):
    """2 Mpc around an object at z = 0.002 (8.9 Mpc away) is 13 degrees: beyond the cap, and the error says which object."""
    _, random = driver_scenario()
    config = yaw.Configuration.create(rmin=[100.0], rmax=[2000.0], unit="kpc", edges=np.array([0.001, 0.35, 0.65]))
    kw = dict(patch_centers=yaw.AngularCoordinates(np.array(CENTERS)), degrees=False)
    ra, dec = np.array([c[0] for c in CENTERS]), np.array([c[1] for c in CENTERS])
    near = yaw.Catalog.from_arrays(ra, dec, redshifts=np.array([0.3, 0.002, 0.5]), **kw)
    with pytest.raises(ValueError, match=r"too close for the largest radius.*bin 0 at z = 0\.002 .*R = 2 Mpc"):
        yaw.autocorrelate_projected(config, near, random, pi_max=40.0)
    with pytest.raises(ValueError, match="too close for the largest radius"):  # the randoms count too
        yaw.autocorrelate_projected(config, random, near, pi_max=40.0)
    # the seam itself refuses by the library's rule, through the engine's check
    layout = near.build_trees(config.binning.edges, with_redshifts=True)
    cells = np.array([(p * 2 + k, p * 2 + k, k, 1) for p in range(3) for k in range(2)])
    with pytest.raises(ValueError, match="too close"):
        proj_oracle.count_projected_fine(layout, layout, cells, np.array([[0.01, 4.0]] * 2), pi_max=40.0, cosmology=COSMO, unit="kpc")
    W, _ = proj_oracle.count_projected_fine(layout, layout, cells, np.array([[0.01, 0.04]] * 2), pi_max=40.0, cosmology=COSMO, unit="kpc")
    assert np.all(W == 0.0)


# --------------------------------------------------------------------------- 7. the oracle's membership, exactly
MARGIN = 1e-9


def exact_cells(a, b, cells, r2, pmax, same):
    """Per cell and fine bin the number of member pairs and the sum of ``w_a w_b``, with ``theta = 2 asin(chord / 2)``,
    ``R^2 = ((d_a + d_b) / 2)^2 theta^2`` and ``|c_a - c_b|`` of the float64 inputs at 50 digits; and the smallest relative
    distance of any pair from an edge > 0 of its row and from ``pmax``."""
    import mpmath

    mpmath.mp.dps = 50
    mpf = mpmath.mpf
    cols_a = {c: [mpf(float(v)) for v in a[c]] for c in "xyzdc"}
    cols_b = cols_a if same else {c: [mpf(float(v)) for v in b[c]] for c in "xyzdc"}
    wa = [mpf(1)] * len(a["x"]) if a["w"] is None else [mpf(float(v)) for v in a["w"]]
    wb = wa if same else ([mpf(1)] * len(b["x"]) if b["w"] is None else [mpf(float(v)) for v in b["w"]])
    nf = r2.shape[1] - 1
    count = np.zeros((len(cells), nf), dtype=np.int64)
    sums = [[mpf(0)] * nf for _ in cells]
    margin_r, margin_p, pm = mpf(1), mpf(1), mpf(pmax)
    for n, (sa, sb, row, diagonal) in enumerate(cells):
        edges = [mpf(float(v)) for v in r2[row]]
        for i in range(int(a["off"][sa]), int(a["off"][sa + 1])):
            ax, ay, az, ad, ac = (cols_a[c][i] for c in "xyzdc")
            for j in range(int(b["off"][sb]), int(b["off"][sb + 1])):
                if diagonal and j >= i:
                    break
                dx, dy, dz = ax - cols_b["x"][j], ay - cols_b["y"][j], az - cols_b["z"][j]
                theta = 2 * mpmath.asin(mpmath.sqrt(dx * dx + dy * dy + dz * dz) / 2)
                D = (ad + cols_b["d"][j]) / 2
                R2 = D * D * theta * theta
                p = abs(ac - cols_b["c"][j])
                margin_p = min(margin_p, abs(p / pm - 1))
                below = 0
                for edge in edges:
                    if edge > 0:
                        margin_r = min(margin_r, abs(R2 / edge - 1))
                    below += edge < R2
                if 0 < below <= nf and p <= pm:  # r2[below - 1] < R2 <= r2[below]
                    count[n, below - 1] += 1
                    sums[n][below - 1] += wa[i] * wb[j]
    return count, sums, float(margin_r), float(margin_p)


def test_the_oracles_membership_is_exact_on_the_device_scene():
    """For the scene of tests/test_gpu_projected.py (four redshift bins, twelve fine bins, one handle and two) every pair is
    classified at 50 digits: no pair lies within 1e-9 (relative) of an edge or of ``pmax`` -- a condition of the scene,
    asserted here and, in float64, by the device tests --, so the comparison leaves out nothing, and the oracle's integer
    count per cell and fine bin is the exact one. The oracle's weighted sums are then held against the exact sums: the worst
    ``|W - exact| / (eps A)`` is printed; four times it, rounded up to a power of two, is the ``K`` of the device tests."""
    nb, per_segment = 4, 24
    a, b = proj_scenes.handle(proj_scenes.SEED_A, nb, per_segment), proj_scenes.handle(proj_scenes.SEED_B, nb, per_segment)
    r2 = proj_scenes.radius_edges(12, nb)
    worst = 0.0
    for first, second, cells in ((a, a, proj_scenes.cells_one_handle(nb)), (a, b, proj_scenes.cells_two_handles(nb))):
        same = first is second
        count, sums, margin_r, margin_p = exact_cells(first, second, cells, r2, proj_scenes.PMAX, same)
        margin_64 = proj_oracle.nearest_margin(first, second, cells, r2, proj_scenes.PMAX)
        print(f"{'one handle' if same else 'two handles'}: {count.sum()} member pairs, nearest to an edge {margin_r:.3e}, to pmax {margin_p:.3e} "
              f"(float64: {margin_64[0]:.3e}, {margin_64[1]:.3e})")
        assert margin_r > MARGIN and margin_p > MARGIN and min(margin_64) > MARGIN
        W, A, N = proj_oracle.proj_cells(first, second, cells, r2, proj_scenes.PMAX)
        assert count.sum() > 3000 and np.count_nonzero(count) > 0.5 * count.size
        assert np.array_equal(N, count.astype(np.float64))
        N1 = proj_oracle.proj_cells(proj_scenes.unweighted(first), proj_scenes.unweighted(second), cells, r2, proj_scenes.PMAX, same=same)[0]
        assert np.array_equal(N1, N)  # unit weights: W is the count
        for n in range(len(cells)):
            for e in range(W.shape[1]):
                if A[n, e] > 0:
                    worst = max(worst, float(abs(sums[n][e] - float(W[n, e]))) / (EPS * A[n, e]))
    print(f"the oracle's worst |W - exact| / (eps A): {worst:.3f}")
    import test_gpu_projected

    assert worst <= test_gpu_projected.K_ORACLE_RATIO * 1.0000001  # the figure K was derived from still holds
    assert test_gpu_projected.K == 2.0 ** np.ceil(np.log2(4.0 * test_gpu_projected.K_ORACLE_RATIO))
