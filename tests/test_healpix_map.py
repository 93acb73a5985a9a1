"""healpix.ang2pix / healpix.healpix_map on the host route (plain numpy, no healpy), Catalog.healpix_map and
HealPixRandoms.from_catalog: pixel centres map to themselves and to their ancestors, the ring numbers agree with the paper's
closed form (Gorski et al. 2005, eqs. 2-9, written here) and with nest2ring, the edges of the belt, the poles and the
phi = 0 seam stay inside the map, and a map is np.bincount of the pixels. No GPU."""
import ctypes
import math

import numpy as np
import pytest

import yet_another_wizz_amd as yaw
from yet_another_wizz_amd import _lib, healpix
from yet_another_wizz_amd.randoms import HealPixRandoms, nest2ring, pix2loc_nest

PI = np.pi
TWOPI = 2.0 * np.pi


def ring_pix2ang(nside, p):
    """(phi, z) of ring-scheme pixel p, scalar, from the paper's closed form."""
    npix, ncap = 12 * nside * nside, 2 * nside * (nside - 1)
    if p < ncap or p >= npix - ncap:
        q = p if p < ncap else npix - 1 - p  # the south cap mirrors the north cap
        i = (1 + math.isqrt(1 + 2 * q)) // 2
        j = q + 1 - 2 * i * (i - 1)
        z = 1.0 - i * i / (3.0 * nside * nside)
        if p >= ncap:
            z, j = -z, 4 * i + 1 - j
        return PI / (2 * i) * (j - 0.5), z
    q = p - ncap
    i = q // (4 * nside) + nside
    j = q % (4 * nside) + 1
    s = (i - nside + 1) % 2  # 1: the ring's first centre is half a pixel from phi = 0; 0: it is at phi = 0
    return PI / (2 * nside) * (j - 1 + s / 2.0), 4.0 / 3.0 - 2.0 * i / (3.0 * nside)


def edge_points():
    """(phi, z): every edge longitude with every edge latitude. Latitudes: the belt / cap boundary and its float64
    neighbours, the poles and theirs, the equator. Longitudes: the seam at 0 and 2 pi from both sides, values outside
    [0, 2 pi), and every multiple of pi / 2 (the base-pixel corners) with its neighbours."""
    third = 2.0 / 3.0
    zs = [0.0, -0.0, 1.0, -1.0, np.nextafter(1.0, 0.0), np.nextafter(-1.0, 0.0)]
    for v in (third, -third):
        zs += [v, np.nextafter(v, 0.0), np.nextafter(v, 2.0 * v)]
    phis = [0.0, np.nextafter(TWOPI, 0.0), TWOPI, np.nextafter(TWOPI, 7.0), -1e-20, 7.0, -7.0, 1e-300, 100.0, -100.0]
    for k in range(-4, 9):
        v = k * (PI / 2)
        phis += [v, np.nextafter(v, -100.0), np.nextafter(v, 100.0)]
    phi, z = np.meshgrid(np.array(phis), np.array(zs))
    return phi.ravel(), z.ravel()


def reduced(phi):
    """phi brought to [0, 2 pi) by the documented steps."""
    r = np.fmod(phi, TWOPI)
    r = np.where(r < 0.0, r + TWOPI, r)
    return np.where(r >= TWOPI, 0.0, r)


def sphere_points(n, seed):
    rng = np.random.default_rng(seed)
    return rng.uniform(-10.0, 10.0, n), rng.uniform(-1.0, 1.0, n)


# ---- pixels ----
@pytest.mark.parametrize("order", range(7))
def test_every_pixel_centre_maps_to_itself(order):
    ipix = np.arange(12 << (2 * order))
    phi, z = pix2loc_nest(order, ipix)
    got = healpix.ang2pix(order, phi, z)
    assert got.dtype == np.int64 and np.array_equal(got, ipix)
    assert np.array_equal(healpix.ang2pix(order, phi, z, nested=False), nest2ring(order, ipix))


@pytest.mark.parametrize("order", range(5))
def test_grandchild_centres_map_to_their_ancestor(order):
    """The 16 order + 2 pixels inside every pixel: their centres reach every belt and cap branch of every face."""
    fine = np.arange(12 << (2 * (order + 2)))
    phi, z = pix2loc_nest(order + 2, fine)
    assert np.array_equal(healpix.ang2pix(order, phi, z), fine >> 4)
    assert np.array_equal(healpix.ang2pix(order, phi + TWOPI, z), fine >> 4)  # two roundings of 1e-16 against a centre's margin


@pytest.mark.parametrize("order", range(6))
def test_ring_centres_of_the_closed_form_map_to_their_own_number(order):
    nside, npix = 1 << order, 12 << (2 * order)
    centres = np.array([ring_pix2ang(nside, p) for p in range(npix)])
    assert np.array_equal(healpix.ang2pix(order, centres[:, 0], centres[:, 1], nested=False), np.arange(npix))


@pytest.mark.parametrize("order", [0, 1, 4, 9, 13])
def test_ring_is_nest2ring_of_nested_on_random_points(order):
    phi, z = sphere_points(100_000, order)
    nested = healpix.ang2pix(order, phi, z)
    assert nested.min() >= 0 and nested.max() < 12 << (2 * order)
    assert np.array_equal(healpix.ang2pix(order, phi, z, nested=False), nest2ring(order, nested))


@pytest.mark.parametrize("order", [0, 1, 2, 5, 10, 13])
def test_edges_stay_inside_the_map(order):
    npix = 12 << (2 * order)
    phi, z = edge_points()
    for nested in (True, False):
        pix = healpix.ang2pix(order, phi, z, nested=nested)
        assert pix.min() >= 0 and pix.max() < npix
        assert np.array_equal(pix, healpix.ang2pix(order, reduced(phi), z, nested=nested))
    # the pole pixels: z = +-1 lies in the cap pixel nearest the pole of the face phi points into
    nside = 1 << order
    for quadrant in range(4):
        at = quadrant * PI / 2 + 0.3
        north, south = healpix.ang2pix(order, [at, at], [1.0, -1.0])
        assert north == quadrant * nside * nside + nside * nside - 1 and south == (8 + quadrant) * nside * nside


def test_just_below_zero_is_the_pixel_of_zero():
    _, z = edge_points()
    for order in (0, 3, 13):
        for nested in (True, False):
            below = healpix.ang2pix(order, np.full_like(z, -1e-20), z, nested=nested)
            assert np.array_equal(below, healpix.ang2pix(order, np.zeros_like(z), z, nested=nested))


def test_belt_and_cap_branches_agree_where_they_meet():
    """|z| = 2/3 is the centre line of ring nside (and 3 nside): a point just inside the belt branch and the point just
    inside the cap branch at the same longitude are in the same pixel, away from that ring's pixel boundaries."""
    phi = np.random.default_rng(23).uniform(0.0, TWOPI, 2000)
    for order in (0, 3, 6, 13):
        nside = 1 << order
        for sign in (1.0, -1.0):
            third = sign * 2.0 / 3.0
            belt = healpix.ang2pix(order, phi, np.full_like(phi, np.nextafter(third, 0.0)), nested=False)
            cap = healpix.ang2pix(order, phi, np.full_like(phi, np.nextafter(third, 2.0 * third)), nested=False)
            ring_start = 2 * nside * (nside - 1) if sign > 0 else 12 * nside * nside - 2 * nside * (nside + 1)
            assert np.array_equal(belt, cap) and np.all((belt >= ring_start) & (belt < ring_start + 4 * nside))


# ---- maps ----
@pytest.mark.parametrize("nested", [True, False])
@pytest.mark.parametrize("order", [0, 2, 7])
def test_map_is_bincount_of_the_pixels(order, nested):
    npix = 12 << (2 * order)
    phi, z = sphere_points(30_000, 100 + order)
    w = 10.0 ** np.random.default_rng(order).uniform(-6.0, 6.0, len(phi))
    pix = healpix.ang2pix(order, phi, z, nested=nested)
    counts = healpix.healpix_map(order, phi, z, nested=nested)
    assert counts.dtype == np.float64 and counts.shape == (npix,) and counts.sum() == len(phi)
    assert np.array_equal(counts, np.bincount(pix, minlength=npix))
    sums = healpix.healpix_map(order, phi, z, w, nested=nested)
    assert sums.dtype == np.float64 and np.array_equal(sums, np.bincount(pix, w, minlength=npix))
    empty = healpix.healpix_map(order, [], [])
    assert empty.shape == (npix,) and not empty.any()


def small_catalog(weights=True):
    rng = np.random.default_rng(42)
    n = 5000
    frame = dict(ra=rng.uniform(0.2, 1.3, n), dec=np.arcsin(rng.uniform(-0.2, 0.9, n)), w=10.0 ** rng.uniform(-3.0, 3.0, n))
    centres = yaw.AngularCoordinates([[0.4, 0.0], [0.8, 0.5], [1.2, 0.2]])
    cat = yaw.Catalog.from_dataframe(None, frame, ra_name="ra", dec_name="dec", weight_name="w" if weights else None,
                                     patch_centers=centres, degrees=False)
    return cat, frame


def test_catalog_map_agrees_with_the_function():
    cat, frame = small_catalog()
    ra = np.concatenate([cat[i].coords.ra for i in cat])  # the catalogue's own order: patch after patch
    dec = np.concatenate([cat[i].coords.dec for i in cat])
    w = np.concatenate([cat[i].weights for i in cat])
    for nested in (True, False):
        pix = healpix.ang2pix(4, ra, np.sin(dec), nested=nested)
        assert np.array_equal(cat.healpix_map(16, nested=nested), np.bincount(pix, w, minlength=3072))
        assert np.array_equal(cat.healpix_map(16, nested=nested, weighted=False), np.bincount(pix, minlength=3072))
    # whatever the order of the objects: the same counts, the same sums up to their rounding
    unordered = healpix.healpix_map(4, frame["ra"], np.sin(frame["dec"]), frame["w"])
    np.testing.assert_allclose(cat.healpix_map(16), unordered, rtol=1e-12)
    plain, _ = small_catalog(weights=False)
    assert np.array_equal(plain.healpix_map(16), cat.healpix_map(16, weighted=False))
    assert plain.healpix_map(1).tolist().count(0.0) < 12 and plain.healpix_map(1).sum() == 5000


def test_catalog_map_rejects_a_bad_nside():
    cat, _ = small_catalog()
    for nside in (0, -4, 3, 12, 16384, 2.0, "8", True):
        with pytest.raises(ValueError, match="nside"):
            cat.healpix_map(nside)
    assert healpix.nside2order(8192) == 13 and cat.healpix_map(1024, weighted=False).sum() == 5000


def test_randoms_from_a_catalogue_fall_into_its_pixels(monkeypatch):
    from yet_another_wizz_amd import engine

    monkeypatch.setattr(engine, "draw_healpix_randoms", lambda *args, **kwargs: None)
    cat, _ = small_catalog()
    occupied = np.flatnonzero(cat.healpix_map(32))
    gen = HealPixRandoms.from_catalog(cat, 32, redshifts=np.linspace(0.1, 1.0, 50), seed=7)
    assert (gen.nside, gen.order, gen.seed) == (32, 5, 7) and gen.has_redshifts and not gen.has_weights
    assert np.array_equal(gen._ipix_unmasked, occupied)
    assert np.array_equal(gen._cdf, np.arange(1, len(occupied) + 1) / len(occupied))  # a mask: every occupied pixel alike
    chunk = gen(20_000)
    assert np.all(np.isin(healpix.ang2pix(5, chunk["ra"], np.sin(chunk["dec"])), occupied))
    rand = yaw.Catalog.from_random(None, gen, 20_000, patch_centers=cat)
    assert rand._random_route == "host" and rand.num_patches == cat.num_patches
    assert np.all(np.isin(np.flatnonzero(rand.healpix_map(32)), occupied))


def test_randoms_from_a_catalogue_follow_its_weights():
    """Two pixels of nside 2 with 100 objects each, weights 1 and 3: drawn 1 : 3 as a probability map, 1 : 1 as a mask."""
    (phi_a, phi_b), (z_a, z_b) = pix2loc_nest(1, np.array([17, 22]))
    frame = dict(ra=np.repeat([phi_a, phi_b], 100), dec=np.arcsin(np.repeat([z_a, z_b], 100)), w=np.repeat([1.0, 3.0], 100))
    cat = yaw.Catalog.from_dataframe(None, frame, ra_name="ra", dec_name="dec", weight_name="w", degrees=False,
                                     patch_centers=yaw.AngularCoordinates([[phi_a, np.arcsin(z_a)]]))
    weighted = HealPixRandoms.from_catalog(cat, 2, is_mask=False)
    assert np.array_equal(weighted._ipix_unmasked, [17, 22]) and np.array_equal(weighted._cdf, [0.25, 1.0])
    mask = HealPixRandoms.from_catalog(cat, 2)
    assert np.array_equal(mask._ipix_unmasked, [17, 22]) and np.array_equal(mask._cdf, [0.5, 1.0])
    n = 40_000
    for gen, p in ((weighted, 0.25), (mask, 0.5)):
        drawn = gen._draw_pixels(n) >> 56
        assert abs(np.count_nonzero(drawn == 17) - n * p) <= 5 * math.sqrt(n * p * (1 - p))


# ---- errors and the symbol ----
def test_errors():
    phi, z = sphere_points(10, 1)
    for order in (-1, 14):
        with pytest.raises(ValueError, match="order"):
            healpix.ang2pix(order, phi, z)
    for bad in (1.0000000000000002, -1.5, np.nan, np.inf):
        with pytest.raises(ValueError, match="sin"):
            healpix.ang2pix(3, phi, np.where(np.arange(10) == 4, bad, z))
    for bad in (np.nan, np.inf, -np.inf):
        with pytest.raises(ValueError, match="phi"):
            healpix.healpix_map(3, np.where(np.arange(10) == 9, bad, phi), z)
    with pytest.raises(ValueError, match="equal length"):
        healpix.ang2pix(3, phi, z[:9])
    with pytest.raises(ValueError, match="weights"):
        healpix.healpix_map(3, phi, z, np.ones(9))
    with pytest.raises(ValueError, match="equal length"):
        healpix.ang2pix(3, phi.reshape(2, 5), z.reshape(2, 5))


def test_healpix_map_symbol_loads_and_checks_its_arguments():
    lib = _lib.load_library()
    assert "yawhip_healpix_map" in _lib.ABI_SYMBOLS and hasattr(ctypes.CDLL(_lib.LIB_PATH), "yawhip_healpix_map")
    assert "healpix" in yaw.__all__ and yaw.healpix is healpix
    phi, z, pix = np.zeros(4), np.zeros(4), np.zeros(4, dtype=np.int64)
    dp, ip = ctypes.POINTER(ctypes.c_double), ctypes.POINTER(ctypes.c_int64)
    rc = lib.yawhip_healpix_map(None, 4, 0, phi.ctypes.data_as(dp), z.ctypes.data_as(dp), None, 3, 1, pix.ctypes.data_as(ip), None)
    assert rc == -1 and b"NULL" in lib.yawhip_last_error()  # YAWHIP_ERR_INVALID: no context
