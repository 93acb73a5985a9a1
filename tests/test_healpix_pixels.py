"""CPU: HEALPix scalar maps as catalogues -- the host route of healpix.map_pixels (the oracle of yawhip_healpix_pixels): the
selection rule value by value, the output order in both schemes, the round trip through ang2pix / healpix_map, map_values,
Catalog.from_healpix_map and the library symbol's argument checks."""
import ctypes
import os

import numpy as np
import pytest

import yet_another_wizz_amd as yaw
from yet_another_wizz_amd import _lib, healpix
from yet_another_wizz_amd.randoms import nest2ring, pix2loc_nest

UNSEEN = -1.6375e30


@pytest.mark.parametrize("nested", [True, False])
@pytest.mark.parametrize("order", range(6))
def test_a_full_map_lists_every_pixel_in_nested_order(order, nested):
    npix = 12 << (2 * order)
    values = np.random.default_rng(order).normal(size=npix)
    ipix, phi, z, kappa, w = healpix.map_pixels(values, nested=nested)
    q = np.arange(npix, dtype=np.int64)
    assert w is None and ipix.dtype == np.int64 and all(c.dtype == np.float64 for c in (phi, z, kappa))
    assert np.array_equal(ipix, q if nested else nest2ring(order, q))
    assert np.array_equal(kappa, values[ipix])
    expect_phi, expect_z = pix2loc_nest(order, q)
    assert np.array_equal(phi, expect_phi) and np.array_equal(z, expect_z)
    assert np.array_equal(healpix.ang2pix(order, phi, z), q)
    assert np.array_equal(healpix.healpix_map(order, phi, z, kappa, nested=nested), values)


def test_the_selection_rule_value_by_value():
    assert healpix.UNSEEN == UNSEEN
    values = np.arange(1.0, 49.0)
    weights = np.ones(48)
    #               0       1        2        3       4     5        6     7
    values[:8] = [np.nan, np.inf, -np.inf, UNSEEN, -0.0, 5e-324, -3.25, 0.0]
    by_value = [False, False, False, False, True, True, True, True]
    #                  8    9     10      11      12      13
    weights[8:14] = [0.0, -1.0, np.nan, np.inf, 5e-324, 1.0]
    by_weight = [False, False, False, False, True, True]
    weights[4] = 0.0  # a valid value under a masked weight
    weights[0] = 2.0  # a masked value under a valid weight
    ipix, _, _, kappa, w = healpix.map_pixels(values, nested=True)
    assert np.array_equal(ipix, np.flatnonzero(by_value + [True] * 40))
    assert np.array_equal(kappa.view(np.int64), values[ipix].view(np.int64))  # -0.0 and the denormal arrive as they are
    ipix, _, _, kappa, w = healpix.map_pixels(values, weights, nested=True)
    expect = np.array(by_value + by_weight + [True] * 34)
    expect[4] = False
    assert np.array_equal(ipix, np.flatnonzero(expect))
    assert np.array_equal(kappa.view(np.int64), values[expect].view(np.int64)) and np.array_equal(w, weights[expect])
    assert healpix.count_selected(values, weights) == expect.sum() == 39  # 48 less four values, four weights and pixel 4


@pytest.mark.parametrize("order", [0, 2, 4])
def test_ring_and_nested_maps_of_one_sky_give_the_same_columns(order):
    npix = 12 << (2 * order)
    rng = np.random.default_rng(7 + order)
    nest_values, nest_weights = rng.normal(size=npix), rng.uniform(0.5, 2.0, npix)
    nest_values[rng.random(npix) < 0.3] = UNSEEN
    nest_weights[rng.random(npix) < 0.2] = 0.0
    to_ring = nest2ring(order, np.arange(npix))
    ring_values, ring_weights = np.empty(npix), np.empty(npix)
    ring_values[to_ring], ring_weights[to_ring] = nest_values, nest_weights
    for weights in (False, True):
        nest = healpix.map_pixels(nest_values, nest_weights if weights else None, nested=True)
        ring = healpix.map_pixels(ring_values, ring_weights if weights else None)  # RING is the default
        for a, b in zip(nest[1:], ring[1:]):
            assert (a is None and b is None and not weights) or np.array_equal(a, b)
        assert np.array_equal(ring[0], nest2ring(order, nest[0]))
        assert np.array_equal(nest[0], np.flatnonzero((nest_values != UNSEEN) & (nest_weights > 0 if weights else True)))


def test_errors():
    with pytest.raises(ValueError, match="every pixel is masked"):
        healpix.map_pixels(np.full(48, UNSEEN))
    with pytest.raises(ValueError, match="every pixel is masked"):
        healpix.map_pixels(np.ones(48), np.zeros(48))
    with pytest.raises(ValueError, match="no HEALPix map"):
        healpix.map_pixels(np.ones(47))
    with pytest.raises(ValueError, match="no HEALPix map"):
        healpix.map_pixels(np.ones(12 * 9))  # nside 3
    with pytest.raises(ValueError, match="one-dimensional"):
        healpix.map_pixels(np.ones((12, 4)))
    with pytest.raises(ValueError, match="weight map"):
        healpix.map_pixels(np.ones(48), np.ones(12))
    with pytest.raises(ValueError, match="order 13"):  # order 14, without the 25 GB: a broadcast view of one value
        healpix.map_pixels(np.broadcast_to(np.float64(1.0), (12 << 28,)))


def test_map_values_samples_the_map():
    order = 3
    npix = 12 << (2 * order)
    rng = np.random.default_rng(11)
    values = rng.normal(size=npix)
    phi, z = rng.uniform(-7.0, 7.0, 5000), rng.uniform(-1.0, 1.0, 5000)
    for nested in (True, False):
        assert np.array_equal(healpix.map_values(order, phi, z, values, nested=nested),
                              values[healpix.ang2pix(order, phi, z, nested=nested)])
    values[rng.random(npix) < 0.4] = np.nan
    ipix, phi, z, kappa, _ = healpix.map_pixels(values, nested=True)
    assert np.array_equal(healpix.map_values(order, phi, z, values), kappa)
    ring = np.empty(npix)
    ring[nest2ring(order, np.arange(npix))] = values
    assert np.array_equal(healpix.map_values(order, phi, z, ring, nested=False), kappa)
    ints = np.arange(npix)  # any dtype: a map of labels
    assert np.array_equal(healpix.map_values(order, phi, z, ints), ipix)
    with pytest.raises(ValueError, match="entries"):
        healpix.map_values(order, phi, z, values[:-1])


@pytest.mark.parametrize("with_weights", [False, True])
def test_catalog_from_healpix_map(with_weights):
    nside, npix = 8, 768
    rng = np.random.default_rng(3)
    values = rng.normal(size=npix)
    values[rng.random(npix) < 0.5] = UNSEEN
    weights = None
    if with_weights:
        weights = rng.uniform(0.5, 2.0, npix)
        weights[rng.random(npix) < 0.25] = 0.0
    selected = (values != UNSEEN) & (weights > 0 if with_weights else True)
    cat = yaw.Catalog.from_healpix_map(None, values, weights=weights, patch_num=4)  # a RING map
    assert cat.has_kappa and not cat.has_redshifts and cat.has_weights == with_weights
    assert cat.num_patches == 4 and sum(cat.get_num_records()) == selected.sum() == len(cat._ra)
    assert cat._random_route == "host"
    footprint = cat.healpix_map(nside, nested=False, weighted=False)
    assert np.array_equal(footprint, selected.astype(np.float64))
    if with_weights:
        assert np.array_equal(cat.healpix_map(nside, nested=False), np.where(selected, weights, 0.0))
    # every object carries its pixel's value
    assert np.array_equal(healpix.map_values(3, cat._ra, np.sin(cat._dec), values, nested=False), cat._k)
    same = yaw.Catalog.from_healpix_map(None, values, weights=weights, patch_centers=cat)
    assert np.array_equal(same._ra, cat._ra) and np.array_equal(same._k, cat._k)


def test_catalog_from_healpix_map_errors(tmp_path):
    from yet_another_wizz_amd.randoms import BoxRandoms

    with pytest.raises(ValueError) as from_random:
        yaw.Catalog.from_random(None, BoxRandoms(0, 1, 0, 1), 10)
    with pytest.raises(ValueError) as from_map:
        yaw.Catalog.from_healpix_map(None, np.ones(48))
    assert str(from_map.value) == str(from_random.value) == "no patch method specified"
    with pytest.raises(ValueError, match="every pixel is masked"):
        yaw.Catalog.from_healpix_map(None, np.full(48, np.nan), patch_num=2)
    cat = yaw.Catalog.from_healpix_map(tmp_path / "cache", np.arange(192.0), nested=True, patch_num=3)
    again = yaw.Catalog(tmp_path / "cache")
    assert again.has_kappa and np.array_equal(again._k, cat._k)


def test_the_driver_is_exported_and_needs_kappa_on_the_map_side():
    assert "crosscorrelate_scalar_map" in yaw.__all__ and callable(yaw.crosscorrelate_scalar_map)
    assert "reference" in yaw.crosscorrelate_scalar_map.__doc__
    cat = yaw.Catalog.from_healpix_map(None, np.arange(192.0), nested=True, patch_num=3)
    config = yaw.Configuration.create(rmin=100.0, rmax=1000.0, zmin=0.1, zmax=1.0, num_bins=2)
    with pytest.raises(ValueError, match="separate Catalog instance"):
        yaw.crosscorrelate_scalar_map(config, cat, cat)
    with pytest.raises(ValueError, match="redshifts"):  # the reference side must carry redshifts
        yaw.crosscorrelate_scalar_map(config, cat, yaw.Catalog.from_healpix_map(None, np.arange(192.0), nested=True, patch_centers=cat))


def test_healpix_pixels_symbol_is_declared_and_checks_its_arguments():
    header = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(_lib.__file__))), "include", "yawhip.h")
    with open(header) as f:
        text = f.read()
    assert "int yawhip_healpix_pixels(" in text and "#define YAWHIP_ABI_VERSION 6" in text
    assert "yawhip_healpix_pixels" in _lib.ABI_SYMBOLS and hasattr(ctypes.CDLL(_lib.LIB_PATH), "yawhip_healpix_pixels")
    lib = _lib.load_library()
    dp = ctypes.POINTER(ctypes.c_double)
    values = np.ones(48)
    n = ctypes.c_int64(-5)
    rc = lib.yawhip_healpix_pixels(None, 48, 0, values.ctypes.data_as(dp), None, 1, 1, 0, None, None, None, None, None, ctypes.byref(n))
    assert rc == -1 and b"NULL" in lib.yawhip_last_error()  # YAWHIP_ERR_INVALID: no context
