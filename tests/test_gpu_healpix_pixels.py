"""GPU: the unmasked pixels of a HEALPix scalar map compacted on the device (yawhip_healpix_pixels, csrc/yawhip_healpix.hip)
against the host route's plain numpy, bit for bit -- every order of pass and workgroup boundary, both schemes, the
capacity check -- then Catalog.from_healpix_map's device route against its host route and crosscorrelate_scalar_map end
to end."""
import functools

import numpy as np
import pytest

import yet_another_wizz_amd as yaw
from yet_another_wizz_amd import _lib, engine, healpix
from yet_another_wizz_amd.randoms import nest2ring, pix2loc_nest

pytestmark = pytest.mark.gpu

UNSEEN = -1.6375e30
VALUE_SPECIALS = [np.nan, np.inf, -np.inf, UNSEEN, -0.0, 5e-324, -3.25, 0.0]
WEIGHT_SPECIALS = [0.0, -1.0, np.nan, np.inf, 5e-324, 1.0]


def on_host(fn, *args, **kwargs):
    """``fn`` with the device route switched off."""
    device, engine.healpix_pixels = engine.healpix_pixels, lambda *a, **k: None
    try:
        return fn(*args, **kwargs)
    finally:
        engine.healpix_pixels = device


def context():
    return engine.get_context(engine.default_devices()[0])


def assert_same(got, expect, what=""):
    """All five columns, the floats also bit by bit."""
    assert len(got) == len(expect) == 5
    for name, a, b in zip(("ipix", "phi", "z", "kappa", "w"), got, expect):
        if b is None:
            assert a is None, (what, name)
            continue
        assert a.dtype == b.dtype and np.array_equal(a, b), (what, name)
        if name in ("phi", "z"):
            assert np.array_equal(a.view(np.int64), b.view(np.int64)), (what, name)


def to_ring(order, nest_map):
    ring = np.empty_like(nest_map)
    ring[nest2ring(order, np.arange(len(nest_map)))] = nest_map
    return ring


@functools.lru_cache(maxsize=None)
def masked_maps(order):
    """A NESTED map of ``order`` with a random 50 % mask and the special values sprinkled in, and its weight map with
    theirs; the last pixel is data under weight 1 (the map is never empty). Read-only."""
    npix = 12 << (2 * order)
    rng = np.random.default_rng(100 + order)
    values, weights = rng.normal(size=npix), rng.uniform(0.5, 2.0, npix)
    values[rng.random(npix) < 0.5] = UNSEEN
    for column, specials in ((values, VALUE_SPECIALS), (weights, WEIGHT_SPECIALS)):
        for rep in range(max(1, min(4, npix // 64))):
            where = rng.permutation(npix - 1)[: len(specials)]
            column[where] = specials[: len(where)]
    values[-1], weights[-1] = 0.75, 1.0
    values.setflags(write=False)
    weights.setflags(write=False)
    return values, weights


@pytest.mark.parametrize("with_weights", [False, True])
@pytest.mark.parametrize("nested", [True, False])
@pytest.mark.parametrize("order", [0, 1, 3, 5, 8])
def test_pixels_are_the_host_routes(order, nested, with_weights):
    values, weights = masked_maps(order)
    if not nested:
        values, weights = to_ring(order, values), to_ring(order, weights)
    weights = weights if with_weights else None
    expect = on_host(healpix.map_pixels, values, weights, nested=nested)
    assert 0 < len(expect[0]) < len(values) or order == 0
    got = engine.healpix_pixels(values, weights, order, nested)
    assert_same(got, expect)
    assert np.array_equal(got[3].view(np.int64), values[got[0]].view(np.int64))  # -0.0 and the denormal as they are


def test_passes_of_any_size_give_the_same_columns():
    order = 3  # 768 pixels
    values, weights = (to_ring(order, m) for m in masked_maps(order))
    expect = on_host(healpix.map_pixels, values, weights)
    for chunksize in (1, 7, 64, 255, 256, 257, 768, 0):
        assert_same(engine.healpix_pixels(values, weights, order, False, chunksize=chunksize), expect, chunksize)
    with pytest.raises(_lib.YawhipError, match="chunksize"):
        engine.healpix_pixels(values, weights, order, False, chunksize=-1)


def _selections():
    """name -> (selected nested pixels of an order-5 map, chunksize)."""
    npix = 12 << 10
    rng = np.random.default_rng(55)
    cases = {"first": ([0], 0), "last": ([npix - 1], 0), "middle": ([6143], 0), "every second": (np.arange(0, npix, 2), 0),
             "all": (np.arange(npix), 0),
             # pass 0 and the head of pass 1, passes 2 and 3 empty, then the middle of pass 4
             "blocks around empty passes": (np.concatenate([np.arange(100, 300), np.arange(1100, 1250)]), 256)}
    for count in (63, 64, 65, 255, 256, 257):
        cases[f"{count} in the first 512"] = (np.sort(rng.choice(512, count, replace=False)), 0)
    return cases


@pytest.mark.parametrize("case", list(_selections()))
def test_compaction_boundaries(case):
    order, npix = 5, 12 << 10
    chosen, chunksize = _selections()[case]
    chosen = np.asarray(chosen, dtype=np.int64)
    rng = np.random.default_rng(len(chosen))
    nest_map = np.full(npix, UNSEEN)
    nest_map[chosen] = rng.normal(size=len(chosen))
    nest_w = rng.uniform(0.5, 2.0, npix)
    phi, z = pix2loc_nest(order, chosen)
    for nested in (True, False):
        values, weights = (nest_map, nest_w) if nested else (to_ring(order, nest_map), to_ring(order, nest_w))
        expect = (chosen if nested else nest2ring(order, chosen), phi, z, nest_map[chosen], nest_w[chosen])
        assert_same(on_host(healpix.map_pixels, values, weights, nested=nested), expect, "host")
        assert_same(engine.healpix_pixels(values, weights, order, nested, chunksize=chunksize), expect, nested)
        assert_same(engine.healpix_pixels(values, None, order, nested, chunksize=chunksize), (*expect[:4], None), nested)


def _sentinel_outputs(n):
    return (np.full(n, -7, dtype=np.int64), *(np.full(n, -7.0) for _ in range(4)))


def test_all_masked_returns_zero_and_writes_nothing():
    order, npix = 3, 768
    values = np.full(npix, UNSEEN)
    values[::3], values[1::3] = np.nan, np.inf
    outputs = _sentinel_outputs(16)
    for chunksize in (0, 100):
        n, *_ = _lib.healpix_pixels(context(), values, None, order, True, 0, chunksize=chunksize, outputs=outputs)
        assert n == 0 and all(np.all(o == -7) for o in outputs)
    n, *_ = _lib.healpix_pixels(context(), np.ones(npix), np.zeros(npix), order, False, 0, outputs=outputs)
    assert n == 0 and all(np.all(o == -7) for o in outputs)
    with pytest.raises(ValueError, match="every pixel is masked"):
        engine.healpix_pixels(values, None, order, True)
    with pytest.raises(ValueError, match="every pixel is masked"):
        engine.healpix_pixels(np.ones(npix), np.zeros(npix), order, True)
    big = np.full(12 << 16, UNSEEN)  # large enough for the public function's device route
    assert len(big) >= healpix.DEVICE_PIXELS_MIN
    with pytest.raises(ValueError, match="every pixel is masked"):
        healpix.map_pixels(big)


@pytest.mark.parametrize("chunksize", [0, 64])
def test_a_capacity_one_short_is_an_error_and_not_a_write(chunksize):
    order = 3
    values, weights = masked_maps(order)
    expect = on_host(healpix.map_pixels, values, weights, nested=True)
    true = len(expect[0])
    assert true > 64
    outputs = _sentinel_outputs(true + 10)
    with pytest.raises(_lib.YawhipError, match="capacity"):
        _lib.healpix_pixels(context(), values, weights, order, True, true - 1, chunksize=chunksize, outputs=outputs)
    assert all(np.all(o[true - 1:] == -7) for o in outputs)  # nothing at or beyond the capacity
    if chunksize == 0:  # one pass: it did not fit, nothing of it was copied
        assert all(np.all(o == -7) for o in outputs)
    with pytest.raises(_lib.YawhipError, match="sized for"):  # one too many: the counts differ, the tail stays
        _lib.healpix_pixels(context(), values, weights, order, True, true + 1, chunksize=chunksize, outputs=outputs)
    assert all(np.all(o[true:] == -7) for o in outputs)
    n, *got = _lib.healpix_pixels(context(), values, weights, order, True, true, chunksize=chunksize, outputs=outputs)
    assert n == true and all(np.all(o[true:] == -7) for o in outputs)
    assert_same(tuple(o[:true] for o in got), expect)


def test_device_keeps_the_argument_checks():
    values = np.ones(768)
    with pytest.raises(_lib.YawhipError, match="order"):
        _lib.healpix_pixels(context(), values, None, 14, True, 768)
    with pytest.raises(_lib.YawhipError, match="n_pix"):
        _lib.healpix_pixels(context(), values, None, 4, True, 768)
    with pytest.raises(_lib.YawhipError, match="n_pix"):
        _lib.healpix_pixels(context(), values[:-1], None, 3, True, 767)
    with pytest.raises(_lib.YawhipError, match="chunksize"):
        _lib.healpix_pixels(context(), values, None, 3, True, 768, chunksize=-1)


def test_order_11_ring_map_with_a_few_pixels():
    """5e7 pixels, 400 MB, three passes: element offsets beyond 2^31 bytes; the expectation comes from the chosen pixels."""
    order = 11
    nside, npix = 1 << order, 12 << (2 * order)
    ncap = 2 * nside * (nside - 1)
    # centres of the ring pixels on either side of the two cap boundaries (the closed form of the ring scheme) -> nested
    fact2 = 4.0 / npix
    nr = nside - 1
    cap_z, belt_z = 1.0 - nr * nr * fact2, 2.0 / 3.0
    first_cap, last_cap = 0.5 * (np.pi / 2) / nr, (4 * nr - 0.5) * (np.pi / 2) / nr
    first_belt, last_belt = 0.5 * (np.pi / 2) / nside, (4 * nside - 0.5) * (np.pi / 2) / nside
    edge = healpix.ang2pix(order, np.array([last_cap, first_belt, last_belt, first_cap]),
                           np.array([cap_z, belt_z, -belt_z, -cap_z]))
    assert np.array_equal(nest2ring(order, edge), [ncap - 1, ncap, npix - ncap - 1, npix - ncap])
    rng = np.random.default_rng(11)
    chosen = np.unique(np.concatenate([[0, npix - 1], edge, rng.integers(0, npix, 100_000)]))
    ring = nest2ring(order, chosen)
    kappa = rng.normal(size=len(chosen))
    values = np.full(npix, UNSEEN)
    values[ring] = kappa
    phi, z = pix2loc_nest(order, chosen)
    got = engine.healpix_pixels(values, None, order, False)
    assert_same(got, (ring, phi, z, kappa, None))


def _smooth_map(nside, seed):
    """A NESTED map of a smooth field with a masked half sky and holes, and a coverage map with empty pixels."""
    order = nside.bit_length() - 1
    npix = 12 * nside * nside
    rng = np.random.default_rng(seed)
    phi, z = pix2loc_nest(order, np.arange(npix))
    values = 0.3 * np.sin(3.0 * phi) * (1.0 - z * z) + 0.1 * z + 0.02 * rng.normal(size=npix)
    values[z < -0.1] = UNSEEN
    values[rng.random(npix) < 0.05] = np.nan
    weights = rng.uniform(0.2, 1.0, npix)
    weights[rng.random(npix) < 0.1] = 0.0
    return values, weights


def test_catalog_from_map_device_route_is_the_host_route():
    nside = 256
    values, weights = _smooth_map(nside, 5)
    values, weights = to_ring(8, values), to_ring(8, weights)
    centres = yaw.AngularCoordinates(np.deg2rad([[30.0, 10.0], [120.0, 40.0], [200.0, 5.0], [290.0, 60.0], [330.0, 20.0], [80.0, 75.0]]))
    for wmap in (None, weights):
        dev = yaw.Catalog.from_healpix_map(None, values, weights=wmap, patch_centers=centres, chunksize=100_000)
        host = on_host(yaw.Catalog.from_healpix_map, None, values, weights=wmap, patch_centers=centres)
        assert dev._random_route == "device" and host._random_route == "host"
        assert dev.has_kappa and not dev.has_redshifts and dev.has_weights == (wmap is not None)
        assert np.array_equal(dev._patch_off, host._patch_off) and dev.get_num_records() == host.get_num_records()
        for a, b in ((dev._ra, host._ra), (dev._dec, host._dec), (dev._k, host._k), (dev._w, host._w)):
            assert (a is None and b is None) or np.array_equal(a.view(np.int64), b.view(np.int64))
        selected = np.isfinite(values) & (values != UNSEEN) & (True if wmap is None else wmap > 0)
        assert np.array_equal(dev.healpix_map(nside, nested=False, weighted=False), selected.astype(np.float64))


def _reference_box(n, seed, *, patch_num=None, patch_centers=None):
    """``n`` objects with redshifts, uniform in ra 10 .. 30, dec 0 .. 20 degrees."""
    rng = np.random.default_rng(seed)
    ra = rng.uniform(10.0, 30.0, n)
    dec = np.rad2deg(np.arcsin(rng.uniform(0.0, np.sin(np.deg2rad(20.0)), n)))
    return yaw.Catalog.from_arrays(ra, dec, redshifts=rng.uniform(0.1, 1.0, n), patch_num=patch_num, patch_centers=patch_centers)


def _box_map(nside, field):
    """NESTED map with ``field(phi, z)`` at the pixels whose centres lie in the box of ``_reference_box``, UNSEEN elsewhere."""
    phi, z = pix2loc_nest(nside.bit_length() - 1, np.arange(12 * nside * nside))
    inside = (phi >= np.deg2rad(10.0)) & (phi <= np.deg2rad(30.0)) & (z >= 0.0) & (z <= np.sin(np.deg2rad(20.0)))
    return np.where(inside, field(phi, z), UNSEEN)


def test_a_constant_field_correlates_to_exactly_zero():
    reference = _reference_box(20_000, 1, patch_num=8)
    values = _box_map(256, lambda phi, z: np.full_like(phi, 0.5))
    kappa_map = yaw.Catalog.from_healpix_map(None, values, nested=True, patch_centers=reference)
    assert kappa_map._random_route == "device" and kappa_map.num_patches == 8
    config = yaw.Configuration.create(rmin=10.0, rmax=60.0, unit="arcmin", zmin=0.1, zmax=1.0, num_bins=3)
    (cf,) = yaw.crosscorrelate_scalar_map(config, reference, kappa_map)
    assert isinstance(cf, yaw.ScalarCorrFunc) and cf.dr is not None
    nk, nn = cf.dd.kappa_counts.counts, cf.dd.number_counts.counts  # [B, P, P]
    assert np.array_equal(nk * 2.0, np.round(nk * 2.0)) and np.array_equal(nn, np.round(nn))  # multiples of 0.5: exact sums
    assert np.array_equal(nk, 0.5 * nn)
    sum_nk, sum_nn = nk.sum(axis=(1, 2)), nn.sum(axis=(1, 2))
    assert np.all(sum_nn > 0)  # every bin has pairs at these scales
    assert np.array_equal(sum_nk / sum_nn, np.full(3, 0.5))
    sample = cf.sample()
    assert np.array_equal(sample.data, np.zeros(3)) and np.array_equal(sample.samples, np.zeros_like(sample.samples))


def test_driver_on_device_and_host_map_catalogues_and_by_hand():
    reference = _reference_box(20_000, 2, patch_num=6)
    ref_rand = _reference_box(40_000, 3, patch_centers=reference)
    values = _box_map(256, lambda phi, z: 0.3 * np.sin(40.0 * phi) + z)
    weights = np.where(values != UNSEEN, 0.5 + np.abs(np.sin(np.arange(len(values)))), 0.0)
    dev_map = yaw.Catalog.from_healpix_map(None, values, weights=weights, nested=True, patch_centers=reference)
    host_map = on_host(yaw.Catalog.from_healpix_map, None, values, weights=weights, nested=True, patch_centers=reference)
    assert dev_map._random_route == "device" and host_map._random_route == "host"
    config = yaw.Configuration.create(rmin=10.0, rmax=60.0, unit="arcmin", zmin=0.1, zmax=1.0, num_bins=3)
    (dev_cf,) = yaw.crosscorrelate_scalar_map(config, reference, dev_map, ref_rand=ref_rand)
    (host_cf,) = yaw.crosscorrelate_scalar_map(config, reference, host_map, ref_rand=ref_rand)
    assert dev_cf == host_cf
    # by hand: the "nk" DD, and DR from the two counts of the randoms against the map
    links = yaw.PatchLinkage.from_catalogs(config, reference, dev_map, ref_rand)
    (dd,) = links.count_scalar_pairs(reference, dev_map, mode="nk")
    (dr_nk,) = links.count_pairs(ref_rand, dev_map, mode="nk")
    (dr_nn,) = links.count_pairs(ref_rand, dev_map, mode="nn")
    by_hand = yaw.ScalarCorrFunc(dd, yaw.NormalisedScalarCounts(dr_nk.counts, dr_nn.counts))
    assert dev_cf == by_hand
    assert np.all(np.isfinite(dev_cf.sample().data)) and np.any(dev_cf.sample().data != 0.0)
    # without randoms the mean field per patch takes DR's place
    (mean_cf,) = yaw.crosscorrelate_scalar_map(config, reference, dev_map)
    assert mean_cf.dd == dev_cf.dd and mean_cf.dr == yaw.compute_scalar_normalisation(dev_map, config.binning.binning)
