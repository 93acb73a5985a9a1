"""GPU: HEALPix pixels and maps on the device (yawhip_healpix_map, csrc/yawhip_healpix.hip) against the host route's plain
numpy, bit for bit -- pixels in both numberings, exact counts, weighted sums in np.bincount's order whatever the pass
size -- then Catalog.healpix_map's device route against its host route, and catalogue -> footprint -> randoms ->
autocorrelate inside the package."""
import functools

import numpy as np
import pytest

import yet_another_wizz_amd as yaw
from yet_another_wizz_amd import _lib, engine, healpix
from yet_another_wizz_amd.randoms import HealPixRandoms, pix2loc_nest

pytestmark = pytest.mark.gpu

TWOPI = 2.0 * np.pi
N_BIG = 300_000


def edge_points():
    """Every edge longitude with every edge latitude: the belt / cap boundary, the poles and the equator with their float64
    neighbours; the seam at 0 and 2 pi from both sides, values outside [0, 2 pi), the multiples of pi / 2 and theirs."""
    third = 2.0 / 3.0
    zs = [0.0, -0.0, 1.0, -1.0, np.nextafter(1.0, 0.0), np.nextafter(-1.0, 0.0)]
    for v in (third, -third):
        zs += [v, np.nextafter(v, 0.0), np.nextafter(v, 2.0 * v)]
    phis = [0.0, np.nextafter(TWOPI, 0.0), TWOPI, np.nextafter(TWOPI, 7.0), -1e-20, 7.0, -7.0, 1e-300, 100.0, -100.0]
    for k in range(-4, 9):
        v = k * (np.pi / 2)
        phis += [v, np.nextafter(v, -100.0), np.nextafter(v, 100.0)]
    phi, z = np.meshgrid(np.array(phis), np.array(zs))
    return phi.ravel(), z.ravel()


@functools.lru_cache(maxsize=None)
def points():
    """N_BIG points: uniform on the sphere (longitudes also outside [0, 2 pi)), then, at the end, the edge set and the
    centres of all pixels of orders 2 .. 5 (the grandchildren of orders 0 .. 3). Read-only."""
    rng = np.random.default_rng(2025)
    special = [edge_points()] + [pix2loc_nest(o, np.arange(12 << (2 * o))) for o in range(2, 6)]
    n_special = sum(len(p) for p, _ in special)
    phi = np.concatenate([rng.uniform(-TWOPI, 2 * TWOPI, N_BIG - n_special)] + [p for p, _ in special])
    z = np.concatenate([rng.uniform(-1.0, 1.0, N_BIG - n_special)] + [v for _, v in special])
    w = 10.0 ** rng.uniform(-6.0, 6.0, N_BIG)  # twelve decades: the order of a sum shows in its last bits
    for a in (phi, z, w):
        a.setflags(write=False)
    return phi, z, w


@functools.lru_cache(maxsize=None)
def host_pixels(order, nested):
    phi, z, _ = points()
    return on_host(healpix.ang2pix, order, phi, z, nested=nested)


def on_host(fn, *args, **kwargs):
    """``fn`` with the device route switched off."""
    device, engine.healpix_map = engine.healpix_map, lambda *a, **k: None
    try:
        return fn(*args, **kwargs)
    finally:
        engine.healpix_map = device


def context():
    return engine.get_context(engine.default_devices()[0])


@pytest.mark.parametrize("nested", [True, False])
@pytest.mark.parametrize("order", [0, 1, 3, 6, 10, 13])
def test_pixels_are_the_host_routes(order, nested):
    phi, z, _ = points()
    expect = host_pixels(order, nested)
    assert expect.min() >= 0 and expect.max() < 12 << (2 * order)
    for n in (1, 255, 256, 257, N_BIG):
        lo = N_BIG - n  # the special points are at the end
        pix, none = _lib.healpix_map(context(), phi[lo:], z[lo:], None, order, nested, want_pixels=True, want_map=False)
        assert none is None and pix.dtype == np.int64 and np.array_equal(pix, expect[lo:]), n
    got = healpix.ang2pix(order, phi, z, nested=nested)  # the public function takes the device route at this size
    assert np.array_equal(got, expect)


@pytest.mark.parametrize("nested", [True, False])
@pytest.mark.parametrize("order", [0, 3, 6, 10])
def test_counts_and_weighted_sums_are_bincount(order, nested):
    phi, z, w = points()
    npix = 12 << (2 * order)
    expect = host_pixels(order, nested)
    pix, counts = _lib.healpix_map(context(), phi, z, None, order, nested, want_pixels=True)
    assert np.array_equal(pix, expect)
    assert counts.dtype == np.float64 and np.array_equal(counts, np.bincount(expect, minlength=npix))
    _, sums = _lib.healpix_map(context(), phi, z, w, order, nested)
    assert np.array_equal(sums, np.bincount(expect, w, minlength=npix))  # order 0: runs of 25 000 weights
    _, again = _lib.healpix_map(context(), phi, z, w, order, nested)
    assert np.array_equal(again, sums)
    assert np.array_equal(healpix.healpix_map(order, phi, z, w, nested=nested), sums)
    assert np.array_equal(healpix.healpix_map(order, phi, z, nested=nested), counts)


@pytest.mark.parametrize("chunksize", [1, 7, 4096, 10_000, 0])
def test_the_map_is_carried_across_passes(chunksize):
    phi, z, w = (a[-10_000:] for a in points())
    for order in (0, 3, 10) if chunksize == 0 or chunksize >= 4096 else (3,):  # 10 000 passes of one object: one order
        npix = 12 << (2 * order)
        expect = host_pixels(order, True)[-10_000:]
        pix, sums = _lib.healpix_map(context(), phi, z, w, order, True, want_pixels=True, chunksize=chunksize)
        assert np.array_equal(pix, expect) and np.array_equal(sums, np.bincount(expect, w, minlength=npix))
        _, counts = _lib.healpix_map(context(), phi, z, None, order, True, chunksize=chunksize)
        assert np.array_equal(counts, np.bincount(expect, minlength=npix))


def test_invalid_points_get_minus_one_and_stay_out_of_the_map():
    phi, z, w = (a[:5000].copy() for a in points())
    bad_phi, bad_z = [3, 1000, 4999], [0, 17, 2500, 4998]
    phi[bad_phi] = [np.nan, np.inf, -np.inf]
    z[bad_z] = [np.nan, 1.0000000000000002, -1.5, np.inf]
    good = np.ones(5000, dtype=bool)
    good[bad_phi + bad_z] = False
    for order, nested in ((0, True), (6, False), (13, True)):
        npix = 12 << (2 * order)
        expect = on_host(healpix.ang2pix, order, phi[good], z[good], nested=nested)
        with_map = order < 13
        pix, counts = _lib.healpix_map(context(), phi, z, None, order, nested, want_pixels=True, want_map=with_map, chunksize=999)
        assert np.all(pix[~good] == -1) and np.array_equal(pix[good], expect)
        if with_map:
            assert np.array_equal(counts, np.bincount(expect, minlength=npix))
            _, sums = _lib.healpix_map(context(), phi, z, w, order, nested, chunksize=999)
            assert np.array_equal(sums, np.bincount(expect, w[good], minlength=npix))


def test_device_keeps_the_argument_checks():
    phi, z, _ = (a[:10] for a in points())
    with pytest.raises(_lib.YawhipError, match="order"):
        _lib.healpix_map(context(), phi, z, None, 14, True, want_pixels=True, want_map=False)
    with pytest.raises(_lib.YawhipError, match="both NULL"):
        _lib.healpix_map(context(), phi, z, None, 3, True, want_pixels=False, want_map=False)
    with pytest.raises(_lib.YawhipError, match="chunksize"):
        _lib.healpix_map(context(), phi, z, None, 3, True, chunksize=-1)
    pix, counts = _lib.healpix_map(context(), phi[:0], z[:0], None, 2, True, want_pixels=True)
    assert len(pix) == 0 and counts.shape == (192,) and not counts.any()


def clustered_box(n_clumps=10_000, per_clump=20, seed=3):
    """~2e5 objects in clumps of 3 arcmin inside ra 10 .. 70, dec -5 .. 25 degrees, with weights and redshifts."""
    rng = np.random.default_rng(seed)
    ra0 = np.deg2rad(rng.uniform(10.0, 70.0, n_clumps))
    dec0 = np.arcsin(rng.uniform(np.sin(np.deg2rad(-5.0)), np.sin(np.deg2rad(25.0)), n_clumps))
    sigma = np.deg2rad(3.0 / 60.0)
    n = n_clumps * per_clump
    return dict(ra=np.repeat(ra0, per_clump) + sigma * rng.normal(size=n), dec=np.repeat(dec0, per_clump) + sigma * rng.normal(size=n),
                z=np.repeat(rng.uniform(0.15, 0.95, n_clumps), per_clump), w=10.0 ** rng.uniform(-2.0, 2.0, n))


def test_catalog_map_device_route_is_the_host_route():
    frame = clustered_box(15_000)  # 3e5 objects
    centres = yaw.AngularCoordinates(np.deg2rad([[20.0, 0.0], [20.0, 18.0], [40.0, 10.0], [60.0, 2.0], [58.0, 20.0]]))
    cat = yaw.Catalog.from_dataframe(None, frame, ra_name="ra", dec_name="dec", weight_name="w", patch_centers=centres,
                                     degrees=False)
    calls = []
    device = engine.healpix_map
    engine.healpix_map = lambda *args, **kwargs: calls.append(device(*args, **kwargs)) or calls[-1]
    try:
        maps = [cat.healpix_map(256), cat.healpix_map(256, nested=False), cat.healpix_map(256, weighted=False), cat.healpix_map(1)]
    finally:
        engine.healpix_map = device
    assert len(calls) == 4 and all(c is not None for c in calls)
    host = [on_host(cat.healpix_map, 256), on_host(cat.healpix_map, 256, nested=False), on_host(cat.healpix_map, 256, weighted=False),
            on_host(cat.healpix_map, 1)]
    for got, expect in zip(maps, host):
        assert np.array_equal(got, expect)
    assert maps[2].sum() == 300_000


def test_catalogue_to_footprint_to_randoms_to_autocorrelation():
    frame = clustered_box()
    centres = yaw.AngularCoordinates(np.deg2rad([[20.0, 0.0], [20.0, 18.0], [40.0, 10.0], [60.0, 2.0], [58.0, 20.0]]))
    data = yaw.Catalog.from_dataframe(None, frame, ra_name="ra", dec_name="dec", redshift_name="z", patch_centers=centres,
                                      degrees=False)
    gen = HealPixRandoms.from_catalog(data, 64, redshifts=frame["z"], seed=5)
    occupied = np.flatnonzero(data.healpix_map(64))
    assert np.array_equal(gen._ipix_unmasked, occupied) and 0 < len(occupied) < 12 * 64 * 64 // 4
    rand = yaw.Catalog.from_random(None, gen, 300_000, patch_centers=data)
    assert rand._random_route == "device" and rand.num_patches == data.num_patches
    assert np.all(np.isin(np.flatnonzero(rand.healpix_map(64)), occupied))
    config = yaw.Configuration.create(rmin=1.0, rmax=10.0, unit="arcmin", zmin=0.1, zmax=1.0, num_bins=3)
    (cf,) = yaw.autocorrelate(config, data, rand)
    assert isinstance(cf, yaw.CorrFunc)
    sample = cf.sample().data
    assert np.all(np.isfinite(sample)) and np.all(sample > 0)  # clumps of 3 arcmin: an excess of close pairs
