"""GPU: HealPixRandoms drawn on the device (yawhip_random_healpix, csrc/yawhip_random.hip) against the host route's plain
numpy, bit for bit -- coordinates, order-29 pixels, indices, gathered attributes and the generator's end state -- then
Catalog.from_random's device route against its host route, and one autocorrelation on mask-drawn randoms."""
import functools

import numpy as np
import pytest

import yet_another_wizz_amd as yaw
from yet_another_wizz_amd import _lib, engine
from yet_another_wizz_amd.randoms import HealPixRandoms, pix2loc_nest

pytestmark = pytest.mark.gpu


@functools.lru_cache(maxsize=None)
def generator(name):
    """Nested maps. The caps and the belt of nside 8 reach both cap branches, belt rings of either kshift and the wrap of the
    position in a ring (face 4 starts west of phi = 0). 65 535 and 65 536 unmasked pixels lie on either side of a power of two
    in the depth of the search; the nside 1024 mask searches 20 levels deep."""
    if name == "nside1":
        return HealPixRandoms(np.ones(12), nested=True)
    if name == "nside2_single":
        values = np.zeros(48)
        values[29] = 0.3
        return HealPixRandoms(values, nested=True)
    if name in ("nside8_caps", "nside8_belt"):
        _, z = pix2loc_nest(3, np.arange(768))
        caps = np.abs(z) > 2.0 / 3.0
        return HealPixRandoms((caps if name == "nside8_caps" else ~caps).astype(float), nested=True, is_mask=True)
    if name == "nside64_dynamic":
        values = 10.0 ** np.random.default_rng(64).uniform(-6.0, 0.0, 12 * 64 * 64)
        values[::5] = 0.0
        return HealPixRandoms(values, nested=True)
    if name in ("nside128_65535", "nside128_65536"):
        values = np.zeros(12 * 128 * 128)
        values[100_000 : 100_000 + int(name[-5:])] = np.random.default_rng(128).uniform(0.5, 1.5, int(name[-5:]))
        return HealPixRandoms(values, nested=True)
    if name == "nside1024_mask":
        npix = 12 * 1024 * 1024
        values = np.zeros(npix)
        values[npix // 3 : npix // 3 + npix // 20] = 1.0  # 5 % of the sky, across the face 3 / face 4 seam
        values[npix // 3 + 1000 : npix // 3 + npix // 20 : 7] = 0.0
        return HealPixRandoms(values, nested=True, is_mask=True)
    raise KeyError(name)


MAPS = ["nside1", "nside2_single", "nside8_caps", "nside8_belt", "nside64_dynamic", "nside128_65535", "nside128_65536",
        "nside1024_mask"]


def start_state(seed, pending=False):
    rng = np.random.default_rng(np.random.SeedSequence(seed).spawn(1)[0])
    if pending:
        rng.integers(0, 5, size=1)  # leaves the high half of one output pending
        assert rng.bit_generator.state["has_uint32"] == 1
    return rng.bit_generator.state


def host_draw(gen, state, n, chunksize, n_data):
    """The host route chunk after chunk: pixels, then indices."""
    gen.rng.bit_generator.state = state
    pix, idx = [np.empty(0, dtype=np.int64)], [np.empty(0, dtype=np.int64)]
    for lo in range(0, n, chunksize):
        k = min(chunksize, n - lo)
        pix.append(gen._draw_pixels(k))
        if n_data != -1:
            idx.append(gen.rng.integers(0, n_data, size=k))
    pix = np.concatenate(pix)
    x, y = pix2loc_nest(29, pix)
    return x, y, pix, (None if n_data == -1 else np.concatenate(idx)), gen.rng.bit_generator.state


def check(name, state, n, chunksize, n_data=-1, weights=False, redshifts=False):
    gen = generator(name)
    data = np.random.default_rng(n_data).uniform(0.0, 2.0, (2, n_data)) if 0 < n_data <= 10**6 else None
    data_w = data[0] if weights else None
    data_z = data[1] if redshifts else None
    ctx = engine.get_context(engine.default_devices()[0])
    x, y, w, z, idx, pix, end = _lib.random_healpix(ctx, n, chunksize, state, gen.order, gen._ipix_unmasked, gen._cdf, n_data,
                                                    data_w, data_z, want_idx=n_data != -1, want_pix=True)
    ex, ey, epix, eidx, eend = host_draw(gen, state, n, chunksize, n_data)
    assert np.array_equal(pix, epix)
    assert np.array_equal(x, ex) and np.array_equal(y, ey)
    if n_data != -1:
        assert np.array_equal(idx, eidx)
    for got, values in ((w, data_w), (z, data_z)):
        assert (got is None) == (values is None) and (got is None or np.array_equal(got, values[eidx]))
    assert end == eend, (end, eend)


@pytest.mark.parametrize("n", [0, 1, 257, 300_000])
@pytest.mark.parametrize("name", MAPS)
def test_maps_and_sizes(name, n):
    for chunksize in ([1] if 0 < n <= 257 else []) + [7919, max(n, 1)]:
        check(name, start_state(n + 5), n, chunksize, 1001, weights=True, redshifts=True)


@pytest.mark.parametrize("n_data,weights,redshifts", [
    (-1, False, False), (1, True, True), (1, False, True), (1001, True, False), (1001, False, True), (1001, True, True),
    (1001, False, False), (1 << 31, False, False)])  # without arrays the indices alone are drawn and compared
def test_attached_values(n_data, weights, redshifts):
    for n, chunksize in ((257, 1), (300_000, 7919), (300_000, 300_000)):
        check("nside8_caps", start_state(13), n, chunksize, n_data, weights, redshifts)


@pytest.mark.parametrize("name", ["nside8_belt", "nside1024_mask"])
def test_pending_half_at_the_start(name):
    for n_data in (1001, 1 << 31):
        for chunksize in (7919, 300_000):
            check(name, start_state(17, pending=True), 300_000, chunksize, n_data)


def test_device_keeps_the_order_and_map_checks():
    ctx = engine.get_context(engine.default_devices()[0])
    with pytest.raises(_lib.YawhipError, match="order"):
        _lib.random_healpix(ctx, 10, 10, start_state(1), 14, np.zeros(1, dtype=np.int64), np.ones(1))
    with pytest.raises(_lib.YawhipError, match="no pixel"):
        _lib.random_healpix(ctx, 10, 10, start_state(1), 0, np.array([12]), np.ones(1))
    with pytest.raises(_lib.YawhipError, match="cdf"):
        _lib.random_healpix(ctx, 10, 10, start_state(1), 0, np.array([3, 4]), np.array([0.5, 0.9]))
    with pytest.raises(_lib.YawhipError, match="2\\^32"):
        _lib.random_healpix(ctx, 10, 10, start_state(1), 0, np.array([3]), np.ones(1), (1 << 32) + 1)


def both_routes(gen, num, chunksize=None, **patches):
    dev = yaw.Catalog.from_random(None, gen, num, chunksize=chunksize, **patches)
    dev_state = gen.rng.bit_generator.state
    drawn, engine.draw_healpix_randoms = engine.draw_healpix_randoms, lambda *args, **kwargs: None
    try:
        host = yaw.Catalog.from_random(None, gen, num, chunksize=chunksize, **patches)
    finally:
        engine.draw_healpix_randoms = drawn
    assert dev._random_route == "device" and host._random_route == "host"
    assert dev_state == gen.rng.bit_generator.state
    return dev, host


def survey_mask():
    """nside 64: a footprint of 60 x 30 degrees around (40, 10) with a completeness gradient."""
    phi, z = pix2loc_nest(6, np.arange(12 * 64 * 64))
    inside = (np.abs(phi - np.deg2rad(40.0)) < np.deg2rad(30.0)) & (np.abs(np.arcsin(z) - np.deg2rad(10.0)) < np.deg2rad(15.0))
    return inside * (0.5 + 0.5 * phi)


def test_from_random_device_route_is_the_host_route():
    data = np.random.default_rng(5).uniform(0.2, 1.1, (2, 10_007))
    gen = HealPixRandoms(survey_mask(), nested=True, weights=data[0], redshifts=data[1], seed=99)
    centres = yaw.AngularCoordinates(np.deg2rad([[20.0, 0.0], [20.0, 18.0], [40.0, 10.0], [60.0, 2.0], [58.0, 20.0]]))
    dev, host = both_routes(gen, 300_000, chunksize=65_537, patch_centers=centres)
    assert dev.num_patches == host.num_patches == 5 and dev.get_num_records() == host.get_num_records()
    for i in range(dev.num_patches):
        for col in ("ra", "dec"):
            assert np.array_equal(getattr(dev[i].coords, col), getattr(host[i].coords, col)), (i, col)
        assert np.array_equal(dev[i].weights, host[i].weights) and np.array_equal(dev[i].redshifts, host[i].redshifts), i


def test_autocorrelate_with_mask_drawn_randoms():
    """A clustered sky inside the mask (pairs of points 2 arcmin apart) against randoms from the mask: finite counts, an
    excess of close pairs, and one CorrFunc whichever route drew the randoms."""
    mask = survey_mask()
    z_values = np.random.default_rng(8).uniform(0.15, 0.95, 5000)
    seeds = HealPixRandoms(mask, nested=True, redshifts=z_values, seed=1)(20_000)
    shift = np.deg2rad(2.0 / 60.0)
    frame = dict(ra=np.concatenate([seeds["ra"], seeds["ra"] + shift]), dec=np.concatenate([seeds["dec"], seeds["dec"]]),
                 z=np.concatenate([seeds["redshifts"], seeds["redshifts"]]))
    centres = yaw.AngularCoordinates(np.deg2rad([[20.0, 0.0], [20.0, 18.0], [40.0, 10.0], [60.0, 2.0], [58.0, 20.0]]))
    data = yaw.Catalog.from_dataframe(None, frame, ra_name="ra", dec_name="dec", redshift_name="z", patch_centers=centres,
                                      degrees=False)
    gen = HealPixRandoms(mask, nested=True, redshifts=z_values, seed=2)
    config = yaw.Configuration.create(rmin=1.0, rmax=10.0, unit="arcmin", zmin=0.1, zmax=1.0, num_bins=3)
    results = [yaw.autocorrelate(config, data, rand)[0] for rand in both_routes(gen, 100_000, patch_centers=centres)]
    for kind in ("dd", "dr", "rr"):
        a, b = (getattr(cf, kind) for cf in results)
        assert np.all(np.isfinite(a.counts.counts)) and a.counts.counts.sum() > 0
        assert np.array_equal(a.counts.counts, b.counts.counts)
        assert np.array_equal(a.sum_weights.sum_weights1, b.sum_weights.sum_weights1)
        assert np.array_equal(a.sum_weights.sum_weights2, b.sum_weights.sum_weights2)
    sample = results[0].sample().data
    assert np.all(np.isfinite(sample)) and np.all(sample > 0)
