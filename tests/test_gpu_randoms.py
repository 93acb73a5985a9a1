"""GPU: BoxRandoms drawn on the device (yawhip_random_box, csrc/yawhip_random.hip) against numpy's own stream, bit for
bit -- values, indices, gathered attributes and the generator's end state -- and Catalog.from_random's device route
against its host route and against the reference (tests/golden/random_box.npz)."""
import numpy as np
import pytest

import yet_another_wizz_amd as yaw
from conftest import load_golden
from yet_another_wizz_amd import _lib, engine
from yet_another_wizz_amd.randoms import BoxRandoms

pytestmark = pytest.mark.gpu

BOX = (np.deg2rad(10.0), np.deg2rad(70.0), np.sin(np.deg2rad(-20.0)), np.sin(np.deg2rad(10.0)))


def start_state(seed, pending=False):
    rng = np.random.default_rng(np.random.SeedSequence(seed).spawn(1)[0])
    if pending:
        rng.integers(0, 5, size=1)  # leaves the high half of one output pending
        assert rng.bit_generator.state["has_uint32"] == 1
    return rng.bit_generator.state


def numpy_draw(state, n, chunksize, n_data, data_w, data_z):
    """What BoxRandoms.__call__ reads, chunk after chunk, from numpy itself."""
    rng = np.random.Generator(np.random.PCG64())
    rng.bit_generator.state = state
    xs, ys, idxs = [], [], []
    for lo in range(0, n, chunksize):
        k = min(chunksize, n - lo)
        xs.append(rng.uniform(BOX[0], BOX[1], k))
        ys.append(rng.uniform(BOX[2], BOX[3], k))
        if n_data != -1:
            idxs.append(rng.integers(0, n_data, size=k))
    idx = None if n_data == -1 else np.concatenate([np.empty(0, dtype=np.int64), *idxs])
    w = None if data_w is None else data_w[idx]
    z = None if data_z is None else data_z[idx]
    return np.concatenate(xs) if xs else np.empty(0), np.concatenate(ys) if ys else np.empty(0), w, z, idx, rng.bit_generator.state


def device_draw(state, n, chunksize, n_data, data_w, data_z, want_idx):
    return _lib.random_box(engine.get_context(engine.default_devices()[0]), n, chunksize, state, BOX[0], BOX[1] - BOX[0], BOX[2],
                           BOX[3] - BOX[2], n_data, data_w, data_z, want_idx=want_idx)


def check(state, n, chunksize, n_data=-1, weights=False, redshifts=False, want_idx=True):
    data = np.random.default_rng(n_data if n_data > 0 else 1).uniform(0.0, 2.0, (2, n_data)) if 0 < n_data <= 10**6 else None
    data_w = data[0] if weights else None
    data_z = data[1] if redshifts else None
    want_idx = want_idx and n_data != -1
    x, y, w, z, idx, end = device_draw(state, n, chunksize, n_data, data_w, data_z, want_idx)
    ex, ey, ew, ez, eidx, eend = numpy_draw(state, n, chunksize, n_data, data_w, data_z)
    assert np.array_equal(x, ex) and np.array_equal(y, ey)
    if want_idx:
        assert np.array_equal(idx, eidx)
    for got, exp in ((w, ew), (z, ez)):
        assert (got is None) == (exp is None) and (got is None or np.array_equal(got, exp))
    assert end == eend, (end, eend)


@pytest.mark.parametrize("n_data,weights,redshifts", [(-1, False, False), (1001, True, False), (1001, False, True),
                                                       (1001, True, True), (1, True, True)])
@pytest.mark.parametrize("chunksize", [1, 7, 7919, 9000])
def test_attached_values(n_data, weights, redshifts, chunksize):
    check(start_state(5), 9000, chunksize, n_data, weights, redshifts)


@pytest.mark.parametrize("n_data", [2, 1 << 31, 3_000_000_001, 1 << 32])
@pytest.mark.parametrize("pending", [False, True])
def test_bounded_indices(n_data, pending):
    """Rejections from none (2^32: raw draws) to ~30 % (3e9), with and without a pending half at the start."""
    for chunksize in (7, 7919, 50_001):
        check(start_state(11, pending), 50_001, chunksize, n_data)


@pytest.mark.parametrize("n", [0, 1, 2, 63, 64, 65, 255, 257, 4095, 4097, 8193, 1_000_003])
def test_sizes(n):
    check(start_state(n + 3, pending=n % 2 == 1), n, max(n, 1), 3_000_000_001)
    check(start_state(n + 4), n, 997, 1001, weights=True)


def test_large_chunks_take_several_windows():
    """2e7 bounded integers at 30 % rejection in one chunk read ~2.9e7 candidates: more than one window of the index
    pass, the continuation included; then the same in the default chunks of from_random."""
    check(start_state(21, pending=True), 20_000_000, 20_000_000, 3_000_000_001, want_idx=True)
    check(start_state(22), 20_000_000, 16_777_216, 1001, weights=True, redshifts=True)


def test_more_than_2_32_values_are_refused():
    with pytest.raises(_lib.YawhipError, match="2\\^32"):
        device_draw(start_state(1), 10, 10, (1 << 32) + 1, None, None, True)


def random_catalogues(num, chunksize=None, **patches):
    data = np.random.default_rng(5).uniform(0.2, 1.1, (2, 10_007))
    gen = BoxRandoms(10.0, 70.0, -20.0, 10.0, weights=data[0], redshifts=data[1], seed=99)
    dev = yaw.Catalog.from_random(None, gen, num, chunksize=chunksize, **patches)
    dev_state = gen.rng.bit_generator.state
    drawn, engine.draw_box_randoms = engine.draw_box_randoms, lambda *args, **kwargs: None
    try:
        host = yaw.Catalog.from_random(None, gen, num, chunksize=chunksize, **patches)
    finally:
        engine.draw_box_randoms = drawn
    assert dev._random_route == "device" and host._random_route == "host"
    assert dev_state == gen.rng.bit_generator.state
    return dev, host


def assert_same_catalogue(a, b):
    assert a.num_patches == b.num_patches
    assert a.get_num_records() == b.get_num_records() and a.get_sum_weights() == b.get_sum_weights()
    assert np.array_equal(a.get_centers().data, b.get_centers().data) and np.array_equal(a.get_radii().data, b.get_radii().data)
    for i in range(a.num_patches):
        pa, pb = a[i], b[i]
        for col in ("ra", "dec"):
            assert np.array_equal(getattr(pa.coords, col), getattr(pb.coords, col)), (i, col)
        assert np.array_equal(pa.weights, pb.weights) and np.array_equal(pa.redshifts, pb.redshifts), i


def test_from_random_device_route_is_the_host_route():
    other = yaw.Catalog.from_dataframe(None, dict(ra=np.linspace(12.0, 68.0, 300), dec=np.linspace(-18.0, 8.0, 300)),
                                       ra_name="ra", dec_name="dec", patch_num=6)
    assert_same_catalogue(*random_catalogues(300_001, chunksize=65_537, patch_centers=other))
    assert_same_catalogue(*random_catalogues(250_000, patch_num=5))


def test_from_random_device_route_at_5e7():
    centres = yaw.AngularCoordinates(np.deg2rad([[25.0, -5.0], [45.0, -12.0], [58.0, 3.0], [30.0, 5.0]]))
    assert_same_catalogue(*random_catalogues(50_000_000, patch_centers=centres))


def test_autocorrelate_with_device_randoms_reproduces_the_reference():
    fx = load_golden("random_box.npz")
    gen = BoxRandoms(*fx["box"], weights=fx["data_w"], redshifts=fx["data_z"], seed=int(fx["seed"]))
    centres = yaw.AngularCoordinates(fx["patch_centers"])
    rand = yaw.Catalog.from_random(None, gen, int(fx["num"]), patch_centers=centres, chunksize=int(fx["chunksize"]))
    assert rand._random_route == "device"
    state = gen.rng.bit_generator.state
    mask = (1 << 64) - 1
    s, inc = state["state"]["state"], state["state"]["inc"]
    assert [s >> 64, s & mask, inc >> 64, inc & mask, state["has_uint32"], state["uinteger"]] == fx["end_state"].tolist()
    frame = {c: fx[f"data.{c}"] for c in ("ra", "dec", "z", "w")}
    data = yaw.Catalog.from_dataframe(None, frame, ra_name="ra", dec_name="dec", weight_name="w", redshift_name="z",
                                      patch_centers=centres)
    config = yaw.Configuration.create(rmin=list(fx["config.rmin"]), rmax=list(fx["config.rmax"]), unit="arcmin", zmin=0.1,
                                      zmax=1.0, num_bins=4)
    for s, cf in enumerate(yaw.autocorrelate(config, data, rand, count_rr=True)):
        for kind in ("dd", "dr", "rr"):
            nc = getattr(cf, kind)
            np.testing.assert_allclose(nc.counts.counts.sum(axis=(1, 2)), fx[f"auto.s{s}.{kind}.counts"], rtol=1e-10)
            np.testing.assert_allclose(nc.sum_weights.sum_weights1, fx[f"auto.s{s}.{kind}.sum_weights1"], rtol=1e-12)
            np.testing.assert_allclose(nc.sum_weights.sum_weights2, fx[f"auto.s{s}.{kind}.sum_weights2"], rtol=1e-12)
