"""BoxRandoms and Catalog.from_random on the host route, against the reference's own draws and catalogue
(tests/golden/random_box.npz, tools/make_golden.py --random-box). No GPU: the device route is forced off where a test
asserts the host route, so that these tests mean the same on a machine with a GPU."""
import ctypes
import hashlib

import numpy as np
import pytest

import yet_another_wizz_amd as yaw
from conftest import load_golden
from yet_another_wizz_amd import _lib, engine
from yet_another_wizz_amd.randoms import BoxRandoms


@pytest.fixture(scope="module")
def fixture():
    return load_golden("random_box.npz")


def generator(fx):
    return BoxRandoms(*fx["box"], weights=fx["data_w"], redshifts=fx["data_z"], seed=int(fx["seed"]))


def state_words(state):
    mask = (1 << 64) - 1
    s, inc = state["state"]["state"], state["state"]["inc"]
    return [s >> 64, s & mask, inc >> 64, inc & mask, state["has_uint32"], state["uinteger"]]


@pytest.fixture
def host_only(monkeypatch):
    monkeypatch.setattr(engine, "draw_box_randoms", lambda *args, **kwargs: None)


def test_first_call_is_the_references_bit_for_bit(fixture):
    gen = generator(fixture)
    chunk = gen(len(fixture["first.ra"]))
    assert sorted(chunk) == ["dec", "ra", "redshifts", "weights"]
    for name in ("ra", "dec", "weights", "redshifts"):
        assert chunk[name].dtype == np.float64
        assert np.array_equal(chunk[name], fixture[f"first.{name}"]), name


def records_sha256(ra, weights, redshifts):
    """SHA-256 of the float64 rows (ra, weights, redshifts) in ascending ra, as tools/make_golden.py stores it."""
    order = np.argsort(ra, kind="stable")
    rows = np.ascontiguousarray(np.column_stack([ra[order], weights[order], redshifts[order]]), dtype="<f8")
    return hashlib.sha256(rows.tobytes()).hexdigest()


def test_from_random_host_route_is_the_references_catalogue(fixture, host_only):
    """Per patch the same records (the reference orders a patch by an unstable argsort, so rows are compared in ra order):
    ra / weights / redshifts of every record exact (digest), a sample of every 64th record in ra order stored in full with dec
    within 1 ulp (numpy's arcsin dispatches per CPU); the generator's end state exact."""
    gen = generator(fixture)
    gen(17)  # from_random reseeds: what was drawn before does not matter
    cat = yaw.Catalog.from_random(None, gen, int(fixture["num"]), patch_centers=yaw.AngularCoordinates(fixture["patch_centers"]),
                                  chunksize=int(fixture["chunksize"]))
    assert cat._random_route == "host"
    assert cat.has_weights and cat.has_redshifts
    assert np.array_equal(np.array(cat.get_num_records()), fixture["random.meta.num_records"])
    for i in range(cat.num_patches):
        patch = cat[i]
        sample = np.argsort(patch.coords.ra, kind="stable")[::64]
        assert np.array_equal(patch.coords.ra[sample], fixture[f"patch_{i}.sample.ra"])
        dec, ref_dec = patch.coords.dec[sample], fixture[f"patch_{i}.sample.dec"]
        assert np.all(np.abs(dec - ref_dec) <= np.spacing(np.abs(ref_dec)))
        assert records_sha256(patch.coords.ra, patch.weights, patch.redshifts) == str(fixture[f"patch_{i}.sha256"])
    assert state_words(gen.rng.bit_generator.state) == fixture["end_state"].tolist()
    assert np.array_equal(cat.get_centers().data, fixture["random.meta.centers"])
    np.testing.assert_allclose(cat.get_radii().data, fixture["random.meta.radii"], rtol=1e-14)
    np.testing.assert_allclose(np.array(cat.get_sum_weights()), fixture["random.meta.sum_weights"], rtol=1e-13)


def test_from_random_writes_a_cache_and_takes_centres_of_a_catalogue(tmp_path, fixture, host_only):
    gen = BoxRandoms(10.0, 40.0, -5.0, 5.0, seed=3)
    first = yaw.Catalog.from_random(None, gen, 5000, patch_num=4, chunksize=999)
    assert first.num_patches == 4 and not first.has_weights and not first.has_redshifts
    cat = yaw.Catalog.from_random(tmp_path / "rand", gen, 5000, patch_centers=first, chunksize=999)
    assert np.array_equal(cat.get_centers().data, first.get_centers().data)
    back = yaw.Catalog(tmp_path / "rand")
    for i in range(cat.num_patches):
        assert np.array_equal(back[i].coords.ra, cat[i].coords.ra)
        assert np.array_equal(back[i].coords.dec, cat[i].coords.dec)
    with pytest.raises(FileExistsError):
        yaw.Catalog.from_random(tmp_path / "rand", gen, 5000, patch_centers=first)
    yaw.Catalog.from_random(tmp_path / "rand", gen, 5000, patch_centers=first, overwrite=True)


def test_chunked_draws_follow_one_stream(host_only):
    """from_random's chunks continue the stream (the pending 32-bit half included): the same values as calling the
    generator chunk by chunk after a reseed, whatever the chunk size."""
    data = np.linspace(0.0, 1.0, 77)
    gen = BoxRandoms(0.0, 90.0, -30.0, 30.0, weights=data, seed=9)
    cats = [yaw.Catalog.from_random(None, gen, 1000, patch_centers=yaw.AngularCoordinates([[0.5, 0.0]]), chunksize=c)
            for c in (1000, 333)]
    gen.reseed()
    draws = [gen(k) for k in (333, 333, 333, 1)]
    assert np.array_equal(cats[1][0].coords.ra, np.concatenate([d["ra"] for d in draws]))
    assert np.array_equal(cats[1][0].weights, np.concatenate([d["weights"] for d in draws]))
    assert not np.array_equal(cats[0][0].weights, cats[1][0].weights)  # a call of 1000 reads the stream differently


def test_errors():
    with pytest.raises(ValueError, match="does not match"):
        BoxRandoms(0.0, 10.0, 0.0, 10.0, weights=np.ones(5), redshifts=np.ones(6))
    gen = BoxRandoms(0.0, 10.0, 0.0, 10.0)
    with pytest.raises(ValueError, match="empty"):
        yaw.Catalog.from_random(None, gen, 0, patch_num=2)
    with pytest.raises(ValueError, match="no patch method"):
        yaw.Catalog.from_random(None, gen, 100)


def test_attributes_and_reseed():
    w = np.arange(10.0)
    gen = BoxRandoms(5.0, 15.0, -10.0, 20.0, weights=w, seed=7)
    assert gen.seed == 7 and gen.has_weights and not gen.has_redshifts and gen.data_size == 10
    assert BoxRandoms(0.0, 1.0, 0.0, 1.0).data_size == -1
    assert gen.x_min == np.deg2rad(5.0) and gen.y_max == np.sin(np.deg2rad(20.0))
    a = gen(100)
    gen.reseed()
    b = gen(100)
    assert all(np.array_equal(a[k], b[k]) for k in a)
    gen.reseed(8)
    assert gen.seed == 8 and not np.array_equal(gen(100)["ra"], a["ra"])
    expect = np.random.default_rng(np.random.SeedSequence(8).spawn(1)[0]).uniform(gen.x_min, gen.x_max, 5)
    gen.reseed()
    assert np.array_equal(gen(5)["ra"], expect)


def test_generate_dataframe_in_degrees():
    gen = BoxRandoms(5.0, 15.0, -10.0, 20.0, redshifts=np.linspace(0.1, 1.0, 9), seed=11)
    df = gen.generate_dataframe(500)
    assert list(df.columns) == ["ra", "dec", "redshifts"]
    assert df["ra"].between(5.0, 15.0).all() and df["dec"].between(-10.0, 20.0).all()
    gen.reseed()
    rad = gen.generate_dataframe(500, degrees=False)
    assert np.array_equal(df["ra"].to_numpy(), np.rad2deg(rad["ra"].to_numpy()))


def test_random_box_symbol_loads_and_checks_its_arguments():
    lib = _lib.load_library()
    assert "yawhip_random_box" in _lib.ABI_SYMBOLS
    state = (ctypes.c_uint64 * 4)(0, 0, 0, 1)
    out = (ctypes.c_uint64 * 2)()
    rc = lib.yawhip_random_box(None, 10, 10, state, 0, 0, 0.0, 1.0, 0.0, 1.0, -1, None, None, None, None, None, None, None, out,
                               ctypes.byref(ctypes.c_int32()), ctypes.byref(ctypes.c_uint32()))
    assert rc == -1 and b"NULL" in lib.yawhip_last_error()


def test_more_than_2_32_attached_values_stay_on_the_host():
    class Huge:
        data_size = (1 << 32) + 1

    assert engine.draw_box_randoms(Huge(), 10, 10) is None
