"""HealPixRandoms on the host route (plain numpy, no healpy) against HEALPix' published geometry by formulas written here,
independent of the package's nested arithmetic: the base-pixel centres, the ring scheme's closed form (Gorski et al. 2005,
eqs. 2-9) and an ang2pix at the mask's own order. The reference draws its mask pixels from numpy's global RNG, so there is
no reference stream to compare with: the stream checked here is the one HealPixRandoms' docstring defines. No GPU."""
import ctypes
import math

import numpy as np
import pytest

import yet_another_wizz_amd as yaw
from yet_another_wizz_amd import _lib, engine
from yet_another_wizz_amd.randoms import HealPixRandoms, nest2ring, pix2loc_nest

PI = np.pi


@pytest.fixture
def host_only(monkeypatch):
    monkeypatch.setattr(engine, "draw_healpix_randoms", lambda *args, **kwargs: None)


# ---- independent HEALPix formulas ----
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
    s = (i - nside + 1) % 2  # 1: the ring's first centre is half a pixel from phi = 0; 0: it is at phi = 0, as the HEALPix
    # library numbers it (eq. 9 taken literally, j - s / 2, counts the same centres of such a ring from pi / 2 nside to 2 pi)
    return PI / (2 * nside) * (j - 1 + s / 2.0), 4.0 / 3.0 - 2.0 * i / (3.0 * nside)


def spread_bits(v):
    out = np.zeros_like(v)
    for b in range(14):
        out |= ((v >> b) & 1) << (2 * b)
    return out


def ang2pix_nest(order, phi, z):
    """Nested pixel of ``order`` that holds the points (phi, z = sin dec): HEALPix' ang2pix (paper section 4.1 / appendix)."""
    nside = 1 << order
    za = np.abs(z)
    tt = np.mod(phi, 2 * PI) / (PI / 2)
    # equatorial region
    t1, t2 = nside * (0.5 + tt), nside * z * 0.75
    jp, jm = np.floor(t1 - t2).astype(np.int64), np.floor(t1 + t2).astype(np.int64)
    ifp, ifm = jp >> order, jm >> order
    face_e = np.where(ifp == ifm, ifp | 4, np.where(ifp < ifm, ifp, ifm + 8))
    ix_e, iy_e = jm & (nside - 1), nside - (jp & (nside - 1)) - 1
    # polar caps
    ntt = np.minimum(tt.astype(np.int64), 3)
    tp = tt - ntt
    tmp = nside * np.sqrt(3.0 * (1.0 - za))
    jp_c = np.minimum((tp * tmp).astype(np.int64), nside - 1)
    jm_c = np.minimum(((1.0 - tp) * tmp).astype(np.int64), nside - 1)
    north = z >= 0
    face_c = np.where(north, ntt, ntt + 8)
    ix_c, iy_c = np.where(north, nside - jm_c - 1, jp_c), np.where(north, nside - jp_c - 1, jm_c)
    belt = za <= 2.0 / 3.0
    face, ix, iy = np.where(belt, face_e, face_c), np.where(belt, ix_e, ix_c), np.where(belt, iy_e, iy_c)
    return face * nside * nside + spread_bits(ix) + 2 * spread_bits(iy)


# ---- geometry ----
def test_base_pixel_centres():
    phi, z = pix2loc_nest(0, np.arange(12))
    expect_z = np.repeat([2.0 / 3.0, 0.0, -2.0 / 3.0], 4)
    assert np.all(np.abs(z - expect_z) <= np.spacing(np.abs(expect_z)))
    quarters = np.array([1, 3, 5, 7, 0, 2, 4, 6, 1, 3, 5, 7])
    assert np.array_equal(phi, quarters * PI / 4)


@pytest.mark.parametrize("order", range(6))
def test_ring_formula_and_bijection(order):
    nside, npix = 1 << order, 12 << (2 * order)
    ring = nest2ring(order, np.arange(npix))
    assert ring.dtype == np.int64 and np.array_equal(np.sort(ring), np.arange(npix))
    phi, z = pix2loc_nest(order, np.arange(npix))
    expect = np.array([ring_pix2ang(nside, int(p)) for p in ring])
    # two formulas for one real number, a handful of roundings each
    assert np.all(np.abs(phi - expect[:, 0]) <= 4 * np.spacing(np.abs(expect[:, 0])))
    assert np.all(np.abs(z - expect[:, 1]) <= 4 * np.spacing(1.0))
    by_ring = np.argsort(ring)  # ring order: z never increases, phi increases inside a ring
    dz, dphi = np.diff(z[by_ring]), np.diff(phi[by_ring])
    assert np.all(dz <= 0) and np.all(dphi[dz == 0] > 0)


def masks(nside):
    """name -> nested map. Caps and belt split at |z| = 0.6 of the pixel centre, so that nside 1 has both (its polar base
    pixels sit at |z| = 2/3); the face-edge mask is the pixels along both ix = 0 and iy = 0 edges of faces 0, 5 and 10."""
    order = nside.bit_length() - 1
    npix = 12 * nside * nside
    _, z = pix2loc_nest(order, np.arange(npix))
    in_face = np.arange(npix) % (nside * nside)
    edge = ((in_face & 0x5555555) == 0) | ((in_face & 0xAAAAAAA) == 0)
    single = np.zeros(npix)
    single[(7 * npix) // 11] = 2.5
    return {
        "full": np.ones(npix),
        "caps": (np.abs(z) > 0.6).astype(float),
        "belt": (np.abs(z) <= 0.6).astype(float),
        "single": single,
        "edge": (edge & np.isin(np.arange(npix) // (nside * nside), (0, 5, 10))).astype(float),
    }


@pytest.mark.parametrize("nside", [1, 2, 8, 64])
@pytest.mark.parametrize("name", ["full", "caps", "belt", "single", "edge"])
def test_round_trip_into_the_drawn_pixel(nside, name):
    order = nside.bit_length() - 1
    gen = HealPixRandoms(masks(nside)[name], nested=True, is_mask=True, seed=nside + len(name))
    n = 20_000
    drawn = gen._draw_pixels(n) >> (2 * (29 - order))
    gen.reseed()
    chunk = gen(n)
    assert sorted(chunk) == ["dec", "ra"] and chunk["ra"].dtype == chunk["dec"].dtype == np.float64
    assert np.all((chunk["ra"] >= 0) & (chunk["ra"] < 2 * PI)) and np.all(np.abs(chunk["dec"]) <= PI / 2)
    back = ang2pix_nest(order, chunk["ra"], np.sin(chunk["dec"]))
    assert np.array_equal(back, drawn)
    assert np.all(np.isin(drawn, gen._ipix_unmasked))
    if name != "single" and len(gen._ipix_unmasked) <= 200:
        assert set(drawn) == set(gen._ipix_unmasked)  # every unmasked pixel is reached


@pytest.mark.parametrize("nside", [1, 4, 32])
def test_ring_map_and_its_nested_reordering_draw_alike(nside):
    order = nside.bit_length() - 1
    npix = 12 * nside * nside
    ring_map = np.random.default_rng(nside).uniform(0.0, 1.0, npix) * (np.arange(npix) % 3 != 0)
    nested_map = ring_map[nest2ring(order, np.arange(npix))]
    a = HealPixRandoms(ring_map, seed=4)
    b = HealPixRandoms(nested_map, nested=True, seed=4)
    assert a.nside == b.nside == nside
    assert np.array_equal(a._ipix_unmasked, b._ipix_unmasked) and np.array_equal(a._cdf, b._cdf)
    ca, cb = a(5000), b(5000)
    assert np.array_equal(ca["ra"], cb["ra"]) and np.array_equal(ca["dec"], cb["dec"])


# ---- stream ----
def test_stream_is_the_documented_one():
    values = np.array([0, 3, 0, 1, 1, 0, 2, 0, 0, 5, 0, 0] * 4, dtype=float)  # nside 2, nested
    data = np.linspace(1.0, 2.0, 11)
    gen = HealPixRandoms(values, nested=True, weights=data, seed=77)
    k = 1000
    raw = np.random.default_rng(np.random.SeedSequence(77).spawn(1)[0])
    first, second = raw.bit_generator.random_raw(k), raw.bit_generator.random_raw(k)
    idx = raw.integers(0, 11, size=k)
    unmasked = np.flatnonzero(values)
    cdf = np.cumsum(values[unmasked]) / values[unmasked].sum()
    u = (first >> np.uint64(11)).astype(np.float64) / 2.0**53
    slot = np.array([np.count_nonzero(cdf <= v) for v in u])
    sub = (second >> np.uint64(64 - 56)).astype(np.int64)  # 2 (29 - 1) = 56 bits
    assert sub.max() < 4**28 and np.array_equal(gen._cdf, cdf)
    pix = unmasked[slot] * 4**28 + sub
    assert np.array_equal(gen._draw_pixels(k), pix)
    gen.reseed()
    chunk = gen(k)
    phi, z = pix2loc_nest(29, pix)
    assert np.array_equal(chunk["ra"], phi) and np.array_equal(chunk["dec"], np.arcsin(z))
    assert np.array_equal(chunk["weights"], data[idx])
    assert gen.rng.bit_generator.state == raw.bit_generator.state
    # one seed, one stream; another seed, another; reseed() restarts
    twin = HealPixRandoms(values, nested=True, weights=data, seed=77)(k)
    assert all(np.array_equal(twin[c], chunk[c]) for c in chunk)
    other = HealPixRandoms(values, nested=True, weights=data, seed=78)(k)
    assert not np.array_equal(other["ra"], chunk["ra"]) and not np.array_equal(other["weights"], chunk["weights"])
    assert not np.array_equal(gen(k)["ra"], chunk["ra"])
    gen.reseed()
    again = gen(k)
    assert all(np.array_equal(again[c], chunk[c]) for c in chunk)
    gen.reseed(78)
    assert gen.seed == 78 and np.array_equal(gen(k)["ra"], other["ra"])


def test_random_raw_leaves_a_pending_half_alone():
    gen = HealPixRandoms(np.ones(12), weights=np.arange(7.0), seed=5)
    gen.rng.integers(0, 5, size=1)
    before = gen.rng.bit_generator.state
    assert before["has_uint32"] == 1
    gen._draw_pixels(10)
    after = gen.rng.bit_generator.state
    assert (after["has_uint32"], after["uinteger"]) == (1, before["uinteger"])


def test_density_follows_the_probability_map():
    """Counts per pixel of 2e5 draws from a 3:1 map of nside 2 (36 unmasked pixels) within 5 sigma of the binomial
    expectation in every pixel. Deterministic: one seed."""
    npix = 48
    values = np.where(np.arange(npix) % 2 == 0, 3.0, 1.0) * (np.arange(npix) % 4 != 3)
    gen = HealPixRandoms(values, nested=True, seed=2024)
    n = 200_000
    counts = np.bincount(gen._draw_pixels(n) >> 56, minlength=npix)
    p = values / values.sum()
    assert counts.sum() == n and np.all(counts[values == 0] == 0)
    sigma = np.sqrt(n * p * (1 - p))
    assert np.all(np.abs(counts - n * p) <= 5 * sigma)
    flat = HealPixRandoms(values, nested=True, is_mask=True, seed=2024)
    counts = np.bincount(flat._draw_pixels(n) >> 56, minlength=npix)
    q = (values > 0) / np.count_nonzero(values)
    assert np.all(np.abs(counts - n * q) <= 5 * np.sqrt(n * q * (1 - q)))


# ---- interface ----
def test_constructor_errors():
    for length in (0, 11, 13, 47):
        with pytest.raises(ValueError, match="no HEALPix map"):
            HealPixRandoms(np.ones(length))
    with pytest.raises(ValueError, match="power of two"):
        HealPixRandoms(np.ones(12 * 3 * 3))
    bad = np.ones(48)
    bad[5] = -0.1
    with pytest.raises(ValueError, match="positive"):
        HealPixRandoms(bad)
    with pytest.raises(ValueError, match="masked"):
        HealPixRandoms(np.zeros(48))
    with pytest.raises(ValueError, match="order 13"):
        HealPixRandoms(np.broadcast_to(1.0, (12 * 4**14,)))  # a view: no 25 GB are allocated
    with pytest.raises(ValueError, match="does not match"):
        HealPixRandoms(np.ones(12), weights=np.ones(5), redshifts=np.ones(6))


def test_attributes_repr_and_dataframe():
    z = np.linspace(0.1, 1.0, 9)
    gen = HealPixRandoms(np.ones(192), redshifts=z, seed=11)
    assert (gen.nside, gen.order, gen.seed, gen.data_size) == (4, 2, 11, 9)
    assert gen.has_redshifts and not gen.has_weights and gen.weights is None
    assert repr(gen) == "HealPixRandoms(has_weights=False, has_redshifts=True)"
    assert HealPixRandoms(np.ones(12)).data_size == -1
    df = gen.generate_dataframe(300)
    assert list(df.columns) == ["ra", "dec", "redshifts"]
    assert df["ra"].between(0.0, 360.0).all() and df["dec"].between(-90.0, 90.0).all() and df["redshifts"].isin(z).all()
    gen.reseed()
    rad = gen.generate_dataframe(300, degrees=False)
    assert np.array_equal(df["ra"].to_numpy(), np.rad2deg(rad["ra"].to_numpy()))


def test_from_random_host_route_is_the_generators_chunked_calls(host_only):
    values = masks(8)["belt"] * np.linspace(1.0, 2.0, 768)
    data = np.random.default_rng(3).uniform(0.1, 1.0, (2, 77))
    gen = HealPixRandoms(values, nested=True, weights=data[0], redshifts=data[1], seed=9)
    gen(17)  # from_random reseeds: what was drawn before does not matter
    cat = yaw.Catalog.from_random(None, gen, 1000, patch_centers=yaw.AngularCoordinates([[0.5, 0.0]]), chunksize=333)
    assert cat._random_route == "host" and cat.has_weights and cat.has_redshifts and cat.num_patches == 1
    end = gen.rng.bit_generator.state
    gen.reseed()
    draws = [gen(k) for k in (333, 333, 333, 1)]
    assert gen.rng.bit_generator.state == end
    patch = cat[0]
    for got, name in ((patch.coords.ra, "ra"), (patch.coords.dec, "dec"), (patch.weights, "weights"), (patch.redshifts, "redshifts")):
        assert np.array_equal(got, np.concatenate([d[name] for d in draws])), name


def test_random_healpix_symbol_loads_and_checks_its_arguments():
    lib = _lib.load_library()
    assert "yawhip_random_healpix" in _lib.ABI_SYMBOLS and hasattr(ctypes.CDLL(_lib.LIB_PATH), "yawhip_random_healpix")
    state = (ctypes.c_uint64 * 4)(0, 0, 0, 1)
    out = (ctypes.c_uint64 * 2)()
    ipix, cdf = np.zeros(1, dtype=np.int64), np.ones(1)
    rc = lib.yawhip_random_healpix(None, 10, 10, state, 0, 0, 0, 1, ipix.ctypes.data_as(ctypes.POINTER(ctypes.c_int64)),
                                   cdf.ctypes.data_as(ctypes.POINTER(ctypes.c_double)), -1, None, None, None, None, None, None, None,
                                   None, out, ctypes.byref(ctypes.c_int32()), ctypes.byref(ctypes.c_uint32()))
    assert rc == -1 and b"NULL" in lib.yawhip_last_error()


def test_more_than_2_32_attached_values_stay_on_the_host():
    class Huge:
        data_size = (1 << 32) + 1

    assert engine.draw_healpix_randoms(Huge(), 10, 10) is None
