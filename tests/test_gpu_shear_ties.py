"""GPU: the four shear counts on catalogues whose sort keys are tied. ``Catalog.from_healpix_map`` puts one object on every
pixel centre, and pixel centres sit on iso-latitude rings: along the default ``sort_axis = 2`` hundreds of objects of a
segment share one key exactly, where every other scene of the shear suites draws positions from a continuous distribution.
The window of a lane tile is two bisections over the streamed segment's key column and a diagonal cell cuts at ``ta + 1``
(``shear_walk`` in csrc/yawhip_shear.hip); here the runs of equal keys straddle tile and stage boundaries.

Catalogues: the pixel centres of ``yaw.healpix.map_pixels`` over a patch of an nside-512 map -- 9 rings x 400 pixels of a map in
RING order (3 patches of 3 rings: 3 keys per segment), a 64 x 64 block of a map in NESTED order (4 patches of 32 x 32: runs of 1
to 32) -- and 2400 objects at ONE declination (a segment is a single key). ``sort_axis = 0`` is the untied control. Thresholds:
two rows whose outer edge is three ring spacings of the key times (1 -/+ 1e-9), so that the window's boundary lands on a run
of ties, and for the pair count a row of two spacings and a wide one besides. Sums hold the rules of the counts' own suites
against the numpy oracles; unweighted ``W`` is the pair count of the shipped exact kernel, bit for bit.

The count in each lens's own radius (``dsigma_count_radial``) runs on the same catalogues with a column ``m`` of three values a
factor 4 apart mixed inside every run of ties, and squared radii whose last edge puts the reach of the NEAREST lenses at those
three spacings: its window is the only one that does not come from the row's last edge.

The two projected counts (``proj_count``, ``proj_count_pi``) run on the shear catalogues with ``d`` of three values a factor 2
apart mixed inside every run of ties and ``c`` a multiple of 1/4 (``p`` is exact and falls ON pi edges), the reach of the nearest
objects again at three spacings: exact integers against tests/proj_oracle.py and tests/proj_pi_oracle.py."""
import functools

import numpy as np
import pytest

import dsigma_oracle
import dsigma_radial_oracle
import proj_oracle
import proj_pi_oracle
import shear_auto_oracle
import shear_oracle
import shear_pair_oracle
import test_gpu_shear
import test_gpu_shear_auto
from conftest import ARCMIN
from yet_another_wizz_amd import _lib, engine, healpix
from yet_another_wizz_amd.catalog import radec_to_xyz

pytestmark = pytest.mark.gpu
NSIDE = 512
RING_SPACING = 2.0 / (3.0 * NSIDE)  # of z = sin(dec) between neighbouring rings of the equatorial belt: 4.5 arcmin
FIRST_RING, N_RINGS, FIRST_PIXEL, PIXELS_PER_RING = 700, 9, 100, 400
NESTED_BLOCK, NESTED_FIRST = 4096, 276 * 4096  # a 64 x 64 block of base pixel 4, an equatorial one
CATALOGUES = ["ring", "nested", "one declination"]
AXES = [2, 0]


def thresholds(n_rows=2):
    """f64[n_rows, 5]: from 1 arcmin to 3 ring spacings x (1 - 1e-9), to 3 x (1 + 1e-9), to 2 x (1 + 1e-9), to 4.4 spacings
    (pixel centres are 6.9 arcmin apart: one spacing holds no pair)."""
    outer = np.array([3.0 * (1.0 - 1e-9), 3.0 * (1.0 + 1e-9), 2.0 * (1.0 + 1e-9), 4.4])[:n_rows] * RING_SPACING
    return np.array([np.geomspace(np.sin(0.5 * ARCMIN) * 2.0, edge, 5) for edge in outer]) ** 2


@functools.lru_cache(maxsize=None)
def positions(name):
    """``(ra, dec, patch, serial)`` of a catalogue: ``serial`` numbers the objects along their ring (or along the nested curve),
    so that its parity spreads redshift bins evenly over every run of ties."""
    if name == "one declination":
        rng = np.random.default_rng(77)
        ra = np.sort(rng.uniform(0.5, 0.5 + 2.0 * np.pi / 180.0, 2400))
        return ra, np.full(2400, 0.35), (np.arange(2400) >= 1100).astype(np.int64), np.arange(2400)
    values = np.full(12 * NSIDE * NSIDE, healpix.UNSEEN)
    if name == "ring":
        belt = 2 * NSIDE * (NSIDE - 1)  # pixels of the polar cap in front of the first ring of the belt, ring NSIDE
        for ring in range(FIRST_RING, FIRST_RING + N_RINGS):
            start = belt + (ring - NSIDE) * 4 * NSIDE + FIRST_PIXEL
            values[start:start + PIXELS_PER_RING] = 1.0
        ipix, ra, z, _, _ = healpix.map_pixels(values, nested=False)
        ring, serial = (ipix - belt) // (4 * NSIDE) + NSIDE, (ipix - belt) % (4 * NSIDE)
        patch = (ring - FIRST_RING) // 3
    else:
        values[NESTED_FIRST:NESTED_FIRST + NESTED_BLOCK] = 1.0
        ipix, ra, z, _, _ = healpix.map_pixels(values, nested=True)
        serial = ipix - NESTED_FIRST
        patch = serial // (NESTED_BLOCK // 4)
    assert np.all(np.abs(z) < 2.0 / 3.0)  # the equatorial belt: rings RING_SPACING apart
    return ra, np.arcsin(z), patch.astype(np.int64), serial.astype(np.int64)


def segments(columns, patch, bins, n_patches, n_bins):
    """The oracle's dict: the objects ordered by (patch, bin) with the offsets int64[P * n_bins + 1]."""
    seg = patch * n_bins + bins
    order = np.argsort(seg, kind="stable")
    cat = {k: v[order] for k, v in columns.items()}
    cat["off"] = np.concatenate([[0], np.cumsum(np.bincount(seg, minlength=n_patches * n_bins))]).astype(np.int64)
    for a in cat.values():
        a.setflags(write=False)
    return cat


@functools.lru_cache(maxsize=None)
def scene(name):
    """``(lenses, sources, catalogue, n_patches)`` on the positions of ``name``, all unweighted: every object a source (one
    segment per patch), every second one a lens (two bins, with the columns ``f, c``), and all of them a shear catalogue in two
    bins. Along z every segment is a few long runs of equal keys (one run at one declination)."""
    ra, dec, patch, serial = positions(name)
    n, n_patches = len(ra), int(patch.max()) + 1
    rng = np.random.default_rng(len(name))
    x, y, z = radec_to_xyz(ra, dec)
    c = rng.uniform(600.0, 2500.0, n)
    columns = dict(x=x, y=y, z=z, g1=rng.normal(0, 0.3, n), g2=rng.normal(0, 0.3, n), u=1.0 / rng.uniform(600.0, 2500.0, n),
                   f=c / rng.uniform(1.2, 1.9, n), c=c)
    shear = {k: columns[k] for k in ("x", "y", "z", "g1", "g2")}
    src = dict(segments(dict(shear, u=columns["u"]), patch, np.zeros(n, dtype=np.int64), n_patches, 1), w=None)
    cat = dict(segments(shear, patch, serial % 2, n_patches, 2), w=None, nb=2)
    even = serial % 2 == 0
    lens = dict(segments({k: columns[k][even] for k in ("x", "y", "z", "f", "c")}, patch[even], (serial[even] // 2) % 2, n_patches, 2), w=None, nb=2)
    for tied in (src, cat, lens):  # segments longer than a lane tile / a stage, made of runs of equal keys
        sizes = np.diff(tied["off"])
        keys_per_segment = [len(np.unique(tied["z"][a:b])) for a, b in zip(tied["off"][:-1], tied["off"][1:])]
        assert sizes.min() >= 256 and max(keys_per_segment) <= {"ring": 3, "nested": 63, "one declination": 1}[name], (name, sizes, keys_per_segment)
        assert len(np.unique(tied["x"])) == len(tied["x"])  # the control axis is untied
    return lens, src, cat, n_patches


def job_lists(n_patches):
    """Every ordered patch pair for the lens counts, every ``p <= q`` for the auto count, and cells in four rows for the pair
    count: same-bin (diagonal and not) with the rows 0 and 1, cross-bin in both orders with the rows 2 and 3."""
    jobs = np.array([(p, q) for p in range(n_patches) for q in range(n_patches)], dtype=np.int32)
    upper = jobs[jobs[:, 0] <= jobs[:, 1]]
    cells = [(p, q, k, k, k) for p, q in upper for k in (0, 1)] + [(p, q, 0, 1, 2 + (p + q) % 2) for p, q in jobs]
    cells += [(p, q, 1, 0, 3) for p, q in upper] + [(p, p, k, k, 3) for p in range(n_patches) for k in (0, 1)]
    return jobs, upper, np.array(cells, dtype=np.int32)


@functools.lru_cache(maxsize=None)
def expected(name, count):
    """The oracle of a count on a catalogue: once, shared by the sort axes, never modified."""
    lens, src, cat, n_patches = scene(name)
    jobs, upper, cells = job_lists(n_patches)
    out = {"shear": lambda: shear_oracle.shear_jobs(lens, src, jobs, thresholds()),
           "dsigma": lambda: dsigma_oracle.dsigma_jobs(lens, src, jobs, thresholds()),
           "auto": lambda: shear_auto_oracle.shear_auto_jobs(cat, upper, thresholds()),
           "pair": lambda: shear_pair_oracle.shear_pair_cells(cat, cat, cells, thresholds(4))}[count]()
    for a in out:
        a.setflags(write=False)
    return out


def upload_lens_side(ctx, lens, src, sort_axis, kind):
    """``kind``: "shear" (a catalogue handle and plain sources), "dsigma" (a lens handle with f, c; sources with u) or "unit"
    (the same with f = 1, c = 0: W is the pair count)."""
    n_patches = len(src["off"]) - 1
    if kind == "shear":
        return test_gpu_shear.upload(ctx, lens, src, sort_axis)
    f, c = (lens["f"], lens["c"]) if kind == "dsigma" else (np.ones_like(lens["f"]), np.zeros_like(lens["c"]))
    lenses = _lib.DsigmaLenses(ctx, lens["x"], lens["y"], lens["z"], None, f, c, n_patches, 2, lens["off"], sort_axis=sort_axis)
    sources = _lib.ShearSources(ctx, src["x"], src["y"], src["z"], None, src["g1"], src["g2"], n_patches, src["off"], sort_axis=sort_axis, u=src["u"])
    return lenses, sources


def exact_counts(ctx, lens, src, jobs, t, sort_axis):
    """The pair counts of the shipped exact kernel between the lenses and the sources as plain catalogues."""
    n_patches = len(src["off"]) - 1
    one = _lib.DeviceCatalog(ctx, lens["x"], lens["y"], lens["z"], None, n_patches, 2, lens["off"], sort_axis=sort_axis)
    two = _lib.DeviceCatalog(ctx, src["x"], src["y"], src["z"], None, n_patches, 1, src["off"], sort_axis=sort_axis)
    try:
        return _lib.count_pairs(ctx, one, two, jobs, t, kernel="exact")[0].astype(np.float64)
    finally:
        one.free(), two.free()


# --------------------------------------------------------------------------- 1. the two counts around lenses
@pytest.mark.parametrize("sort_axis", AXES)
@pytest.mark.parametrize("count", ["shear", "dsigma"])
@pytest.mark.parametrize("name", CATALOGUES)
def test_lens_counts_on_tied_keys(name, count, sort_axis):
    lens, src, _, n_patches = scene(name)
    jobs, t = job_lists(n_patches)[0], thresholds()
    exp = expected(name, count)
    assert np.count_nonzero(exp[3]) > 4 * n_patches and np.all(exp[3][::n_patches + 1].sum(axis=2) > 0)  # both rows of every diagonal job
    ctx = engine.get_context(0)
    call = _lib.shear_count if count == "shear" else _lib.dsigma_count
    handles = upload_lens_side(ctx, lens, src, sort_axis, count)
    try:
        T, X, W, stats = call(ctx, *handles, jobs, t)
    finally:
        handles[0].free(), handles[1].free()
    assert stats.n_workgroups == len(jobs) * 2 and 0 < stats.evaluated_pairs <= stats.candidate_pairs
    test_gpu_shear.check_against_oracle(f"{count} on {name} axis={sort_axis}", (T, X, W), exp)
    if count == "dsigma":  # unit columns: W counts the pairs
        handles = upload_lens_side(ctx, lens, src, sort_axis, "unit")
        try:
            W = _lib.dsigma_count(ctx, *handles, jobs, t)[2]
        finally:
            handles[0].free(), handles[1].free()
    pairs = exact_counts(ctx, lens, src, jobs, t, sort_axis)
    assert pairs.sum() > 5000 and np.array_equal(W, pairs)


# --------------------------------------------------------------------------- 1b. the count in each lens's own radius
RADIAL_M = 900.0**2 * np.array([1.0, 4.0, 16.0])  # the lenses' column m: three values a factor 4 apart


def radii2():
    """f64[2, 5]: squared radii from 1 arcmin at the nearest lenses to a last edge with ``sqrt(r2max / min_m)`` = 3 ring
    spacings x (1 -/+ 1e-9): the window, whose half width follows the NEAREST lens of the bin (``reach`` in ``run_count``), ends
    on a run of ties; the lenses 2 and 4 times farther stop 1.5 and 0.75 spacings out."""
    outer = np.array([3.0 * (1.0 - 1e-9), 3.0 * (1.0 + 1e-9)]) * RING_SPACING
    return RADIAL_M[0] * np.array([np.geomspace(ARCMIN, edge, 5) for edge in outer]) ** 2


@functools.lru_cache(maxsize=None)
def radial_scene(name):
    """The lenses and sources of ``scene(name)`` with ``m`` cycling through RADIAL_M along ``serial``, so that every run of
    ties mixes the three."""
    lens, src, _, n_patches = scene(name)
    ra, dec, patch, serial = positions(name)
    even = serial % 2 == 0
    order = np.argsort(patch[even] * 2 + (serial[even] // 2) % 2, kind="stable")  # the order of ``segments``
    assert np.array_equal(radec_to_xyz(ra, dec)[0][even][order], lens["x"])
    m = RADIAL_M[(serial[even] // 2) % 3][order]
    m.setflags(write=False)
    for a, b in zip(lens["off"][:-1], lens["off"][1:]):
        keys, run = np.unique(lens["z"][a:b], return_inverse=True)
        long_runs = [r for r in range(len(keys)) if np.count_nonzero(run == r) >= 12]
        assert long_runs and all(len(np.unique(m[a:b][run == r])) == 3 for r in long_runs), name
        assert m[a:b].min() == RADIAL_M[0]  # the nearest kind of lens in every segment: both bins reach 3 spacings
    return dict(lens, m=m), src, n_patches


@functools.lru_cache(maxsize=None)
def radial_expected(name, columns):
    """The mirror oracle of the radial count on a catalogue (``columns`` "real" or "unit": ``f = 1``, ``c = 0``): once, shared
    by the sort axes, never modified."""
    lens, src, n_patches = radial_scene(name)
    if columns == "unit":
        lens = dict(lens, f=np.ones_like(lens["f"]), c=np.zeros_like(lens["c"]))
    out = dsigma_radial_oracle.radial_jobs(lens, src, job_lists(n_patches)[0], radii2())
    for a in out:
        a.setflags(write=False)
    return out


@pytest.mark.parametrize("sort_axis", AXES)
@pytest.mark.parametrize("name", CATALOGUES)
def test_radial_count_on_tied_keys(name, sort_axis):
    lens, src, n_patches = radial_scene(name)
    jobs, r2 = job_lists(n_patches)[0], radii2()
    exp, exp_unit = radial_expected(name, "real"), radial_expected(name, "unit")
    assert np.count_nonzero(exp[3]) > 4 * n_patches and np.all(exp[3][::n_patches + 1].sum(axis=2) > 0)  # both rows of every diagonal job
    # what the nearest lenses alone hold: without them the counts fall (on pixel centres, 6.9 arcmin apart, to nothing: the
    # farther lenses reach 6.75 arcmin -- any pair counted around them is a pair binned with a neighbour's m)
    far_only = dsigma_radial_oracle.radial_jobs(dict(lens, f=np.ones_like(lens["f"]), c=np.zeros_like(lens["c"]),
                                                     m=np.where(lens["m"] == RADIAL_M[0], 1e12, lens["m"])), src, jobs[:1], r2)[2]
    assert far_only.sum() < exp_unit[2][:1].sum() and (far_only.sum() > 0) == (name == "one declination")
    ctx = engine.get_context(0)
    n = len(src["off"]) - 1
    results = {}
    for columns in ("real", "unit"):
        f, c = (lens["f"], lens["c"]) if columns == "real" else (np.ones_like(lens["f"]), np.zeros_like(lens["c"]))
        lenses = _lib.DsigmaLenses(ctx, lens["x"], lens["y"], lens["z"], None, f, c, n, 2, lens["off"], sort_axis=sort_axis, m=lens["m"])
        sources = _lib.ShearSources(ctx, src["x"], src["y"], src["z"], None, src["g1"], src["g2"], n, src["off"], sort_axis=sort_axis, u=src["u"])
        try:
            results[columns] = _lib.dsigma_count_radial(ctx, lenses, sources, jobs, r2)
        finally:
            lenses.free(), sources.free()
    T, X, W, stats = results["real"]
    assert stats.n_workgroups == len(jobs) * 2 and 0 < stats.evaluated_pairs <= stats.candidate_pairs
    test_gpu_shear.check_against_oracle(f"radial on {name} axis={sort_axis}", (T, X, W), exp[:4])
    W = results["unit"][2]
    assert exp_unit[2].sum() >= 2000 and np.all(exp_unit[2] == np.rint(exp_unit[2])) and np.array_equal(W, exp_unit[2])


# --------------------------------------------------------------------------- 2. the two shear-shear counts
@pytest.mark.parametrize("sort_axis", AXES)
@pytest.mark.parametrize("name", CATALOGUES)
def test_auto_count_on_tied_keys(name, sort_axis):
    _, _, cat, n_patches = scene(name)
    upper, t = job_lists(n_patches)[1], thresholds()
    exp = expected(name, "auto")
    diagonal = upper[:, 0] == upper[:, 1]
    assert np.all(exp[3][diagonal].sum(axis=2) > 0)
    P, M, C, W, stats = test_gpu_shear_auto.count(cat, upper, t, sort_axis)
    assert stats.n_workgroups == len(upper) * 2 and stats.evaluated_pairs > 0
    test_gpu_shear_auto.check_against_oracle(f"auto on {name} axis={sort_axis}", (P, M, C, W), exp)
    pairs = test_gpu_shear_auto.exact_pair_count(cat, upper, t, sort_axis)
    assert pairs.sum() > 3000 and np.array_equal(W, pairs)


@pytest.mark.parametrize("sort_axis", AXES)
@pytest.mark.parametrize("name", CATALOGUES)
def test_pair_count_on_tied_keys(name, sort_axis):
    """Against the oracle, whose unweighted ``W`` is a pair count in the float64 predicate of every kernel: equal bit for bit;
    the same-bin cells of the rows 0 and 1 are the auto count's bits."""
    _, _, cat, n_patches = scene(name)
    _, upper, cells = job_lists(n_patches)
    exp = expected(name, "pair")
    live = exp[3].sum(axis=1) > 0
    assert all(np.any(live & (cells[:, 4] == row)) for row in range(4)) and np.any(live & (cells[:, 2] != cells[:, 3]) & (cells[:, 0] > cells[:, 1]))
    ctx = engine.get_context(0)
    handle = test_gpu_shear_auto.upload(ctx, cat, sort_axis)
    try:
        P, M, C, W, stats = _lib.shear_pair_count(ctx, handle, handle, cells, thresholds(4))
        auto = _lib.shear_auto_count(ctx, handle, upper, thresholds())
    finally:
        handle.free()
    assert stats.n_workgroups == len(cells) and stats.evaluated_pairs > 0
    test_gpu_shear_auto.check_against_oracle(f"pair on {name} axis={sort_axis}", (P, M, C, W), exp)
    assert exp[3].sum() > 5000 and np.array_equal(W, exp[3])
    for ours, ref in zip((P, M, C, W), auto[:4]):
        assert np.array_equal(ours[:2 * len(upper)].reshape(ref.shape), ref)


# --------------------------------------------------------------------------- 2b. the two projected counts
PROJ_D = 900.0 * np.array([1.0, 2.0, 4.0])  # the column d: three values a factor 2 apart
PROJ_PMAX = 40.0
PROJ_PI = np.linspace(0.0, PROJ_PMAX, 5)  # c is a multiple of 1/4: pairs fall ON the edges 10, 20, 30 and 40


def proj_radii2():
    """f64[2, 5]: squared radii from 1 arcmin at the nearest pairs to a last edge with ``sqrt(r2max) / min d`` = 3 ring spacings
    x (1 -/+ 1e-9): the window, whose half width follows the least ``d`` of the bins a row pairs, ends on a run of ties."""
    outer = np.array([3.0 * (1.0 - 1e-9), 3.0 * (1.0 + 1e-9)]) * RING_SPACING
    return (PROJ_D[0] * np.array([np.geomspace(ARCMIN, edge, 5) for edge in outer])) ** 2


def proj_columns(n):
    """``(d, c)`` by index: ``d`` cycles through PROJ_D, a step further after every third object (rings that alternate with a
    period of 3 inside a segment mix them too), ``c`` through the multiples of 1/4 below 120 in strides of a prime."""
    index = np.arange(n)
    return PROJ_D[(index + index // 3) % 3], ((index * 7919) % 480) * 0.25


@functools.lru_cache(maxsize=None)
def proj_scene(name):
    """The shear catalogue of ``scene(name)`` as a projected handle of unit weight, and its cells: same-bin (diagonal and
    ``p < q``) with the row of the bin, cross-bin in both orders with alternating rows."""
    _, _, cat, n_patches = scene(name)
    d, c = proj_columns(len(cat["x"]))
    h = dict(x=cat["x"], y=cat["y"], z=cat["z"], w=None, d=d, c=c, nb=2, off=cat["off"])
    for a, b in zip(h["off"][:-1], h["off"][1:]):
        keys, run = np.unique(h["z"][a:b], return_inverse=True)
        long_runs = [r for r in range(len(keys)) if np.count_nonzero(run == r) >= 12]
        assert long_runs and all(len(np.unique(d[a:b][run == r])) == 3 for r in long_runs), name  # every run of ties mixes the three
    jobs, upper, _ = job_lists(n_patches)
    cells = [(p * 2 + k, q * 2 + k, k, p == q) for p, q in upper for k in (0, 1)] + [(p * 2, q * 2 + 1, (p + q) % 2, 0) for p, q in jobs]
    cells = np.array(cells, dtype=np.int32)
    out = (proj_oracle.proj_cells(h, h, cells, proj_radii2(), PROJ_PMAX)[2], proj_pi_oracle.proj_pi_cells(h, h, cells, proj_radii2(), PROJ_PI)[2])
    for a in (d, c, cells) + out:
        a.setflags(write=False)
    return h, cells, out


@pytest.mark.parametrize("sort_axis", AXES)
@pytest.mark.parametrize("name", CATALOGUES)
def test_projected_counts_on_tied_keys(name, sort_axis):
    """The single cylinder and four pi planes, as exact integers; the planes sum to the cylinder."""
    import test_gpu_projected

    h, cells, (exp, exp_pi) = proj_scene(name)
    r2 = proj_radii2()
    live = exp.sum(axis=1) > 0
    # (pixel centres are 6.9 arcmin apart and only pairs of the two nearer kinds reach that far: a thousand pairs, not more)
    assert exp.sum() > 1000 and np.any(live[cells[:, 3] != 0]) and np.any(live & (cells[:, 0] % 2 != cells[:, 1] % 2))
    assert np.all(exp_pi.sum(axis=(1, 2)) > 0) and np.array_equal(exp_pi.sum(axis=0), exp)
    # what the nearest objects hold: with every d = 900 sent far away the counts fall
    far_only = proj_oracle.proj_cells(dict(h, d=np.where(h["d"] == PROJ_D[0], 1e9, h["d"])), h, cells[:1], r2, PROJ_PMAX, same=True)[2]
    assert far_only.sum() < exp[:1].sum()
    on_an_edge = np.abs(h["c"][:300, None] - h["c"][None, :300])
    assert np.any(on_an_edge == 10.0) and np.any(on_an_edge == PROJ_PMAX)
    ctx = engine.get_context(0)
    handle = test_gpu_projected.upload(ctx, h, sort_axis)
    try:
        W, stats = _lib.proj_count(ctx, handle, handle, cells, r2, PROJ_PMAX)
        W_pi, stats_pi = _lib.proj_count_pi(ctx, handle, handle, cells, r2, PROJ_PI)
    finally:
        handle.free()
    for st in (stats, stats_pi):
        assert st.n_workgroups == len(cells) and 0 < st.evaluated_pairs <= st.candidate_pairs
    assert np.array_equal(W, exp), (name, sort_axis, np.abs(W - exp).sum())
    assert np.array_equal(W_pi, exp_pi), (name, sort_axis, np.abs(W_pi - exp_pi).sum())


# --------------------------------------------------------------------------- 3. the diagonal on tied keys
@pytest.mark.parametrize("name", ["ring", "one declination"])
def test_diagonal_cells_hold_every_unordered_pair_once(name):
    """The sources of patch 0 (1200 objects in 3 runs of equal keys; at one declination 1100 in a single run) as one segment:
    the diagonal cell against the oracle's unordered sum and the exact kernel's halved count; then cut into two patches inside a
    run: the three cells together hold every pair of the whole once."""
    _, src, _, _ = scene(name)
    n, cut = int(src["off"][1]), 470
    by_key = np.argsort(src["z"][:n], kind="stable")  # (the upload sorts anyway: this only shows where the cut falls)
    columns = {k: src[k][:n][by_key] for k in ("x", "y", "z", "g1", "g2")}
    assert len(np.unique(columns["z"])) == (3 if name == "ring" else 1) and columns["z"][cut - 1] == columns["z"][cut]
    t = thresholds()[1:]
    whole = dict(columns, w=None, nb=1, off=np.array([0, n], dtype=np.int64))
    split = dict(whole, off=np.array([0, cut, n], dtype=np.int64))
    jobs = np.array([(0, 0), (1, 1), (0, 1)], dtype=np.int32)
    got_whole = test_gpu_shear_auto.count(whole, [[0, 0]], t)[:4]
    test_gpu_shear_auto.check_against_oracle(f"diagonal on {name}", got_whole, shear_auto_oracle.shear_auto_jobs(whole, [[0, 0]], t))
    got_split = test_gpu_shear_auto.count(split, jobs, t)[:4]
    exp_split = shear_auto_oracle.shear_auto_jobs(split, jobs, t)
    assert exp_split[3][2].sum() > 100  # pairs across the cut
    test_gpu_shear_auto.check_against_oracle(f"split on {name}", got_split, exp_split)
    assert got_whole[3].sum() > 2000 and np.array_equal(got_whole[3][0], got_split[3].sum(axis=0))
    assert np.array_equal(got_whole[3], test_gpu_shear_auto.exact_pair_count(whole, [[0, 0]], t))
    # the projected count: the diagonal cell is the oracle's, and half the segment against a bit-identical copy uploaded as a
    # second handle (that one sees every pair twice, and every object with itself at R2 = 0, which no bin holds)
    import test_gpu_projected

    d, c = proj_columns(n)
    proj = dict({k: columns[k] for k in "xyz"}, w=None, d=d, c=c, nb=1, off=np.array([0, n], dtype=np.int64))
    copy = {key: (value.copy() if isinstance(value, np.ndarray) else value) for key, value in proj.items()}
    r2 = proj_radii2()[1:]
    assert r2[0, 0] > 0.0
    once, _ = test_gpu_projected.count(proj, proj, test_gpu_projected.DIAGONAL, r2, PROJ_PMAX)
    both, stats = test_gpu_projected.count(proj, copy, test_gpu_projected.ACROSS, r2, PROJ_PMAX)
    assert stats.candidate_pairs == n * n and once.sum() > 300 and np.array_equal(both, 2.0 * once)
    assert np.array_equal(once, proj_oracle.proj_cells(proj, proj, test_gpu_projected.DIAGONAL, r2, PROJ_PMAX)[2])
