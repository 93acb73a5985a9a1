"""GPU: the four shear entry points (``shear_count``, ``dsigma_count``, ``shear_auto_count``, ``shear_pair_count``) on job lists
of the size a measurement sends -- 150 patches, two redshift bins, every patch pair in one call -- against the numpy oracles
with the rules of their own suites (``1e-10 * A``, ``RTOL_W``, exact zeros): the question here is the bookkeeping of
``run_count`` and of the policies' ``cell()``, not the arithmetic. What only runs at this scale: result blocks
``[planes][n_cells][E-1]`` of tens of thousands of cells with the evaluated counters behind them, most cells without a single
object; the grow-only call buffers of a handle through calls of other sizes; ``nb == 1`` lenses folded under many rows of
thresholds; handles without any object.

The count in each lens's own radius (``dsigma_count_radial``, ``"radial"``) runs through the same cases on the same scene with
``m = f * f`` and squared radii made from the rows of ``thresholds`` at the median ``m``, against tests/dsigma_radial_oracle.py;
besides, a redshift bin without any lens (``min_m = +inf``) under a last edge of 1e30.

The two projected counts (``proj_count`` on one handle, ``"proj"``, and on two, ``"proj2"``; ``proj_count_pi`` on one handle,
``"proj_pi"``: the branch of ``run_count`` on which the pi edges travel between the half widths and the cell table and ``n_pi``
planes leave in one copy) run through the same cases on the positions of the two shear catalogues, with ``d`` taken from the
lenses' ``f`` and a line-of-sight column ``c``, unit weights, and the cells of the pair count: against tests/proj_oracle.py and
tests/proj_pi_oracle.py as exact integers. On one pair of handles the two entry points also alternate."""
import functools

import numpy as np
import pytest

import dsigma_oracle
import dsigma_radial_oracle
import proj_exact
import proj_oracle
import proj_pi_oracle
import shear_auto_oracle
import shear_oracle
import shear_pair_oracle
import test_gpu_shear
import test_gpu_shear_auto
from conftest import ARCMIN
from yet_another_wizz_amd import _lib, engine
from yet_another_wizz_amd.catalog import radec_to_xyz

pytestmark = pytest.mark.gpu
P, NB, GRID_X, GRID_Y = 150, 2, 15, 10
BOX_DEG = 2.0
PROJ = ("proj", "proj2", "proj_pi")
PROJ_PMAX = 100.0  # against c of 0 .. 300
SMALL = np.array([(16, 16), (16, 17), (17, 16), (31, 16), (32, 32), (0, 149)], dtype=np.int32)  # six jobs for the empty handles


def freeze(arrays):
    for a in arrays:
        if isinstance(a, np.ndarray):
            a.setflags(write=False)
    return arrays


def chord2(arcmin):
    return (2.0 * np.sin(0.5 * np.asarray(arcmin, dtype=np.float64) * ARCMIN)) ** 2


def thresholds(n_rows=NB):
    """f64[n_rows, 5]: 0.5 to 15 arcmin and other limits in every row; a patch is 8 x 12 arcmin, so neighbouring patches pair."""
    return chord2([np.geomspace(0.5 * (1.0 + 0.1 * k), 15.0 * (1.0 - 0.04 * k), 5) for k in range(n_rows)])


def radii2(m, n_rows=NB):
    """The rows of ``thresholds`` as squared radii of the radial count: ``median(m) theta^2`` with the angle of each chord, so that
    around the median lens the bins are the same; neighbouring patches pair."""
    return np.median(m) * (2.0 * np.arcsin(0.5 * np.sqrt(thresholds(n_rows)))) ** 2


def draw_positions(rng, n_bins):
    """0 to 3 objects in every patch (a cell of the 15 x 10 grid over the 2-degree box), none in the first and the last, each in
    any of ``n_bins`` redshift bins -> (ra, dec) ordered by (patch, bin) and the offsets int64[P * n_bins + 1]."""
    sizes = rng.integers(0, 4, P)
    sizes[[0, P - 1]] = 0
    patch = np.repeat(np.arange(P), sizes)
    bins = rng.integers(0, n_bins, len(patch))
    order = np.argsort(patch * n_bins + bins, kind="stable")
    patch, bins = patch[order], bins[order]
    ra = (100.0 + (patch % GRID_X + rng.uniform(0.0, 1.0, len(patch))) * BOX_DEG / GRID_X) * np.pi / 180.0
    dec = (30.0 + (patch // GRID_X + rng.uniform(0.0, 1.0, len(patch))) * BOX_DEG / GRID_Y) * np.pi / 180.0
    off = np.concatenate([[0], np.cumsum(np.bincount(patch * n_bins + bins, minlength=P * n_bins))]).astype(np.int64)
    return ra, dec, off


def shear_catalogue(rng, n_bins):
    ra, dec, off = draw_positions(rng, n_bins)
    x, y, z = radec_to_xyz(ra, dec)
    n = len(x)
    return dict(x=x, y=y, z=z, w=rng.uniform(0.5, 2.0, n), g1=rng.normal(0, 0.3, n), g2=rng.normal(0, 0.3, n), nb=n_bins, off=off)


@functools.lru_cache(maxsize=None)
def scene():
    """``(lenses, sources, catalogue, second catalogue)``: lenses in two bins with the columns ``f, c``, unbinned sources with
    ``u`` (about half the pairs have the source in front), and two shear catalogues in two bins on the same patches."""
    rng = np.random.default_rng(20261)
    ra, dec, off = draw_positions(rng, NB)
    x, y, z = radec_to_xyz(ra, dec)
    c = rng.uniform(600.0, 2500.0, len(x))
    lens = dict(x=x, y=y, z=z, w=rng.uniform(0.5, 2.0, len(x)), f=c / rng.uniform(1.2, 1.9, len(x)), c=c, nb=NB, off=off)
    src = shear_catalogue(rng, 1)
    src = dict({k: v for k, v in src.items() if k != "nb"}, u=1.0 / rng.uniform(600.0, 2500.0, len(src["x"])))
    cats = (lens, src, shear_catalogue(rng, NB), shear_catalogue(rng, NB))
    for cat in cats:
        assert cat["off"][1] == 0 and cat["off"][-2] == cat["off"][-1] and len(cat["x"]) > 150  # first and last patch empty
        freeze(cat.values())
    return cats


@functools.lru_cache(maxsize=None)
def proj_scene():
    """The two shear catalogues as projected handles of unit weight: ``d`` from the lenses' ``f`` (315 .. 2080, repeated to the
    length), ``c`` 0 .. 300; and the pi edges, the uneven set of tests/golden/proj_exact.npz scaled to ``PROJ_PMAX``."""
    lens, _, cat, cat_b = scene()
    rng = np.random.default_rng(20262)
    out = []
    for h, shift in ((cat, 0), (cat_b, 7)):
        n = len(h["x"])
        out.append(freeze_dict(dict(x=h["x"], y=h["y"], z=h["z"], w=None, d=np.roll(np.resize(lens["f"], n), shift), c=rng.uniform(0.0, 300.0, n),
                                    nb=NB, off=h["off"])))
    fx = proj_exact.fixture()
    pe = fx["pi.uneven"] * (PROJ_PMAX / float(fx["pmax"]))
    assert len(pe) >= 9 and pe[0] == 0.0 and pe[-1] == PROJ_PMAX
    return out[0], out[1], freeze([pe])[0]


def freeze_dict(cat):
    freeze(cat.values())
    return cat


def proj_cells(one_handle):
    """The cells of the pair count as those of the projected counts: ``(segment of a, segment of b, row, diagonal)``."""
    p, q, ka, kb, row = pair_cells(one_handle).T
    sa, sb = p * NB + ka, q * NB + kb
    return np.ascontiguousarray(np.column_stack([sa, sb, row, (sa == sb) & one_handle]).astype(np.int32))


def all_jobs():
    return np.array([(p, q) for p in range(P) for q in range(P)], dtype=np.int32)


def auto_jobs():
    return np.array([(p, q) for p in range(P) for q in range(p, P)], dtype=np.int32)


def neighbours(reach=2):
    """Ordered patch pairs at most ``reach`` grid cells apart in either direction."""
    p = np.arange(P)
    near = (np.abs(p[:, None] % GRID_X - p[None, :] % GRID_X) <= reach) & (np.abs(p[:, None] // GRID_X - p[None, :] // GRID_X) <= reach)
    return np.argwhere(near).astype(np.int32)


def pair_cells(one_handle):
    """Cells ``(p, q, ka, kb, row)`` over the neighbouring patch pairs: inside both bins with the row of the bin (one handle:
    ``p <= q`` only), across the bins with alternating rows, and 600 cells of far patches that hold nothing."""
    near = neighbours()
    same = [(p, q, k, k, k) for p, q in near for k in range(NB) if p <= q or not one_handle]
    cross = [(p, q, ka, 1 - ka, (p + q) % 2) for p, q in near for ka in ((p + q) % 2,)]
    cross += [(p, q, 1, 0, 1) for p, q in near[::3]]
    far = [(p, P - 1 - p, p % 2, (p // 2) % 2, p % 2) for p in range(60)] * 10
    return np.array(same + cross + far, dtype=np.int32)


def shuffled(n, n_repeated=20, seed=5):
    """Indices into a list of ``n`` entries: a fixed permutation with ``n_repeated`` entries inserted a second time."""
    rng = np.random.default_rng(seed)
    index = rng.permutation(n)
    for r in rng.choice(n, n_repeated, replace=False):
        index = np.insert(index, rng.integers(0, len(index) + 1), r)
    return index


def small_cells(one_handle):
    """Six cells for the handles without objects (one handle: ``p <= q`` inside a bin)."""
    return np.array([(16, 16, 0, 0, 0), (16, 17, 1, 1, 1), (17, 16, 0, 1, 1), (31, 16, 1, 0, 0), (32, 32, 1, 1, 1), (0, 149, 0, 1, 0)]
                    if one_handle else [(16, 16, 0, 0, 0), (16, 17, 1, 1, 1), (17, 16, 0, 1, 1), (17, 16, 1, 1, 1), (32, 32, 1, 1, 1), (0, 149, 0, 1, 0)],
                    dtype=np.int32)


# --------------------------------------------------------------------------- the four counts behind one interface
class Count:
    """One entry point: its handles, its full list, the oracle on a list, and the check of its own suite."""

    def __init__(self, name):
        self.name = name
        self.lens, self.src, self.cat, self.cat_b = scene()
        if name == "radial":  # m = D_A^2 as the driver sends it for kpc and Mpc (engine.dsigma_radial_columns)
            self.lens = dict(self.lens, m=self.lens["f"] * self.lens["f"])
        if name in PROJ:
            self.pa, self.pb, self.pe = proj_scene()
            if name != "proj2":
                self.pb = self.pa
        self.t = self.rows()

    def rows(self, n_rows=NB):
        """The thresholds of the count: squared chords, or squared radii for the radial count."""
        if self.name in PROJ:  # squared radii around the median D of a pair; the nearest object reaches 12 times as far in s2
            return radii2(self.pa["d"] ** 2, n_rows)
        return radii2(self.lens["m"], n_rows) if self.name == "radial" else thresholds(n_rows)

    def full_list(self):
        return {"shear": all_jobs, "dsigma": all_jobs, "radial": all_jobs, "auto": auto_jobs, "pair": lambda: pair_cells(True),
                "pair2": lambda: pair_cells(False), "proj": lambda: proj_cells(True), "proj2": lambda: proj_cells(False),
                "proj_pi": lambda: proj_cells(True)}[self.name]()

    def small_list(self):
        """The 6-entry call: the first four entries of the full list that hold pairs, and its first and last, which hold none."""
        entries = self.full_list()
        live = expected(self.name)[-1].reshape(len(entries), -1).sum(axis=1) > 0
        assert not live[0] and not live[-1]
        return entries[np.concatenate([np.flatnonzero(live)[:4], [0, len(entries) - 1]])]

    def cells_of(self, entries):
        return len(entries) * (NB if self.name in ("shear", "dsigma", "radial", "auto") else 1)

    def upload(self, ctx, sort_axis=2):
        if self.name in PROJ:
            handles = tuple(_lib.ProjHandle(ctx, h["x"], h["y"], h["z"], h["w"], h["d"], h["c"], P, NB, h["off"], sort_axis=sort_axis)
                            for h in ((self.pa,) if self.pb is self.pa else (self.pa, self.pb)))
            return handles
        if self.name == "shear":
            return test_gpu_shear.upload(ctx, self.lens, self.src, sort_axis)
        if self.name in ("dsigma", "radial"):
            lenses = _lib.DsigmaLenses(ctx, *(self.lens[c] for c in "xyzwfc"), P, self.lens["nb"], self.lens["off"], sort_axis=sort_axis,
                                       m=self.lens.get("m"))
            sources = _lib.ShearSources(ctx, *(self.src[c] for c in ("x", "y", "z", "w", "g1", "g2")), P, self.src["off"], sort_axis=sort_axis,
                                        u=self.src["u"])
            return lenses, sources
        a = test_gpu_shear_auto.upload(ctx, self.cat, sort_axis)
        return (a,) if self.name != "pair2" else (a, test_gpu_shear_auto.upload(ctx, self.cat_b, sort_axis))

    def run(self, ctx, handles, entries, t=None, exchanged=False):
        """-> (planes..., stats); ``exchanged`` (pair2): the two handles in the other order, the cells transposed."""
        t = self.t if t is None else t
        if self.name in PROJ:
            return self.run_proj(ctx, handles, entries, self.name == "proj_pi", t)
        if self.name == "shear":
            return _lib.shear_count(ctx, *handles, entries, t)
        if self.name == "dsigma":
            return _lib.dsigma_count(ctx, *handles, entries, t)
        if self.name == "radial":
            return _lib.dsigma_count_radial(ctx, *handles, entries, t)
        if self.name == "auto":
            return _lib.shear_auto_count(ctx, handles[0], entries, t)
        if exchanged:
            return _lib.shear_pair_count(ctx, handles[1], handles[0], np.ascontiguousarray(entries[:, [1, 0, 3, 2, 4]]), t)
        return _lib.shear_pair_count(ctx, handles[0], handles[-1], entries, t)

    def run_proj(self, ctx, handles, entries, planes, t=None):
        """``proj_count`` -> (W[cells, nf], stats), or ``proj_count_pi`` -> (W[cells, n_pi, nf], stats): its planes per cell."""
        t = self.t if t is None else t
        if not planes:
            return _lib.proj_count(ctx, handles[0], handles[-1], entries, t, PROJ_PMAX)
        W, stats = _lib.proj_count_pi(ctx, handles[0], handles[-1], entries, t, self.pe)
        assert W.shape == (len(self.pe) - 1, len(entries), t.shape[1] - 1)
        return np.ascontiguousarray(W.transpose(1, 0, 2)), stats

    def oracle(self, entries, planes=None):
        if self.name in PROJ:
            if self.name == "proj_pi" if planes is None else planes:
                return (np.ascontiguousarray(proj_pi_oracle.proj_pi_cells(self.pa, self.pb, entries, self.t, self.pe)[2].transpose(1, 0, 2)),)
            return (proj_oracle.proj_cells(self.pa, self.pb, entries, self.t, PROJ_PMAX)[2],)
        if self.name == "shear":
            return shear_oracle.shear_jobs(self.lens, self.src, entries, self.t)
        if self.name == "dsigma":
            return dsigma_oracle.dsigma_jobs(self.lens, self.src, entries, self.t)
        if self.name == "radial":
            return dsigma_radial_oracle.radial_jobs(self.lens, self.src, entries, self.t)[:4]
        if self.name == "auto":
            return shear_auto_oracle.shear_auto_jobs(self.cat, entries, self.t)
        return shear_pair_oracle.shear_pair_cells(self.cat, self.cat if self.name == "pair" else self.cat_b, entries, self.t)

    def check(self, key, got, exp):
        if self.name in PROJ:  # unit weights: the integer number of pairs, and +0.0 where there is none
            assert len(got) == len(exp) == 1 and np.array_equal(got[0], exp[0]) and not np.any(np.signbit(got[0])), (key, np.abs(got[0] - exp[0]).sum())
            return
        (test_gpu_shear if self.name in ("shear", "dsigma", "radial") else test_gpu_shear_auto).check_against_oracle(key, got, exp)


COUNTS = ["shear", "dsigma", "radial", "auto", "pair", "pair2", "proj", "proj2", "proj_pi"]


@functools.lru_cache(maxsize=None)
def expected(name):
    """The oracle of the count's full list: once per count, shared, never modified."""
    count = Count(name)
    return freeze(count.oracle(count.full_list()))


def free(handles):
    for h in handles:
        h.free()


# --------------------------------------------------------------------------- 1. the full lists
@pytest.mark.parametrize("order", ["as listed", "shuffled"])
@pytest.mark.parametrize("name", COUNTS)
def test_full_list_matches_the_oracle(name, order):
    """All 150^2 jobs (tangential, Delta Sigma), all p <= q jobs (auto), thousands of cells (pair count on one and on two
    handles); shuffled: the same list in a fixed random order with 20 entries twice -- the rows are the oracle's rows of those
    entries, and a repeated entry returns the same bits in both of its slots."""
    count = Count(name)
    entries, exp = count.full_list(), expected(name)
    live = exp[-1].reshape(len(entries), -1).sum(axis=1) > 0
    assert len(entries) > 5000 and live.sum() > 250 and (~live).sum() > len(entries) // 3  # many cells with pairs, more without
    index = np.arange(len(entries)) if order == "as listed" else shuffled(len(entries))
    ctx = engine.get_context(0)
    handles = count.upload(ctx)
    try:
        *got, stats = count.run(ctx, handles, entries[index])
    finally:
        free(handles)
    n_cells = count.cells_of(index)
    assert len(index) > 1024 and n_cells > 2048 and stats.n_workgroups == n_cells and stats.evaluated_pairs > 0
    count.check(f"{name} {order}: {len(index)} entries, {n_cells} cells", got, tuple(plane[index] for plane in exp))
    if order == "shuffled":
        twice = [np.flatnonzero(index == v) for v in np.flatnonzero(np.bincount(index) > 1)]
        assert len(twice) == 20
        for first, second in twice:
            for plane in got:
                assert np.array_equal(plane[first], plane[second]), (name, index[first])


# --------------------------------------------------------------------------- 2. one handle through calls of other sizes
@pytest.mark.parametrize("name", COUNTS)
def test_a_handle_through_calls_that_grow_and_shrink(name):
    """A 6-entry call, the full list, the 6-entry call again on the same handles: the first and the third are the same bits,
    the middle one the bits of the same call on freshly uploaded handles. Between two handles of the pair count the full list
    also runs with the handles exchanged (and again after it), so that the buffers of both have been the call's. On the
    handles of the projected count ``proj_count`` and ``proj_count_pi`` also take turns (few / full / few): the call's input and
    result blocks are then laid out both ways in the same buffers, and every turn is the bits of that call on fresh handles."""
    count = Count(name)
    entries, few = count.full_list(), count.small_list()
    ctx = engine.get_context(0)
    handles = count.upload(ctx)
    try:
        first = count.run(ctx, handles, few)[:-1]
        middle = count.run(ctx, handles, entries)[:-1]
        if name == "pair2":
            few_exchanged = count.run(ctx, handles, few, exchanged=True)[:-1]
            middle_exchanged = count.run(ctx, handles, entries, exchanged=True)[:-1]
            middle_again = count.run(ctx, handles, entries)[:-1]
            few_exchanged_again = count.run(ctx, handles, few, exchanged=True)[:-1]
        if name in ("proj", "proj2"):  # the two entry points in turn: d_in and d_out laid out both ways, few / full / few
            turns = [count.run_proj(ctx, handles, list_, planes)[0] for list_, planes in ((few, True), (entries, False), (entries, True), (few, False), (few, True))]
        third = count.run(ctx, handles, few)[:-1]
    finally:
        free(handles)
    fresh = count.upload(ctx)
    try:
        alone = count.run(ctx, fresh, entries)[:-1]
    finally:
        free(fresh)
    if name in ("proj", "proj2"):  # every turn is the bits of the same call on fresh handles, and the oracle's integers
        for list_ in (few, entries):
            fresh = count.upload(ctx)
            try:
                planes_alone = count.run_proj(ctx, fresh, list_, True)[0]
            finally:
                free(fresh)
            for turn in (turns[0], turns[4]) if list_ is few else (turns[2],):
                assert np.array_equal(turn, planes_alone)
            assert np.array_equal(planes_alone, count.oracle(list_, planes=True)[0]) and planes_alone.sum() > 0
            assert np.array_equal(planes_alone.sum(axis=1), (first if list_ is few else alone)[0])  # the planes sum to the single cylinder
        assert np.array_equal(turns[1], alone[0]) and np.array_equal(turns[3], first[0])
    exp_few = count.oracle(few)
    assert np.count_nonzero(exp_few[-1].reshape(len(few), -1).sum(axis=1)) == 4
    count.check(f"{name} 6 entries", first, exp_few)
    for a, b in zip(first, third):
        assert np.array_equal(a, b)
    for a, b in zip(middle, alone):
        assert np.array_equal(a, b)
    if name == "pair2":
        for a, b in zip(middle, middle_again):
            assert np.array_equal(a, b)
        for a, b in zip(few_exchanged, few_exchanged_again):
            assert np.array_equal(a, b)
        count.check("pair2 exchanged, 6 entries", few_exchanged, exp_few)
        count.check("pair2 exchanged, full list", middle_exchanged, expected(name))


# --------------------------------------------------------------------------- 3. unbinned lenses under many rows
@pytest.mark.parametrize("name", ["shear", "dsigma", "radial"])
def test_unbinned_lenses_under_eight_rows_of_thresholds(name):
    """``nb == 1`` lenses, 8 rows of thresholds, 2000 jobs: all 8 cells of a job stream the one lens segment of its patch, each
    with the edges of its own row (``Tangential::cell`` / ``DeltaSigma::cell``)."""
    count = Count(name)
    count.lens = dict(count.lens, nb=1, off=count.lens["off"][::NB].copy())
    count.t = count.rows(8)
    near = neighbours()
    jobs = near[np.random.default_rng(9).choice(len(near), 2000, replace=False)]
    exp = count.oracle(jobs)
    rows_with_pairs = exp[2].sum(axis=(0, 2)) > 0
    assert rows_with_pairs.all() and np.count_nonzero(np.any(exp[2][:, 0] != exp[2][:, 7], axis=1)) > 100  # the rows differ
    ctx = engine.get_context(0)
    if name == "shear":
        handles = test_gpu_shear.upload(ctx, count.lens, count.src, 2)
    elif name == "radial":
        handles = count.upload(ctx)  # (the lenses as they are now: one bin)
    else:
        lenses = _lib.DsigmaLenses(ctx, *(count.lens[c] for c in "xyzwfc"), P, 1, count.lens["off"])
        handles = (lenses, _lib.ShearSources(ctx, *(count.src[c] for c in ("x", "y", "z", "w", "g1", "g2")), P, count.src["off"], u=count.src["u"]))
    try:
        *got, stats = count.run(ctx, handles, jobs)
    finally:
        free(handles)
    assert stats.n_workgroups == 2000 * 8 and stats.evaluated_pairs > 0
    count.check(f"{name} nb=1, 8 rows, 2000 jobs", got, exp)


# --------------------------------------------------------------------------- 4. handles without objects
def empty_like(cat, n_bins):
    none = np.empty(0, dtype=np.float64)
    return dict({c: none for c in cat if c not in ("nb", "off")}, nb=n_bins, off=np.zeros(P * n_bins + 1, dtype=np.int64))


def assert_nothing(key, result, n_cells):
    *planes, stats = result
    assert stats.evaluated_pairs == 0 and stats.candidate_pairs == 0 and stats.n_workgroups == n_cells, key
    for plane in planes:
        assert plane.size > 0 and np.all(plane == 0.0) and not np.any(np.signbit(plane)), key


def test_handles_without_objects():
    """A handle uploaded with ``n = 0`` uploads, counts to all-zero planes with no pair evaluated, and is freed: as sources, as
    lenses (a catalogue handle, a lens handle and a radial lens handle), as the catalogue of the auto count and on either side
    of the pair count. The radial count besides: lenses whose second redshift bin is empty in every patch. The two projected
    counts: an empty handle as the first, as the second and as both."""
    lens, src, cat, _ = scene()
    no_lens, no_src, no_cat = empty_like(lens, NB), empty_like(src, 1), empty_like(cat, NB)
    t = thresholds()
    jobs, cells = SMALL, small_cells(False)
    ctx = engine.get_context(0)

    def dsigma_handles(lens_, src_):
        lenses = _lib.DsigmaLenses(ctx, *(lens_[c] for c in "xyzwfc"), P, NB, lens_["off"])
        return lenses, _lib.ShearSources(ctx, *(src_[c] for c in ("x", "y", "z", "w", "g1", "g2")), P, src_["off"], u=src_["u"])

    for lens_, src_ in ((lens, no_src), (no_lens, src), (no_lens, no_src)):
        key = f"{len(lens_['x'])} lenses, {len(src_['x'])} sources"
        handles = test_gpu_shear.upload(ctx, lens_, src_, 2)
        try:
            assert_nothing("shear " + key, _lib.shear_count(ctx, *handles, jobs, t), len(jobs) * NB)
        finally:
            free(handles)
        handles = dsigma_handles(lens_, src_)
        try:
            assert_nothing("dsigma " + key, _lib.dsigma_count(ctx, *handles, jobs, t), len(jobs) * NB)
        finally:
            free(handles)
    nobody, somebody = test_gpu_shear_auto.upload(ctx, no_cat), test_gpu_shear_auto.upload(ctx, cat)
    try:
        assert_nothing("auto", _lib.shear_auto_count(ctx, nobody, np.sort(jobs, axis=1), t), len(jobs) * NB)
        for key, a, b in (("pair, a empty", nobody, somebody), ("pair, b empty", somebody, nobody), ("pair, one empty handle", nobody, nobody)):
            assert_nothing(key, _lib.shear_pair_count(ctx, a, b, small_cells(a is b) if a is b else cells, t), 6)
        count = Count("pair")  # the handle with objects is still good
        few = count.small_list()
        count.check("after the empty handles", _lib.shear_pair_count(ctx, somebody, somebody, few, t)[:4], count.oracle(few))
    finally:
        free((nobody, somebody))

    # the radial count: a lens handle with n == 0 still carries a column m, and sources without objects
    radial = Count("radial")
    full, r2 = radial.lens, radial.t

    def radial_handles(lens_, src_):
        lenses = _lib.DsigmaLenses(ctx, *(lens_[c] for c in "xyzwfc"), P, NB, lens_["off"], m=lens_["m"])
        return lenses, _lib.ShearSources(ctx, *(src_[c] for c in ("x", "y", "z", "w", "g1", "g2")), P, src_["off"], u=src_["u"])

    for lens_, src_ in ((full, no_src), (empty_like(full, NB), src), (empty_like(full, NB), no_src)):
        handles = radial_handles(lens_, src_)
        try:
            assert_nothing(f"radial {len(lens_['x'])} lenses, {len(src_['x'])} sources", _lib.dsigma_count_radial(ctx, *handles, jobs, r2),
                           len(jobs) * NB)
        finally:
            free(handles)
    # ... and a redshift bin without a lens in any patch (min_m = +inf, a reach of 0): its row takes any last edge and stays
    # exactly +0.0; the first row is the bits of the call on all lenses
    in_first = (np.searchsorted(full["off"], np.arange(len(full["x"])), side="right") - 1) % NB == 0
    sizes = np.diff(full["off"]) * (np.arange(P * NB) % NB == 0)
    first_only = dict({c: full[c][in_first] for c in "xyzwfcm"}, nb=NB, off=np.concatenate([[0], np.cumsum(sizes)]).astype(np.int64))
    assert 50 < in_first.sum() < len(in_first) - 50
    far_edge = r2.copy()
    far_edge[1, -1] = 1e30
    in_row = expected("radial")[2].sum(axis=2) > 0  # three jobs with pairs in the first row, three in the second
    few = radial.full_list()[np.concatenate([np.flatnonzero(in_row[:, 0])[:3], np.flatnonzero(in_row[:, 1] & ~in_row[:, 0])[:3]])]
    all_lenses, one_bin = radial_handles(full, src), radial_handles(first_only, src)
    try:
        with pytest.raises(_lib.YawhipError, match="a lens is too close for the largest radius"):
            _lib.dsigma_count_radial(ctx, *all_lenses, few, far_edge)  # (with lenses in that bin the edge is refused)
        *both, _ = _lib.dsigma_count_radial(ctx, *all_lenses, few, r2)
        *first, stats = _lib.dsigma_count_radial(ctx, *one_bin, few, far_edge)
    finally:
        free(all_lenses + one_bin)
    assert stats.n_workgroups == len(few) * NB and stats.evaluated_pairs > 0
    exp = radial.oracle(few)
    assert np.count_nonzero(exp[2][:, 0].sum(axis=1)) >= 3 and np.count_nonzero(exp[2][:, 1].sum(axis=1)) >= 3  # both rows hold pairs
    radial.check("radial, 6 jobs", both, exp)
    for ours, ref in zip(first, both):
        assert np.array_equal(ours[:, 0], ref[:, 0])
        assert np.all(ours[:, 1] == 0.0) and not np.any(np.signbit(ours[:, 1]))

    # the projected counts: a handle with n == 0 on either side and on both, through both entry points
    proj = Count("proj2")
    no_proj = dict(empty_like(proj.pa, NB), w=None)
    few = proj.small_list()
    for first_, second_ in ((proj.pa, no_proj), (no_proj, proj.pb), (no_proj, no_proj)):
        handles = tuple(_lib.ProjHandle(ctx, h["x"], h["y"], h["z"], h["w"], h["d"], h["c"], P, NB, h["off"]) for h in (first_, second_))
        try:
            key = f"proj {len(first_['x'])} with {len(second_['x'])} objects"
            assert_nothing(key, _lib.proj_count(ctx, *handles, few, proj.t, PROJ_PMAX), len(few))
            assert_nothing(key + ", pi", _lib.proj_count_pi(ctx, *handles, few, proj.t, proj.pe), len(few))
            if first_ is second_:  # one empty handle with itself, its diagonal cells included
                one = Count("proj").small_list()
                assert np.any(one[:, 3] != 0)
                assert_nothing(key + ", one handle", _lib.proj_count_pi(ctx, handles[0], handles[0], one, proj.t, proj.pe), len(one))
        finally:
            free(handles)
