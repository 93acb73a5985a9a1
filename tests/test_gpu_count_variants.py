"""Every reachable compiled count-kernel variant against the CPU oracle.

``CASES`` is a table: each case names the input it counts (catalogue pair and threshold grid), the documented options it
sets and the two kernel variants it must reach -- the unweighted and the weighted launch of a weighted count that returns
counts and sums. The library reports what it launched (``yawhip_stats.count_variant*``, rendered by ``_lib.variant_name`` as
``nm -C`` prints the kernel), so reach is read from the library itself. tests/test_count_variants.py checks, without a GPU,
that the cases together with ``UNREACHABLE`` account for every ``k_count*`` instantiation of the built library.

The inputs are built for the parts where kernels go wrong: partners within a few ulp of every edge of every grid (float32
guard bands), lane tiles with tails, an empty patch and an empty (patch, bin) segment, diagonal and off-diagonal jobs,
weights over six decades, a clump whose windows are longer than every LDS stage, self counts (half bands on and off),
more fine bins than private histograms fit the LDS (k_count with PRIV = false) and, in every third band case, a
flush of the 32-bit counters after every stage. Counts must equal the oracle bit for bit, weighted sums to 1e-10, and a
weighted call repeated must give the same sums bit for bit.
"""
from __future__ import annotations

import functools
from dataclasses import dataclass, field

import numpy as np
import pytest

from conftest import ARCMIN
from oracle import oracle

pytestmark = pytest.mark.gpu
RTOL_W = 1e-10

B, P = 3, 4
STRIP_MICRO = 2000         # grid spacing 2e-3 > chord of the largest separation (6' -> 1.745e-3): reach 1, triples possible
BIN_SCALE = (1.0, 0.85, 0.7)  # per-bin threshold rows ("/bins"): bin k's angles x BIN_SCALE[k]
GRIDS = {                  # edges in arcmin (bin 0's row); the largest separation is 6' in every grid
    "e2": np.array([1.0, 6.0]),
    "e3": np.array([1.0, 2.5, 6.0]),
    "e4": np.array([1.0, 2.0, 3.5, 6.0]),
    "fine": oracle.ang_bins_for(oracle.parse_ang_limits([0.5 * ARCMIN], [6.0 * ARCMIN]), -1.0, 24) / ARCMIN,  # 25 edges, log-spaced
    "many": np.linspace(0.05, 6.0, 201),  # 200 fine bins: k_count's private histograms exceed the LDS
}
# option defaults of a context (include/yawhip.h), restored after every case
DEFAULTS = {"kernel": 0, "tile_r": 0, "band_cap": 0, "triple_runs": 1, "band_fp32": 1, "half_bands": 1, "seg_strips": 1,
            "flush_stages_log2": 17, "seg_strips_min_run": 16}
KERNEL = {"exact": 1, "filter": 2, "sweep": 3, "band": 4}


def angles(grid: str) -> np.ndarray:
    """Edge angles in radian, [B, E]."""
    name, _, per_bin = grid.partition("/")
    row = GRIDS[name] * ARCMIN
    return np.stack([row * (BIN_SCALE[k] if per_bin else 1.0) for k in range(B)])


def thresholds(grid: str) -> np.ndarray:
    """[B, E] thresholds of a grid. Every edge of the engineered grids is moved (by a few ulp) onto the squared chord of an
    engineered pair of its bin, so that pairs lie EXACTLY on every edge too (s == t belongs to the lower fine bin)."""
    t = np.stack([oracle.thresholds_for(a) for a in angles(grid)])
    if grid.startswith("many"):
        return t
    ties = _catalogues()[1]
    per_bin = "/" in grid
    for k in range(B):
        cand = ties[k] if per_bin else np.concatenate(ties)
        for e in range(t.shape[1]):
            s = cand[np.argmin(np.abs(cand - t[0 if not per_bin else k, e]))]
            assert abs(s - t[k, e]) <= 1e-12 * t[k, e], (grid, k, e)
            t[k, e] = s
        if not per_bin:
            t[:] = t[0]
            break
    assert np.all(np.diff(t, axis=1) > 0)
    return t


# ----------------------------------------------------------------------------------------------------------------- the table
@dataclass(frozen=True)
class Case:
    id: str
    pair: str                # "cross": binned c1 x unbinned c2 (merged items), "binned": binned c1 x binned c2, "self": c1 x c1
    grid: str                # key of GRIDS, "/bins": a threshold row per redshift bin
    options: dict            # documented options of yawhip_ctx_set_option
    reach: tuple             # variant names of the unweighted and the weighted launch
    alt: tuple = field(default=())  # further option settings the case also runs: same variants, same results
    reevaluates: bool = False       # float32 classification: the engineered partners must go to the exact predicate


def _b(v: bool) -> str:
    return "true" if v else "false"


def _pair_reach(family: str, *args) -> tuple:
    """(unweighted, weighted) names of a kernel whose WEIGHTED argument is at position 2 (band kernels) or 1 (the others)."""
    pos = 2 if family.startswith("k_count_band") else 1
    names = []
    for w in (False, True):
        a = list(args)
        a.insert(pos, w)
        names.append(f"{family}<{', '.join(_b(v) if isinstance(v, bool) else str(v) for v in a)}>")
    return tuple(names)


S64 = ((1, 192), (2, 192), (2, 288), (4, 288))  # (R, CAP) of k_count_band / k_count_band32_fine
S32 = ((1, 320), (2, 320), (2, 512), (4, 512))  # ... of k_count_band32 / _one
COERCED = {192: 288, 288: 192, 320: 512, 512: 320}


def _stage_options(r: int, cap: int, n: int) -> dict:
    """tile_r and band_cap for a stage. One object per lane has only the small stage, four only the large one: every other
    such case asks for the other capacity, which the planner must overrule."""
    if r == 2:
        return {"tile_r": 2, "band_cap": cap}
    return {"tile_r": r, "band_cap": COERCED[cap] if n % 2 else 0}


def _build_cases() -> list:
    cases = []

    def add(fam_id, pair, grid, options, reach, **kw):
        n = len(cases)
        if options.get("kernel") == "band" and n % 3 == 0:
            options = {**options, "flush_stages_log2": 0}  # mid-item flush of the 32-bit LDS counters
        tag = ",".join(f"{k}={v}" for k, v in options.items())
        cases.append(Case(f"{fam_id}-{pair}-{grid}-{tag}", pair, grid, options, reach, **kw))

    # float32 band kernels: one window per item (merged triple runs) or three (the chunk loop)
    for one in (True, False):
        fam = "k_count_band32_one" if one else "k_count_band32"
        for r, cap in S32:
            for merged, per_bin in ((True, False), (True, True), (False, None)):
                for ne in (2, 3, 4):
                    if merged:
                        pair, grid, uni = "cross", f"e{ne}" + ("/bins" if per_bin else ""), not per_bin
                    else:  # per-bin items have one threshold row each (UNI), whatever the rows of the bins are
                        pair, grid, uni = "self" if one and r == 1 else "binned", f"e{ne}" + ("/bins" if ne == 3 else ""), True
                    opts = {"kernel": "band", "band_fp32": 1, "triple_runs": 2 if one else 0, **_stage_options(r, cap, len(cases))}
                    alt = ({"half_bands": 0},) if pair == "self" else ()
                    add(fam, pair, grid, opts, _pair_reach(fam, r, cap, ne, merged, uni), alt=alt, reevaluates=True)
    # float32 fine-grid kernel (more than four log-spaced edges)
    for r, cap in S64:
        for merged, uni in ((True, True), (True, False), (False, True), (False, False)):
            pair, grid = ("cross" if merged else "binned"), "fine" + ("" if uni else "/bins")
            opts = {"kernel": "band", "band_fp32": 1, "triple_runs": 2 * (len(cases) % 2), **_stage_options(r, cap, len(cases))}
            add("k_count_band32_fine", pair, grid, opts, _pair_reach("k_count_band32_fine", r, cap, merged, uni), reevaluates=True)
    # float64 band kernel. NE: the edge count up to four edges, 0 beyond; merged items with a threshold row per bin only have
    # NE = 2 (one fine bin) or 0 -- three or four edges there are coerced to 0 (see UNREACHABLE)
    for r, cap in S64:
        rows = [("cross", "fine", 0), ("cross", "e2", 2), ("cross", "e3", 3), ("cross", "e4", 4),
                ("cross", "e4/bins" if r % 2 else "fine/bins", 0), ("cross", "e2/bins", 2),
                ("binned", "fine/bins", 0), ("binned", "e2", 2), ("binned", "e3/bins", 3), ("binned", "e4", 4)]
        for pair, grid, ne in rows:
            merged, uni = pair == "cross", "/bins" not in grid or pair != "cross"
            opts = {"kernel": "band", "band_fp32": 0, **_stage_options(r, cap, len(cases))}
            if pair == "binned" and ne in (0, 3):
                opts["seg_strips"] = 0  # ordinary (job, bin) items on the plain layout (layout mode 0)
            add("k_count_band", pair, grid, opts, _pair_reach("k_count_band", r, cap, ne, merged, uni))
    # lean sweep kernel: four objects per lane in k_count_merged, one and two in its eight-wave twin
    for r in (1, 2, 4):
        for nf1 in (True, False):
            for merged in (True, False):
                fam = "k_count_merged_occ8" if r <= 2 else "k_count_merged"
                grid = "e2" if nf1 else ("e4/bins" if merged else "fine")
                opts = {"kernel": "sweep", "tile_r": r}
                if not merged and r == 2:
                    opts["seg_strips"] = 0
                add(fam, "cross" if merged else "binned", grid, opts, _pair_reach(fam, r, nf1, merged))
    # brute-force kernels: private per-lane histograms while they fit the LDS, one shared histogram beyond
    for kernel in ("exact", "filter"):
        for r in (1, 2, 4):
            for priv in (True, False):
                grid = ("e3" if r != 2 else "e4/bins") if priv else "many"
                add("k_count", "cross" if r != 1 else "binned", grid, {"kernel": kernel, "tile_r": r},
                    _pair_reach("k_count", r, priv, kernel == "filter"))
    return cases


CASES = _build_cases()

# Compiled variants that make_plan never picks, with the reason.
UNREACHABLE = {
    f"k_count_band<{r}, {cap}, {_b(w)}, {ne}, true, false>":
        "make_plan: band_ne = n_edges only for per-bin items or one threshold row for all bins; merged items whose bins have "
        "their own rows get NE = 2 (one fine bin) or 0"
    for r, cap in S64 for w in (False, True) for ne in (3, 4)
}


def reached() -> set:
    return {name for c in CASES for name in c.reach}


# ------------------------------------------------------------------------------------------------------------------ inputs
@functools.lru_cache(maxsize=1)
def _catalogues():
    """(catalogues, ties). c1: binned, weighted; an empty patch (3) and an empty segment (patch 1, bin 1). c2: uniform objects, a partner of
    every fourth c1 object placed at theta_edge (1 + delta) of an edge of that object's bin in one of the grids (delta from 0
    to 1e-6, within a few ulp in most), and a clump shared with c1; binned with the redshift of the partnered object, and
    unbinned. Footprint 1.5 x 1.5 deg in four quadrant patches. ties[k]: squared chords of the partners of bin k's objects."""
    rng = np.random.default_rng(20261015)

    def sky(n):
        return np.deg2rad(rng.uniform(30.0, 31.5, n)), np.arcsin(rng.uniform(np.sin(np.deg2rad(-0.75)), np.sin(np.deg2rad(0.75)), n))

    def clump(n):
        return np.deg2rad(30.4 + rng.normal(0.0, 0.03, n)), np.deg2rad(-0.4 + rng.normal(0.0, 0.03, n))

    def patch_of(ra, dec):
        return (ra > np.deg2rad(30.75)).astype(np.int64) + 2 * (dec > 0.0)

    zedges = np.linspace(0.1, 0.9, B + 1)
    ra1, dec1 = (np.concatenate(v) for v in zip(sky(21000), clump(3000)))
    z1 = rng.uniform(0.11, 0.89, len(ra1))
    k1 = np.digitize(z1, zedges, right=True) - 1
    p1 = patch_of(ra1, dec1)
    keep = (p1 != 3) & ~((p1 == 1) & (k1 == 1))
    ra1, dec1, z1, k1, p1 = ra1[keep], dec1[keep], z1[keep], k1[keep], p1[keep]
    n1 = len(ra1)
    w1 = 10.0 ** rng.uniform(-3.0, 3.0, n1)

    # engineered partners: one edge of the object's bin, from all grids but the 200-bin one
    src = rng.choice(n1, n1 // 4, replace=False)
    edge_lists = [np.unique(np.concatenate([angles(g + s)[k] for g in ("e2", "e3", "e4", "fine") for s in ("", "/bins")]))
                  for k in range(B)]
    edge = np.array([rng.choice(edge_lists[k1[i]]) for i in src])
    delta = rng.choice([0.0, 1e-16, -1e-16, 2e-16, -2e-16, 4e-16, -4e-16, 1e-14, -1e-14, 1e-12, -1e-12, 1e-9, -1e-9, 1e-6, -1e-6],
                       len(src))
    a = np.column_stack(oracle.to_3d(ra1[src], dec1[src]))
    v = rng.normal(size=a.shape)
    v -= (v * a).sum(1, keepdims=True) * a
    v /= np.linalg.norm(v, axis=1, keepdims=True)
    ang = edge * (1.0 + delta)
    b = a * np.cos(ang)[:, None] + v * np.sin(ang)[:, None]
    b /= np.linalg.norm(b, axis=1, keepdims=True)
    ra_p, dec_p = np.arctan2(b[:, 1], b[:, 0]) % (2 * np.pi), np.arcsin(np.clip(b[:, 2], -1.0, 1.0))

    ra_u, dec_u = sky(20000)
    ra_c, dec_c = clump(3000)
    ra2 = np.concatenate([ra_u, ra_c, ra_p])
    dec2 = np.concatenate([dec_u, dec_c, dec_p])
    z2 = np.concatenate([rng.uniform(0.11, 0.89, len(ra_u) + len(ra_c)), z1[src]])
    w2 = 10.0 ** rng.uniform(-3.0, 3.0, len(ra2))
    p2 = patch_of(ra2, dec2)
    # the library's predicate: s = ((ax - bx)^2 + (ay - by)^2) + (az - bz)^2 in float64, of the coordinates the catalogues hold
    xa, xb = np.column_stack(oracle.to_3d(ra1[src], dec1[src])), np.column_stack(oracle.to_3d(ra_p, dec_p))
    d = xa - xb
    s = (d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1]) + d[:, 2] * d[:, 2]
    ties = [np.sort(s[k1[src] == k]) for k in range(B)]
    return {
        "c1": oracle.sort_catalog(ra1, dec1, z1, w1, p1, P, zedges, "right"),
        "c2b": oracle.sort_catalog(ra2, dec2, z2, w2, p2, P, zedges, "right"),
        "c2u": oracle.sort_catalog(ra2, dec2, None, w2, p2, P, None, "right"),
    }, ties


PAIRS = {"cross": ("c1", "c2u"), "binned": ("c1", "c2b"), "self": ("c1", "c1")}
JOBS = np.array([(p, q) for p in range(P) for q in range(P)], dtype=np.int32)  # diagonal and off-diagonal, empty patch 3 included


@pytest.fixture(scope="module")
def cats():
    return _catalogues()[0]


@pytest.fixture(scope="module")
def expected(cats):
    """Oracle (counts, sums) per (pair, grid), computed once."""
    memo = {}

    def get(pair, grid):
        if (pair, grid) not in memo:
            a, b = PAIRS[pair]
            memo[(pair, grid)] = oracle.count_jobs(cats[a], cats[b], JOBS, thresholds(grid))
        return memo[(pair, grid)]

    return get


def _upload(ctx, cat):
    from yet_another_wizz_amd import _lib

    return _lib.DeviceCatalog(ctx, cat["x"], cat["y"], cat["z"], cat["w"], P, cat["nb"], cat["off"], strip_micro=STRIP_MICRO)


class _Device:
    """A context with the catalogues uploaded on the strip grid of the table."""

    def __init__(self, device, cats):
        from yet_another_wizz_amd import _lib

        self.ctx = _lib.Context(device)
        try:
            self.dev = {name: _upload(self.ctx, c) for name, c in cats.items()}
        finally:
            self.ctx.set_option("strip_width_micro", _lib.DEFAULT_STRIP_MICRO)

    def pair(self, name):
        a, b = PAIRS[name]
        return self.dev[a], self.dev[b]

    def close(self):
        for d in self.dev.values():
            d.free()
        self.ctx.close()


@pytest.fixture(scope="module")
def device(cats):
    d = _Device(0, cats)
    yield d
    d.close()


def _apply(ctx, options):
    for key, value in options.items():
        ctx.set_option(key, KERNEL.get(value, value) if key == "kernel" else value)


def _restore(ctx):
    _apply(ctx, DEFAULTS)


def _check_result(case, counts, sums, exp):
    exp_c, exp_s = exp
    assert np.array_equal(counts, exp_c), case.id
    np.testing.assert_allclose(sums, exp_s, rtol=RTOL_W, atol=0, err_msg=case.id)


def _run_case(d, case, expected):
    from yet_another_wizz_amd import _lib

    c1, c2 = d.pair(case.pair)
    exp = expected(case.pair, case.grid)
    assert exp[0].sum() > 10000 and np.count_nonzero(exp[0] == 0) > 0  # real pairs, and empty slots (patch 3, segment (1, 1))
    t = thresholds(case.grid)
    try:
        _apply(d.ctx, {"seg_strips_min_run": 1, **case.options})  # (per-bin strip runs of these sparse catalogues)
        for extra in ({}, *case.alt):
            _apply(d.ctx, extra)
            counts, sums, st = _lib.count_pairs(d.ctx, c1, c2, JOBS, t, want_counts=True, want_sums=True)
            assert st.variants == set(case.reach), (case.id, extra, st.variants)
            _check_result(case, counts, sums, exp)
            if case.reevaluates:
                assert st.exact_reevaluations > 0, case.id
            elif case.options.get("band_fp32") == 0:
                assert st.exact_reevaluations == 0, case.id
            # the weighted sums do not depend on the run (the ordering claim of yawhip.h; k_count with one histogram shared
            # by four waves is the documented exception)
            _, sums2, st2 = _lib.count_pairs(d.ctx, c1, c2, JOBS, t, want_counts=False, want_sums=True)
            assert st2.variants == {case.reach[1]}, case.id
            if case.reach[1].startswith("k_count<") and ", false, " in case.reach[1]:
                np.testing.assert_allclose(sums2, sums, rtol=RTOL_W, atol=0, err_msg=case.id)
            else:
                assert np.array_equal(sums2, sums), case.id
    finally:
        _restore(d.ctx)


@pytest.mark.parametrize("case", CASES, ids=[c.id for c in CASES])
def test_variant_against_oracle(device, expected, case):
    _run_case(device, case, expected)


def test_three_chunk_windows_are_longer_than_the_stage(cats):
    """The clump puts more streamed objects into one strip cell of a window (2 r_max along the sort axis, one grid spacing
    across) than the largest stage holds (512): the three-chunk kernels take such windows in several pieces."""
    c2 = cats["c2u"]
    r = 2.0 * np.sin(6.0 * ARCMIN / 2.0)
    w = STRIP_MICRO * 1e-6
    centre = np.array(oracle.to_3d(np.deg2rad(30.4), np.deg2rad(-0.4))).ravel()
    # library sort axis z, strips across y (footprint around x): a cell centred on the clump
    inside = (np.abs(c2["z"] - centre[2]) <= r) & (np.abs(c2["y"] - centre[1]) <= w / 2)
    assert inside.sum() > 2 * 512


def _dense_of(exp_s):
    """The dense tensor [1, B, P, P] of one scale over all fine bins, from the per-job sums."""
    dense = np.zeros((1, B, P, P))
    for j, (p, q) in enumerate(JOBS):
        dense[0, :, p, q] = exp_s[j].sum(axis=1)
    return dense


def _first(prefix: str, pair: str) -> Case:
    return next(c for c in CASES if c.reach[0].startswith(prefix + "<") and c.pair == pair)


# a few cases for the other entry points: every family, merged and per-bin items, a self count
ENTRY_CASES = [_first("k_count_band32_one", "self"), _first("k_count_band32", "cross"), _first("k_count_band32_fine", "binned"),
               _first("k_count_band", "cross"), _first("k_count_merged", "cross"), _first("k_count", "binned")]


def test_dense_batch_reports_each_request(device, expected):
    """yawhip_count_pairs_dense_batch: every request of the batch reports the kernel it ran and matches the oracle."""
    from yet_another_wizz_amd import _lib

    for case in ENTRY_CASES:
        t = thresholds(case.grid)
        slices = np.tile(np.array([[0, t.shape[1] - 1]], dtype=np.int32), (B, 1, 1))  # one scale over all fine bins
        try:
            _apply(device.ctx, {"seg_strips_min_run": 1, **case.options})
            reqs = [(*device.pair(case.pair), JOBS, False), (*device.pair(case.pair), JOBS[::-1].copy(), False)]
            out = _lib.count_pairs_dense_batch(device.ctx, reqs, t, slices, None)
        finally:
            _restore(device.ctx)
        want = _dense_of(expected(case.pair, case.grid)[1])
        for dense, st in out:
            assert st.count_variant == 0 and st.variants == {case.reach[1]}, case.id  # weighted: the sums only
            np.testing.assert_allclose(dense, want, rtol=RTOL_W, atol=0, err_msg=case.id)


def test_multi_stream_context_reports_the_variant(cats, expected):
    """A context of three streams on one device splits the job list; every share launches the case's variants and the
    report names them (not "mixed")."""
    from yet_another_wizz_amd import _lib

    d = _Device([0, 0, 0], cats)
    try:
        for case in ENTRY_CASES:
            c1, c2 = d.pair(case.pair)
            try:
                _apply(d.ctx, {"seg_strips_min_run": 1, **case.options})
                counts, sums, st = _lib.count_pairs(d.ctx, c1, c2, JOBS, thresholds(case.grid), want_counts=True, want_sums=True)
            finally:
                _restore(d.ctx)
            assert st.variants == set(case.reach), (case.id, st.variants)
            _check_result(case, counts, sums, expected(case.pair, case.grid))
    finally:
        d.close()


def test_pieces_with_different_variants_are_reported_mixed(cats):
    """A call counted in pieces (slab budget) or on several devices whose pieces launch different variants reports
    VARIANT_MIXED, not the last piece. k_count picks R from the longest lane-side segment of the jobs it is given: a job on a
    dense patch gets four objects per lane, one on a sparse patch one."""
    from yet_another_wizz_amd import _lib

    rng = np.random.default_rng(5)
    n = (12000, 300)  # patch 0 dense (R = 4), patch 1 sparse (R = 1)
    ra = np.deg2rad(np.concatenate([rng.uniform(10.0, 10.5, n[0]), rng.uniform(11.0, 11.5, n[1])]))
    dec = np.deg2rad(rng.uniform(0.0, 0.5, sum(n)))
    patch = np.repeat([0, 1], n)
    cat = oracle.sort_catalog(ra, dec, None, 10.0 ** rng.uniform(-2, 2, sum(n)), patch, 2, None, "right")
    jobs = np.array([[0, 0], [1, 1]], dtype=np.int32)
    t = thresholds("many")[:1]  # 200 fine bins: the slabs of the two jobs exceed the smallest budget
    exp_c, exp_s = oracle.count_jobs(cat, cat, jobs, t)
    name = {r: _pair_reach("k_count", r, False, False) for r in (1, 4)}
    for devices in (0, [0, 0]):
        ctx = _lib.Context(devices)
        d = None
        try:
            d = _lib.DeviceCatalog(ctx, cat["x"], cat["y"], cat["z"], cat["w"], 2, 1, cat["off"])
            ctx.set_option("kernel", KERNEL["exact"])
            for j, r in ((0, 4), (1, 1)):
                _, _, st = _lib.count_pairs(ctx, d, d, jobs[j:j + 1], t, want_counts=True, want_sums=True)
                assert st.variants == set(name[r])
            if devices == 0:
                ctx.set_option("slab_budget_bytes", 4096)  # one job per piece
            counts, sums, st = _lib.count_pairs(ctx, d, d, jobs, t, want_counts=True, want_sums=True)
            assert st.count_variant == st.count_variant_weighted == _lib.VARIANT_MIXED
            assert st.variants == {"mixed"}
            assert np.array_equal(counts, exp_c)
            np.testing.assert_allclose(sums, exp_s, rtol=RTOL_W, atol=0)
        finally:
            ctx.close()  # frees the catalogue first (its free reads the context)
        assert d is None or not d._h
