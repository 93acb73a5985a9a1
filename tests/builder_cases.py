"""Scenes and cases of tests/test_gpu_builder_records.py, shared with tools/make_golden_builder_windows.py (which records on
the parent commit what the strip item builder made of them): small seeded catalogues around (1, 0, 0) -- the library sorts
along z and cuts strips along y there, so a strip is a band of right ascension and the sort key is sin(dec) -- whose runs
hold what a per-run or per-tile record can get wrong.

Patches of a scene (ids are labels; every ordered pair of them is a job):
  0 .. 3  the quadrants of a uniform field of 2.0 x 1.7 degrees: runs of hundreds of objects on seven strips, the left
          quadrants on strips 0 .. 3, the right ones on 3 .. 6 -- partner strips fall outside the streamed group on either
          side (s1 < 0, s1 >= n_strips1);
  4       a ROW: objects at one declination, so every key of every run is the same double (RunGrid::inv = 0): 65, 127, 255
          objects and 1 object on the strips 1, 2, 4 and 5 -- last lane tiles of 1, 63 and 127 objects for tiles of 64 and 128,
          a run of length 1, and no object on strip 3: an empty run between two others;
  5       SINGLES: one object on each of the strips 0, 2, 3 and 6: runs of length 1 with empty runs between them.
"""
import functools

import numpy as np

from oracle import oracle

ARCMIN = np.pi / 10800
STRIP = 0.005  # strip grid spacing in rad (strip_width_micro = 5000, the library's default)
# The latitude grid (strip_grid = 1, the default) has its boundaries where latitude + pi / 2 is a multiple of the spacing: strip s
# of a scene is [ORIGIN + s STRIP, ORIGIN + (s + 1) STRIP) in right ascension. (On the linear grid, strip_grid = 0, the
# boundaries lie elsewhere and the run lengths below are not the ones named: those cases exercise the other grid, no more.)
ORIGIN = (np.ceil(0.5 * np.pi / STRIP) - 0.5 * np.pi / STRIP) * STRIP
P = 6
B = 3
ROW_COUNTS = {1: 65, 2: 127, 4: 255, 5: 1}
SINGLE_STRIPS = (0, 2, 3, 6)
ROW_DEC = 0.004

# every option a case may set, with the library's default (restored after the case)
DEFAULTS = dict(tile_r=0, triple_runs=1, band_trim=1, strip_grid=1, seg_strips_min_run=16, half_bands=1,
                strip_width_micro=5000)


def _columns(seed, n_field, nb, weighted):
    rng = np.random.default_rng(seed)
    ra = rng.uniform(ORIGIN + 0.02 * STRIP, ORIGIN + 6.98 * STRIP, n_field)
    dec = np.arcsin(rng.uniform(np.sin(-0.015), np.sin(0.015), n_field))
    patch = 2 * (ra >= ORIGIN + 3.5 * STRIP).astype(np.int64) + (dec >= 0.0)
    # the row: evenly spread over the inner 80 % of its strips, so that no object lies near a strip boundary
    row_ra = np.concatenate([ORIGIN + (s + 0.1 + 0.8 * np.arange(c) / c) * STRIP for s, c in ROW_COUNTS.items()])
    one_ra = np.array([ORIGIN + (s + 0.5) * STRIP for s in SINGLE_STRIPS])
    one_dec = np.array([-0.006 + 0.002 * i for i in range(len(SINGLE_STRIPS))])
    ra = np.concatenate([ra, row_ra, one_ra])
    dec = np.concatenate([dec, np.full(len(row_ra), ROW_DEC), one_dec])
    patch = np.concatenate([patch, np.full(len(row_ra), 4), np.full(len(one_ra), 5)])
    n = len(ra)
    z = rng.uniform(0.1, 0.9, n)
    w = rng.uniform(0.5, 1.5, n)  # (always drawn: the weighted and the unweighted scene share their positions)
    edges = np.linspace(0.1, 0.9, nb + 1) if nb > 1 else None
    cat = oracle.sort_catalog(ra, dec, z, w if weighted else None, patch, P, edges, "right")
    for a in (cat["x"], cat["y"], cat["z"], cat["w"], cat["off"]):
        if a is not None:
            a.setflags(write=False)
    return cat


@functools.lru_cache(maxsize=None)
def catalog(name, weighted):
    """"binned": 12 000 field objects in B redshift bins; "unbinned": 20 000 in one; "binned2": a second binned one."""
    seed, n, nb = {"binned": (811, 12000, B), "unbinned": (812, 20000, 1), "binned2": (813, 9000, B)}[name]
    return _columns(seed, n, nb, weighted)


ALL_PAIRS = np.array([(p, q) for p in range(P) for q in range(P)], dtype=np.int32)
UPPER_PAIRS = np.array([(p, q) for p in range(P) for q in range(p, P)], dtype=np.int32)  # as an autocorrelation lists them
LONG_INDEX = np.arange(1025) % len(ALL_PAIRS)  # 1 025 jobs: the builder's job table no longer fits its LDS copy


@functools.lru_cache(maxsize=None)
def thresholds():
    """One annulus of 1 to 10 arcmin in every bin: the largest chord, 2.9e-3, is narrower than a strip (reach 1: partner strips
    c - 1, c, c + 1, what merged triple runs need)."""
    lim = oracle.parse_ang_limits([1.0 * ARCMIN], [10.0 * ARCMIN])
    t = np.tile(oracle.thresholds_for(oracle.ang_bins_for(lim, None, None)), (B, 1))
    t.setflags(write=False)
    return t


# pairing -> (first catalogue, second catalogue, jobs); "self": the binned catalogue against itself (one device catalogue)
PAIRINGS = {
    "cross": ("binned", "unbinned", ALL_PAIRS),
    "long": ("binned", "unbinned", ALL_PAIRS[LONG_INDEX]),
    "segments": ("binned", "binned2", ALL_PAIRS),
    "self": ("binned", "binned", UPPER_PAIRS),
}


@functools.lru_cache(maxsize=None)
def expected(pairing, weighted):
    """The oracle's (counts, sums) of a pairing (brute force in float64 over every pair of every job), computed once."""
    a, b, jobs = PAIRINGS["cross" if pairing == "long" else pairing]
    counts, sums = oracle.count_jobs(catalog(a, weighted), catalog(b, weighted), jobs, thresholds())
    if pairing == "long":
        counts, sums = counts[LONG_INDEX], sums[LONG_INDEX]
    counts.setflags(write=False)
    sums.setflags(write=False)
    return counts, sums


def _case(name, pairing, weighted=False, kernel="band", mode=1, **options):
    return dict(name=name, pairing=pairing, weighted=weighted, kernel=kernel, mode=mode, options=options)


def _cases():
    out = []
    # merged triple runs (one window per item) and the strips themselves (three windows in lockstep), on every tile size
    for tile_r in (1, 2, 4):
        for triple in (0, 2):
            out.append(_case(f"tile{tile_r}_triple{triple}", "cross", tile_r=tile_r, triple_runs=triple))
    # trimmed and untrimmed windows on both strip grids
    for trim in (0, 1):
        for grid in (0, 1):
            for triple in (0, 2):
                out.append(_case(f"trim{trim}_grid{grid}_triple{triple}", "cross", band_trim=trim, strip_grid=grid, triple_runs=triple))
    # weighted: kept[] and the slab reduction see the same potential items
    for triple in (0, 2):
        out.append(_case(f"weighted_triple{triple}", "cross", weighted=True, triple_runs=triple))
    out.append(_case("sweep", "cross", kernel="sweep"))
    # per-(patch, bin) layouts, one object per lane; the self count walks half bands on its diagonal jobs
    for pairing in ("segments", "self"):
        for triple in (0, 2):
            out.append(_case(f"{pairing}_triple{triple}", pairing, mode=3, seg_strips_min_run=1, tile_r=1, triple_runs=triple))
    out.append(_case("self_weighted", "self", weighted=True, mode=3, seg_strips_min_run=1, tile_r=1, triple_runs=2))
    out.append(_case("self_whole_bands", "self", mode=3, seg_strips_min_run=1, tile_r=1, triple_runs=2, half_bands=0))
    # the job table in global memory
    for triple in (0, 2):
        out.append(_case(f"long_triple{triple}", "long", triple_runs=triple))
    return out


CASES = _cases()
CASE_NAMES = [c["name"] for c in CASES]
# what the golden file holds per case, as "<case>.<field>"
STAT_FIELDS = ("evaluated_pairs", "n_workgroups", "layout_mode", "merged_triples", "band_variant")


def run_case(ctx, case):
    """Upload the case's catalogues under its options, count once (counts and sums) and ask for the per-job work.
    -> (counts, sums, stats, job_work). The context's options are back at their defaults afterwards."""
    from yet_another_wizz_amd import _lib

    a, b, jobs = PAIRINGS[case["pairing"]]
    try:
        for key, value in case["options"].items():
            ctx.set_option(key, value)
        ctx.set_option("strip_width_micro", DEFAULTS["strip_width_micro"])

        def upload(name):
            cat = catalog(name, case["weighted"])
            return _lib.DeviceCatalog(ctx, cat["x"], cat["y"], cat["z"], cat["w"], P, cat["nb"], cat["off"])

        d1 = upload(a)
        d2 = d1 if b == a else upload(b)
        counts, sums, stats = _lib.count_pairs(ctx, d1, d2, jobs, thresholds(), kernel=case["kernel"], want_counts=True, want_sums=True)
        work = _lib.job_work(ctx, d1, d2, jobs, thresholds(), kernel=case["kernel"])
        d1.free()
        if d2 is not d1:
            d2.free()
    finally:
        for key, value in DEFAULTS.items():
            ctx.set_option(key, value)
    return counts, sums, stats, work
