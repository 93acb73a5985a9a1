"""GPU: the count paths on job lists past 1024 jobs and on many small patches, against the CPU oracle (a float64 brute force
over every pair of every job: it knows no layouts, no linkage and no job order).

What only runs at this scale: the strip item builder bisects its job table in LDS while the table has at most 1023 entries
and in global memory above (merged items: entries = jobs; per-segment items: entries = jobs x bins); lists of all P^2 pairs
of compact patches are mostly jobs without a single potential item; with patches of 0-3 objects a wave of the ingest kernels
spans dozens of patches; ``run_single`` halves a long weighted list several levels deep; and the public path links a fraction
of 150^2 patch pairs. Every test asserts through ``CountStats`` that its call ran on the path it is meant for. Unweighted
counts are equal to the oracle's, weighted sums within 1e-10 relative and exactly 0 where the oracle has 0."""
import functools

import numpy as np
import pytest

import helpers
from oracle import oracle

pytestmark = pytest.mark.gpu
RTOL_W = 1e-10
ARCMIN = np.pi / 10800
LDS_TABLE = 1024  # BUILD_PREFIX_LDS of csrc/yawhip_count_kernels.h: job tables of n + 1 <= 1024 entries are searched in LDS


@pytest.fixture(scope="module")
def ctx():
    from yet_another_wizz_amd import _lib

    c = _lib.Context(0)
    yield c
    c.close()


def _upload(ctx, cat, sort_axis=2):
    from yet_another_wizz_amd import _lib

    n_patches = (len(cat["off"]) - 1) // cat["nb"]
    return _lib.DeviceCatalog(ctx, cat["x"], cat["y"], cat["z"], cat["w"], n_patches, cat["nb"], cat["off"], sort_axis=sort_axis)


def _freeze(*arrays):
    for a in arrays:
        if a is not None:
            a.setflags(write=False)
    return arrays


def _frozen_cat(cat):
    _freeze(cat["x"], cat["y"], cat["z"], cat["w"], cat["off"])
    return cat


def _unweighted(cat):
    return dict(cat, w=None)


def _box_points(rng, n, box_deg):
    """``n`` points uniform on the sphere inside the box of ``box_deg`` degrees at ra 100, dec 30 -> (ra, dec) in degrees."""
    ra = rng.uniform(100.0, 100.0 + box_deg, n)
    dec = np.rad2deg(np.arcsin(rng.uniform(np.sin(np.deg2rad(30.0)), np.sin(np.deg2rad(30.0 + box_deg)), n)))
    return ra, dec


def _grid_cell(ra, dec, g, box_deg):
    ix = np.minimum(((ra - 100.0) / box_deg * g).astype(np.int64), g - 1)
    iy = np.minimum(((dec - 30.0) / box_deg * g).astype(np.int64), g - 1)
    return iy * g + ix


def grid_catalog(rng, n, P, nb, weighted, box_deg):
    """``n`` objects uniform in the box, the patch id the cell of a ceil(sqrt(P))^2 grid over it (cells beyond P, where P is no
    square, wrap around): compact patches, as k-means patches are, so most of the P^2 patch pairs hold no pair of objects."""
    ra, dec = _box_points(rng, n, box_deg)
    g = int(np.ceil(np.sqrt(P)))
    patch = _grid_cell(ra, dec, g, box_deg) % P
    z = rng.uniform(0.0, 1.0, n)
    w = rng.uniform(0.5, 1.5, n)  # (always drawn: the weighted and the unweighted scene share their positions)
    edges = np.linspace(0.1, 0.9, nb + 1) if nb > 1 else None
    return oracle.sort_catalog(np.deg2rad(ra), np.deg2rad(dec), z, w if weighted else None, patch, P, edges, "right")


def _per_bin_rows(ang_bins, n_bins):
    """Threshold rows that differ per redshift bin (physical scales do that), as in test_ragged_jobs_vs_oracle."""
    return np.stack([oracle.thresholds_for(ang_bins * (1.0 + 0.1 * k)) for k in range(n_bins)])


def _all_pairs(P):
    return np.array([(p, q) for p in range(P) for q in range(P)], dtype=np.int32)


def _check(counts, sums, exp_c, exp_s, weights, msg):
    """The project's tolerances: counts equal; unweighted sums equal to the counts; weighted sums 1e-10, 0 where the oracle has 0."""
    assert np.array_equal(counts, exp_c), msg
    if weights == "uu":
        assert np.array_equal(sums, exp_c.astype(np.float64)), msg
    else:
        np.testing.assert_allclose(sums, exp_s, rtol=RTOL_W, atol=0, err_msg=str(msg))
        assert not np.any(sums[exp_c == 0]), msg


# ------------------------------------------------------------------------------------------------ scene 1: 49 patches, 2401 jobs
P1, B1 = 49, 3


@functools.lru_cache(maxsize=None)
def scene1():
    rng = np.random.default_rng(20240)
    c1 = _frozen_cat(grid_catalog(rng, 30000, P1, B1, True, 4.0))
    c2 = _frozen_cat(grid_catalog(rng, 30000, P1, 1, True, 4.0))
    return c1, c2


def _scene1_cats(weights):
    c1, c2 = scene1()
    return (c1, c2) if weights == "ww" else (_unweighted(c1), _unweighted(c2))


@functools.lru_cache(maxsize=None)
def edges1(name):
    """Thresholds [B1, E] of scene 1. "two_scales": 3 edges (0.5', 2', 6'); "log13": 13 log-spaced edges from 0.5' to 6'
    (the grid ``rweight`` makes); "lin13": 13 edges uniform in angle, which the log-spaced model does not fit."""
    if name == "two_scales":
        ab = oracle.ang_bins_for(oracle.parse_ang_limits(np.array([0.5, 2.0]) * ARCMIN, np.array([2.0, 6.0]) * ARCMIN), None, None)
    elif name == "log13":
        ab = oracle.ang_bins_for(oracle.parse_ang_limits([0.5 * ARCMIN], [6.0 * ARCMIN]), -1.0, 12)
    else:
        ab = np.linspace(0.5, 6.0, 13) * ARCMIN
    t = _per_bin_rows(ab, B1)
    assert t.shape == (B1, 3 if name == "two_scales" else 13)
    return _freeze(t)[0]


@functools.lru_cache(maxsize=None)
def expected1(name):
    """The oracle's (counts, sums) of the weighted scene 1 on all 2401 ordered patch pairs; the unweighted scene has the
    same positions, hence the same counts."""
    c1, c2 = scene1()
    return _freeze(*oracle.count_jobs(c1, c2, _all_pairs(P1), edges1(name)))


@functools.lru_cache(maxsize=None)
def shuffled1():
    """The 2401 jobs in a fixed random order with jobs that hold pairs moved to the list positions 1019 ... 1026, on both
    sides of the last position (1023) of the longest list whose table the builder searches in LDS -> (order, live)."""
    live_of = expected1("two_scales")[0].any(axis=(1, 2))
    order = np.random.default_rng(7).permutation(P1 * P1)
    for pos in range(LDS_TABLE - 5, LDS_TABLE + 3):
        if not live_of[order[pos]]:
            swap = next(i for i in range(1100, len(order)) if live_of[order[i]])
            order[[pos, swap]] = order[[swap, pos]]
    return _freeze(order, live_of[order])


BAND_CASES = [("band", "two_scales", 32), ("band", "log13", 33), ("band", "lin13", 64), ("sweep", "two_scales", 0),
              ("filter", "two_scales", 0), ("exact", "two_scales", 0)]


@pytest.mark.parametrize("weights", ["uu", "ww"])
@pytest.mark.parametrize("kernel,edges,variant", BAND_CASES)
def test_merged_items_past_1024_jobs(ctx, kernel, edges, variant, weights):
    """1. Binned x unbinned on merged items (layout mode 1) with all 49^2 = 2401 ordered patch pairs as the job list: the
    builder's job table has 2402 entries and is bisected in global memory; six jobs in seven have no potential item, so the
    prefix search runs across long flat stretches. The band kernels of all three variants, the sweep kernel and the two
    brute-force kernels (which enumerate (job, bin) slots, most of them live) against the oracle."""
    from yet_another_wizz_amd import _lib

    c1, c2 = _scene1_cats(weights)
    jobs, t = _all_pairs(P1), edges1(edges)
    exp_c, exp_s = expected1(edges)
    live = exp_c.any(axis=(1, 2))
    assert (~live).sum() > 2000 and live.sum() > 300  # mostly jobs without pairs, and enough with
    d1, d2 = _upload(ctx, c1), _upload(ctx, c2)
    # The float32 band kernel streams the three partner strips of an item here (the plan expects merged windows of ~700 entries,
    # beyond its stage) and, with ``triple_runs`` = 2, their merged triple runs: the job records then point into the V + 2 G
    # triples of the G = 49 groups.
    try:
        for triple_runs in (1, 2) if variant == 32 else (1,):
            ctx.set_option("triple_runs", triple_runs)
            counts, sums, st = _lib.count_pairs(ctx, d1, d2, jobs, t, kernel=kernel, want_counts=True, want_sums=True)
            assert st.kernel_used == _lib.KERNEL_IDS[kernel]
            if kernel in ("band", "sweep"):
                assert st.layout_mode == 1 and st.n_orientations >= 1
            else:
                assert st.layout_mode == 0
            assert st.band_variant == variant
            if variant == 32:
                assert st.merged_triples == (1 if triple_runs == 2 else 0)
            _check(counts, sums, exp_c, exp_s, weights, (kernel, edges, triple_runs))
    finally:
        ctx.set_option("triple_runs", 1)


@pytest.mark.parametrize("weights", ["uu", "ww"])
@pytest.mark.parametrize("kernel", ["band", "sweep"])
def test_both_sides_of_the_lds_job_table(ctx, kernel, weights):
    """2. Prefixes of 1022, 1023 (job table in LDS), 1024 and 1025 jobs (global memory) of the shuffled list: every row is
    the oracle's row of that job, and the rows two prefixes share are the same bits, counts and sums."""
    from yet_another_wizz_amd import _lib

    c1, c2 = _scene1_cats(weights)
    t = edges1("two_scales")
    exp_c, exp_s = expected1("two_scales")
    order, live = shuffled1()
    assert live[:LDS_TABLE - 2].sum() > 100 and live[LDS_TABLE - 5:LDS_TABLE + 1].all()  # pairs on both sides of position 1023
    jobs = _all_pairs(P1)[order]
    d1, d2 = _upload(ctx, c1), _upload(ctx, c2)
    got = {}
    for n in (LDS_TABLE - 2, LDS_TABLE - 1, LDS_TABLE, LDS_TABLE + 1):
        counts, sums, st = _lib.count_pairs(ctx, d1, d2, jobs[:n], t, kernel=kernel, want_counts=True, want_sums=True)
        assert st.kernel_used == _lib.KERNEL_IDS[kernel] and st.layout_mode == 1
        _check(counts, sums, exp_c[order[:n]], exp_s[order[:n]], weights, (kernel, n))
        got[n] = (counts, sums)
    for n in (LDS_TABLE - 1, LDS_TABLE, LDS_TABLE + 1):
        m = n - 1
        assert np.array_equal(got[n][0][:m], got[m][0]), (kernel, n)
        assert np.array_equal(got[n][1][:m], got[m][1]), (kernel, n)  # bit for bit, weighted too


# ------------------------------------------------------------------------------------------------ scene 3: per-segment items
P3, B3 = 16, 8


@functools.lru_cache(maxsize=None)
def scene3():
    rng = np.random.default_rng(20243)
    c1 = _frozen_cat(grid_catalog(rng, 40000, P3, B3, True, 3.0))
    c2 = _frozen_cat(grid_catalog(rng, 40000, P3, B3, True, 3.0))
    ab = oracle.ang_bins_for(oracle.parse_ang_limits(np.array([0.5, 2.0]) * ARCMIN, np.array([2.0, 6.0]) * ARCMIN), None, None)
    t = _freeze(_per_bin_rows(ab, B3))[0]
    # the self count's list: the 136 jobs with p <= q, then the 120 with p > q
    self_jobs = np.array([(p, q) for p in range(P3) for q in range(p, P3)] + [(p, q) for p in range(P3) for q in range(p)],
                         dtype=np.int32)
    return c1, c2, t, _freeze(self_jobs)[0]


@functools.lru_cache(maxsize=None)
def expected3(kind):
    c1, c2, t, self_jobs = scene3()
    if kind == "cross":
        return _freeze(*oracle.count_jobs(c1, c2, _all_pairs(P3), t))
    return _freeze(*oracle.count_jobs(c2, c2, self_jobs, t))


@functools.lru_cache(maxsize=None)
def shuffled3():
    """The 256 cross jobs in a fixed random order with live jobs at the positions 124 ... 129: lists of 127, 128 and 129
    jobs make 1016, 1024 and 1032 pseudo jobs (job, bin)."""
    live_of = expected3("cross")[0].any(axis=(1, 2))
    order = np.random.default_rng(8).permutation(P3 * P3)
    for pos in range(124, 130):
        if not live_of[order[pos]]:
            swap = next(i for i in range(140, len(order)) if live_of[order[i]])
            order[[pos, swap]] = order[[swap, pos]]
    return _freeze(order, live_of[order])


def _segment_options(ctx, seg_strips):
    ctx.set_option("seg_strips_min_run", 1)
    ctx.set_option("seg_strips", seg_strips)


def _restore_segment_options(ctx):
    ctx.set_option("seg_strips_min_run", 16)
    ctx.set_option("seg_strips", 1)


@pytest.mark.parametrize("weights", ["uu", "ww"])
@pytest.mark.parametrize("kernel", ["band", "sweep"])
def test_segment_items_past_1024_pseudo_jobs(ctx, kernel, weights):
    """3. Binned x binned on the per-(patch, bin) strip layouts (layout mode 3; forced with ``seg_strips_min_run`` = 1): the
    builder's table has one pseudo job per (job, bin), 256 x 8 = 2048 of them. The cross count on all 256 ordered patch pairs
    and the self count of one catalogue on its p <= q jobs followed by the p > q ones (the diagonal jobs walk half bands where
    the plan allows), against the oracle and against the ordinary (job, bin) items of ``seg_strips`` = 0."""
    from yet_another_wizz_amd import _lib

    c1, c2, t, self_jobs = scene3()
    if weights == "uu":
        c1, c2 = _unweighted(c1), _unweighted(c2)
    try:
        _segment_options(ctx, 1)
        d1, d2 = _upload(ctx, c1), _upload(ctx, c2)
        for kind, da, db, jobs in (("cross", d1, d2, _all_pairs(P3)), ("self", d2, d2, self_jobs)):
            exp_c, exp_s = expected3(kind)
            assert exp_c.sum() > 100000 and 50 < exp_c.any(axis=(1, 2)).sum() < 200  # live and dead jobs, both many
            ctx.set_option("seg_strips", 1)
            counts, sums, st = _lib.count_pairs(ctx, da, db, jobs, t, kernel=kernel, want_counts=True, want_sums=True)
            assert st.kernel_used == _lib.KERNEL_IDS[kernel] and st.layout_mode == 3, kind
            assert len(jobs) * B3 > LDS_TABLE
            _check(counts, sums, exp_c, exp_s, weights, (kernel, kind))
            ctx.set_option("seg_strips", 0)
            counts0, sums0, st0 = _lib.count_pairs(ctx, da, db, jobs, t, kernel=kernel, want_counts=True, want_sums=True)
            assert st0.layout_mode == 0, kind
            assert np.array_equal(counts0, counts), (kernel, kind)
            np.testing.assert_allclose(sums0, sums, rtol=RTOL_W, atol=0)
    finally:
        _restore_segment_options(ctx)


@pytest.mark.parametrize("weights", ["uu", "ww"])
@pytest.mark.parametrize("kernel", ["band", "sweep"])
def test_both_sides_of_the_lds_table_of_pseudo_jobs(ctx, kernel, weights):
    """3, threshold: lists of 127 (1016 pseudo jobs: table in LDS), 128 and 129 jobs (1024 and 1032: global memory) of the
    shuffled cross list on layout mode 3; rows equal the oracle's and are the same bits in every list."""
    from yet_another_wizz_amd import _lib

    c1, c2, t, _ = scene3()
    if weights == "uu":
        c1, c2 = _unweighted(c1), _unweighted(c2)
    exp_c, exp_s = expected3("cross")
    order, live = shuffled3()
    assert live[:124].sum() > 20 and live[124:130].all()
    jobs = _all_pairs(P3)[order]
    try:
        _segment_options(ctx, 1)
        d1, d2 = _upload(ctx, c1), _upload(ctx, c2)
        got = {}
        for n in (127, 128, 129):
            assert (n * B3 + 1 <= LDS_TABLE) == (n == 127)
            counts, sums, st = _lib.count_pairs(ctx, d1, d2, jobs[:n], t, kernel=kernel, want_counts=True, want_sums=True)
            assert st.kernel_used == _lib.KERNEL_IDS[kernel] and st.layout_mode == 3
            _check(counts, sums, exp_c[order[:n]], exp_s[order[:n]], weights, (kernel, n))
            got[n] = (counts, sums)
        for n in (128, 129):
            assert np.array_equal(got[n][0][:n - 1], got[n - 1][0]) and np.array_equal(got[n][1][:n - 1], got[n - 1][1]), (kernel, n)
    finally:
        _restore_segment_options(ctx)


# ------------------------------------------------------------------------------------------------ 4: the list is only a list
@pytest.mark.parametrize("weights", ["uu", "ww"])
@pytest.mark.parametrize("kernel", ["band", "sweep"])
def test_the_job_list_is_only_a_list(ctx, kernel, weights):
    """4. The shuffled 2401 jobs plus 50 of them repeated at random positions: the rows of a repeated job are the same bits,
    and counting ``jobs[perm]`` gives ``counts[perm]`` and ``sums[perm]`` bit for bit -- each slot's slabs are reduced in the
    order of its own potential items, whatever the order of the jobs. ``job_work`` of the list adds up to the evaluated
    pairs of the sweep call."""
    from yet_another_wizz_amd import _lib

    c1, c2 = _scene1_cats(weights)
    t = edges1("two_scales")
    exp_c, exp_s = expected1("two_scales")
    order, live = shuffled1()
    rng = np.random.default_rng(44)
    repeated = np.concatenate([rng.choice(np.flatnonzero(live), 40, replace=False), rng.choice(np.flatnonzero(~live), 10, replace=False)])
    index = order.copy()
    for r in repeated:
        index = np.insert(index, rng.integers(0, len(index) + 1), order[r])
    assert len(index) == P1 * P1 + 50
    jobs = _all_pairs(P1)[index]
    d1, d2 = _upload(ctx, c1), _upload(ctx, c2)
    counts, sums, st = _lib.count_pairs(ctx, d1, d2, jobs, t, kernel=kernel, want_counts=True, want_sums=True)
    assert st.kernel_used == _lib.KERNEL_IDS[kernel] and st.layout_mode == 1
    _check(counts, sums, exp_c[index], exp_s[index], weights, kernel)
    n_twice = 0
    for r in repeated:
        rows = np.flatnonzero(index == order[r])
        assert len(rows) >= 2
        for other in rows[1:]:
            assert np.array_equal(counts[rows[0]], counts[other]) and np.array_equal(sums[rows[0]], sums[other]), (kernel, order[r])
        n_twice += counts[rows[0]].sum() > 0
    assert n_twice >= 40
    perm = rng.permutation(len(jobs))
    counts_p, sums_p, st_p = _lib.count_pairs(ctx, d1, d2, jobs[perm], t, kernel=kernel, want_counts=True, want_sums=True)
    assert st_p.layout_mode == 1
    assert np.array_equal(counts_p, counts[perm]), kernel
    assert np.array_equal(sums_p, sums[perm]), kernel  # bit for bit, weighted too
    assert st_p.candidate_pairs == st.candidate_pairs
    if kernel == "sweep":
        work = _lib.job_work(ctx, d1, d2, jobs, t, kernel="sweep")
        # (a weighted call that also returns counts runs the kernel twice)
        assert work.sum() * (2 if weights == "ww" else 1) == st.evaluated_pairs == st_p.evaluated_pairs
        assert np.array_equal(work[perm], _lib.job_work(ctx, d1, d2, jobs[perm], t, kernel="sweep"))
        assert np.all(work[exp_c[index].any(axis=(1, 2))] > 0)  # a job with pairs has evaluated some


# ------------------------------------------------------------------------------------------------ 5: a long list cut in pieces
# slab_budget_bytes per kernel: a fraction of what the whole list's slabs take, so that run_single halves the list five levels
# deep, into 32 pieces of 75 jobs. Observed n_launches, uncut -> cut: band 6 -> 192 (the list is first cut between 262144 and
# 131072 bytes, and is down to single jobs below 4096), sweep 6 -> 192 (first cut at 262144), filter 6 -> 192 (first cut at
# 262144; (job, bin) items on the plain layout).
SLAB_BUDGETS = {"band": 8192, "sweep": 16384, "filter": 16384}


@pytest.mark.parametrize("kernel", ["band", "sweep", "filter"])
def test_long_weighted_list_cut_in_pieces(ctx, kernel):
    """5. The weighted scene 1 on all 2401 jobs with a slab budget far below the list's slabs: ``run_single`` halves the list
    recursively into dozens of pieces of dozens of jobs (``test_weighted_slab_budget_splits_the_job_list`` cuts 36 jobs down to
    single ones). Same bits as the uncut call, and the statistics add up."""
    from yet_another_wizz_amd import _lib

    c1, c2 = _scene1_cats("ww")
    jobs, t = _all_pairs(P1), edges1("two_scales")
    exp_c, exp_s = expected1("two_scales")
    d1, d2 = _upload(ctx, c1), _upload(ctx, c2)
    counts0, sums0, st0 = _lib.count_pairs(ctx, d1, d2, jobs, t, kernel=kernel, want_counts=True, want_sums=True)
    _check(counts0, sums0, exp_c, exp_s, "ww", kernel)
    try:
        ctx.set_option("slab_budget_bytes", SLAB_BUDGETS[kernel])
        counts1, sums1, st1 = _lib.count_pairs(ctx, d1, d2, jobs, t, kernel=kernel, want_counts=True, want_sums=True)
    finally:
        ctx.set_option("slab_budget_bytes", 1 << 30)
    print(f"{kernel}: n_launches {st0.n_launches} -> {st1.n_launches}")
    assert st0.kernel_used == st1.kernel_used == _lib.KERNEL_IDS[kernel]
    assert st0.layout_mode == st1.layout_mode == (0 if kernel == "filter" else 1)
    assert st1.n_launches >= 16 * st0.n_launches          # several levels deep ...
    assert st1.n_launches <= len(jobs) // 8 * st0.n_launches  # ... and far from single jobs
    assert np.array_equal(counts1, counts0) and np.array_equal(sums1, sums0)
    assert st1.candidate_pairs == st0.candidate_pairs and st1.evaluated_pairs == st0.evaluated_pairs


# ------------------------------------------------------------------------------------------------ 6: hundreds of patches, most tiny
P6, B6, N_BIG, N_TINY, LONG_RUN = 300, 3, 100, 200, 30


@functools.lru_cache(maxsize=None)
def tiny_patch_ids():
    """Patch ids of scene 6: the 100 grid cells and 200 tiny patches interleaved in id order -- one tiny patch in front of every
    big one, a second behind seventy of them, and one run of 30 tiny patches in the middle -> (ids of the cells, ids of the
    tiny patches)."""
    kinds = []  # True: grid cell
    for b in range(N_BIG):
        kinds += [False, True] + ([False] if b < 70 else [])
        if b == 50:
            kinds += [False] * LONG_RUN
    kinds = np.array(kinds)
    assert len(kinds) == P6 and kinds.sum() == N_BIG
    return _freeze(np.flatnonzero(kinds), np.flatnonzero(~kinds))


def tiny_patch_catalog(rng, n, nb, weighted):
    """About ``n`` objects in a 6-degree box: the bulk in the 10 x 10 grid cells, and 0, 1, 2 or 3 objects (60, 60, 40 and 40
    times) anywhere in the box for each of the 200 tiny patches."""
    big_ids, tiny_ids = tiny_patch_ids()
    sizes = rng.permutation(np.repeat([0, 1, 2, 3], [60, 60, 40, 40]))
    ra, dec = _box_points(rng, n, 6.0)
    patch = big_ids[_grid_cell(ra, dec, 10, 6.0)]
    patch[:sizes.sum()] = np.repeat(tiny_ids, sizes)  # (the first objects drawn, wherever they lie)
    z = rng.uniform(0.0, 1.0, n)
    if nb > 1:
        z[:sizes.sum()] = rng.uniform(0.15, 0.85, sizes.sum())  # the tiny patches keep their objects: inside the binning
    w = rng.uniform(0.5, 1.5, n)
    edges = np.linspace(0.1, 0.9, nb + 1) if nb > 1 else None
    return oracle.sort_catalog(np.deg2rad(ra), np.deg2rad(dec), z, w if weighted else None, patch, P6, edges, "right"), sizes


@functools.lru_cache(maxsize=None)
def scene6():
    rng = np.random.default_rng(20246)
    c1, sizes1 = tiny_patch_catalog(rng, 20000, B6, True)
    c2, sizes2 = tiny_patch_catalog(rng, 20000, 1, True)
    ab = oracle.ang_bins_for(oracle.parse_ang_limits(np.array([0.5, 2.0]) * ARCMIN, np.array([2.0, 6.0]) * ARCMIN), None, None)
    t = _freeze(_per_bin_rows(ab, B6))[0]
    self_jobs = np.array([(p, q) for p in range(P6) for q in range(p, P6)], dtype=np.int32)
    return _frozen_cat(c1), _frozen_cat(c2), t, _freeze(self_jobs)[0], _freeze(sizes1, sizes2)


@functools.lru_cache(maxsize=None)
def expected6(kind):
    c1, c2, t, self_jobs, _ = scene6()
    if kind == "cross":
        return _freeze(*oracle.count_jobs(c1, c2, _all_pairs(P6), t))
    return _freeze(*oracle.count_jobs(c1, c1, self_jobs, t))


def _longest_sparse_run(per_patch):
    """Most consecutive patch ids that hold fewer than 64 objects together (one wave of an ingest kernel spans them all)."""
    best = lo = total = 0
    for hi, n in enumerate(per_patch):
        total += n
        while total >= 64:
            total -= per_patch[lo]
            lo += 1
        best = max(best, hi - lo + 1)
    return best


def _segment_sums_reference(cat):
    """Per (patch, bin) sum of the weights in float64 (``np.add.reduceat`` reads empty segments wrongly: sliced sums)."""
    off = cat["off"]
    return np.array([cat["w"][a:b].sum() for a, b in zip(off[:-1], off[1:])]).reshape(-1, cat["nb"])


@pytest.mark.parametrize("sort_axis", [0, 1, 2])
def test_hundreds_of_patches_most_of_them_tiny(ctx, sort_axis):
    """6. 300 patches of which 200 hold 0 to 3 objects, interleaved with 100 grid cells in id order: a wave of ``k_strip_index``,
    ``k_patch_boxes``, ``k_run_of`` and ``k_gather_bins`` spans dozens of patches with empty ones between occupied ones (the
    per-lane atomics instead of the wave reduction), the segmented sort gets 900 segments most of which are empty or one object
    long, and the triple runs are laid out for 300 groups. All 90 000 ordered patch pairs against the unbinned catalogue, the
    binned catalogue against itself on its 45 150 p <= q jobs, and the segment sums of the upload."""
    from yet_another_wizz_amd import _lib

    c1w, c2w, t, self_jobs, (sizes1, sizes2) = scene6()
    per_patch = np.diff(c1w["off"][::B6])
    big_ids, tiny_ids = tiny_patch_ids()
    assert (sizes1 == 0).sum() >= 50 and (sizes1 == 1).sum() >= 50 and np.array_equal(per_patch[tiny_ids], sizes1)
    assert np.array_equal(np.diff(c2w["off"])[tiny_ids], sizes2) and per_patch[big_ids].min() > 64
    assert _longest_sparse_run(per_patch) > 20
    assert np.diff(big_ids).min() >= 2 and tiny_ids[0] < big_ids[0]  # interleaved: a tiny patch between any two big ones
    jobs = _all_pairs(P6)
    exp_c, exp_s = expected6("cross")
    exp_self_c, exp_self_s = expected6("self")
    live = exp_c.any(axis=(1, 2))
    tiny_job = np.isin(jobs[:, 0], tiny_ids) | np.isin(jobs[:, 1], tiny_ids)
    assert exp_c.sum() > 100000 and (live & tiny_job).sum() > 100 and live.sum() < 0.05 * len(jobs)
    for weights in ("uu", "ww"):
        c1, c2 = (c1w, c2w) if weights == "ww" else (_unweighted(c1w), _unweighted(c2w))
        d1, d2 = _upload(ctx, c1, sort_axis), _upload(ctx, c2, sort_axis)
        # the upload's own per-segment sums
        seg = d1.segment_sums()
        if weights == "ww":
            ref = _segment_sums_reference(c1)
            np.testing.assert_allclose(seg, ref, rtol=1e-13, atol=0)
            assert not np.any(seg[np.diff(c1["off"]).reshape(P6, B6) == 0])
        else:
            assert np.array_equal(seg, np.diff(c1["off"]).reshape(P6, B6).astype(np.float64))
        try:
            # (band, 2: the streamed side in merged triple runs, V + 2 G of them for the G = 300 groups, two per empty group)
            for kernel, triple_runs in (("band", 1), ("band", 2), ("sweep", 1)):
                ctx.set_option("triple_runs", triple_runs)
                counts, sums, st = _lib.count_pairs(ctx, d1, d2, jobs, t, kernel=kernel, want_counts=True, want_sums=True)
                assert st.kernel_used == _lib.KERNEL_IDS[kernel] and st.layout_mode == 1 and st.n_orientations >= 1, (kernel, sort_axis)
                if kernel == "band":
                    assert st.band_variant == 32 and (triple_runs == 1 or st.merged_triples == 1)
                _check(counts, sums, exp_c, exp_s, weights, (kernel, triple_runs, weights, sort_axis))
        finally:
            ctx.set_option("triple_runs", 1)
        for kernel in ("band", "sweep", "exact"):  # binned x binned, default options
            counts, sums, st = _lib.count_pairs(ctx, d1, d1, self_jobs, t, kernel=kernel, want_counts=True, want_sums=True)
            assert st.kernel_used == _lib.KERNEL_IDS[kernel], (kernel, sort_axis)
            # a dozen objects per (patch, bin, strip) run: the default options keep the ordinary (job, bin) items of the base
            # layout, whose 900 segments the upload sorted; the band request runs the float64 band kernel on them
            assert st.layout_mode == 0 and st.band_variant == (64 if kernel == "band" else 0), (kernel, sort_axis)
            _check(counts, sums, exp_self_c, exp_self_s, weights, ("self", kernel, weights, sort_axis))


# ------------------------------------------------------------------------------------------------ 7: the public path at 150 patches
P7, B7 = 150, 4


@functools.lru_cache(maxsize=None)
def scene7(weighted):
    """Columns of the four catalogues in a 12 x 12 degree box, patch ids the cells of a 15 x 10 grid."""
    rng = np.random.default_rng(20247)

    def frame(n, with_z):
        ra = rng.uniform(40.0, 52.0, n)
        dec = np.rad2deg(np.arcsin(rng.uniform(np.sin(np.deg2rad(-6.0)), np.sin(np.deg2rad(6.0)), n)))
        ix = np.minimum(((ra - 40.0) / 12.0 * 15).astype(np.int64), 14)
        iy = np.minimum(((dec + 6.0) / 12.0 * 10).astype(np.int64), 9)
        d = {"ra": ra, "dec": dec, "patch": iy * 15 + ix, "w": rng.uniform(0.3, 2.0, n)}
        if with_z:
            d["z"] = rng.uniform(0.1, 1.0, n)  # some objects fall outside the binning
        if not weighted:
            del d["w"]
        _freeze(*d.values())
        return d

    return dict(ref=frame(40000, True), unk=frame(50000, False), rand=frame(50000, False), ref_rand=frame(40000, True))


def _config7():
    import yet_another_wizz_amd as yaw

    return yaw.Configuration.create(rmin=[1, 3], rmax=[3, 10], unit="arcmin", zmin=0.2, zmax=0.9, num_bins=B7)


@functools.lru_cache(maxsize=None)
def expected7(weighted, name1, name2):
    """``oracle.count_pairs`` of two catalogues of scene 7 on ALL patch pairs -- every ordered pair, or every p <= q for a
    catalogue against itself (the pairs an autocorrelation lists; the x 0.5 on its diagonal is the oracle's ``auto``) --
    from the same columns, the configuration's bin edges and ``closed``."""
    frames, config = scene7(weighted), _config7()
    edges, closed = np.asarray(config.binning.edges), str(config.binning.closed)

    def ocat(f):
        return oracle.sort_catalog(np.deg2rad(f["ra"]), np.deg2rad(f["dec"]), f.get("z"), f.get("w"), f["patch"], P7,
                                   edges if "z" in f else None, closed)

    auto = name1 == name2
    jobs = np.array([(p, q) for p in range(P7) for q in range(p if auto else 0, P7)], dtype=np.int32)
    lo = np.tile(np.array([1.0, 3.0]) * ARCMIN, (B7, 1))
    hi = np.tile(np.array([3.0, 10.0]) * ARCMIN, (B7, 1))
    return _freeze(*oracle.count_pairs(ocat(frames[name1]), ocat(frames[name2]), jobs, lo, hi, P7, auto=auto))


def _catalogs7(weighted):
    import yet_another_wizz_amd as yaw

    kw = dict(ra_name="ra", dec_name="dec", patch_name="patch", weight_name="w" if weighted else None)
    return {name: yaw.Catalog.from_dataframe(None, f, redshift_name="z" if "z" in f else None, **kw)
            for name, f in scene7(weighted).items()}


def _check_counts7(weighted, cfs, sides, msg):
    """Every count of the correlation functions (one per scale) against the oracle's [S, B, P, P] tensor."""
    for kind, (name1, name2) in sides.items():
        exp, sw1, sw2 = expected7(weighted, name1, name2)
        assert exp.sum() > 10000
        for s, cf in enumerate(cfs):
            got = getattr(cf, kind)
            assert got is not None, (msg, kind)
            dev = got.counts.counts
            assert dev.shape == (B7, P7, P7)
            assert not np.any(exp[s][dev == 0]), \
                f"{msg} {kind} scale {s}: the oracle, which knows no linkage, counts pairs in a slot the device left empty: a dropped link"
            if weighted:
                np.testing.assert_allclose(dev, exp[s], rtol=RTOL_W, atol=0, err_msg=f"{msg} {kind} scale {s}")
                np.testing.assert_allclose(got.sum_weights.sum_weights1, sw1, rtol=1e-13, atol=0)
                np.testing.assert_allclose(got.sum_weights.sum_weights2, sw2, rtol=1e-13, atol=0)
            else:
                assert np.array_equal(dev, exp[s]), (msg, kind, s)
                assert np.array_equal(got.sum_weights.sum_weights1, sw1) and np.array_equal(got.sum_weights.sum_weights2, sw2)


def _check_samples7(dev, ora):
    for cd, co in zip(dev, ora):
        sd, so = cd.sample(), co.sample()
        assert np.all(np.isfinite(sd.data[np.isfinite(so.data)])) and np.isfinite(so.data).sum() >= B7 - 1
        np.testing.assert_allclose(sd.data, so.data, rtol=1e-12, atol=1e-14, equal_nan=True)
        np.testing.assert_allclose(sd.samples, so.samples, rtol=1e-12, atol=1e-14, equal_nan=True)


def _partial_linkage(config, *cats):
    import yet_another_wizz_amd as yaw

    links = yaw.PatchLinkage.from_catalogs(config, *cats)
    assert 0.02 < links.density < 0.5, links
    return links


@pytest.mark.parametrize("weighted", [False, True])
def test_crosscorrelate_at_150_patches_vs_oracle_without_linkage(weighted, monkeypatch):
    """7. ``crosscorrelate`` on the device with 150 given patches -- linkage, job table, the dense call and its scatter into
    [S, B, P, P] -- against the oracle on all 22 500 patch pairs: a linked pair the host dropped would leave a slot empty that the
    oracle fills. The API tests otherwise compare with an engine that shares the linkage."""
    import yet_another_wizz_amd as yaw
    from yet_another_wizz_amd import _lib

    config, cats = _config7(), _catalogs7(weighted)
    try:
        dev = yaw.crosscorrelate(config, cats["ref"], cats["unk"], unk_rand=cats["rand"])
        links = _partial_linkage(config, cats["ref"], cats["unk"], cats["rand"])
        assert len(links.get_patch_pairs(cats["ref"], cats["unk"])) > LDS_TABLE
        links.count_pairs(cats["ref"], cats["unk"])
        st = links.last_stats
        assert st.kernel_used == _lib.KERNEL_BAND and st.layout_mode == 1 and st.band_variant == 32 and st.n_orientations >= 1
        _check_counts7(weighted, dev, dict(dd=("ref", "unk"), dr=("ref", "rand")), "cross")
        helpers.use_oracle_engine(monkeypatch)
        ora = yaw.crosscorrelate(config, cats["ref"], cats["unk"], unk_rand=cats["rand"])
        _check_samples7(dev, ora)
    finally:
        for cat in cats.values():
            cat.drop_layouts()


@pytest.mark.parametrize("weighted", [False, True])
def test_autocorrelate_at_150_patches_vs_oracle_without_linkage(weighted, monkeypatch):
    """7. ``autocorrelate`` (DD and RR on the p <= q pairs with halved diagonal, DR on ordered pairs) the same way."""
    import yet_another_wizz_amd as yaw
    from yet_another_wizz_amd import _lib

    config, cats = _config7(), _catalogs7(weighted)
    try:
        dev = yaw.autocorrelate(config, cats["ref"], cats["ref_rand"])
        links = _partial_linkage(config, cats["ref"], cats["ref_rand"])
        links.count_pairs(cats["ref"])
        st = links.last_stats
        # (binned x binned at ~10 objects per (patch, bin, strip) run: the ordinary (job, bin) items, on which AUTO sweeps)
        assert st.kernel_used == _lib.KERNEL_SWEEP and st.layout_mode == 0
        _check_counts7(weighted, dev, dict(dd=("ref", "ref"), dr=("ref", "ref_rand"), rr=("ref_rand", "ref_rand")), "auto")
        for cf in dev:  # an autocorrelation fills the upper triangle only
            assert not np.any(np.tril(cf.dd.counts.counts, -1)) and not np.any(np.tril(cf.rr.counts.counts, -1))
        helpers.use_oracle_engine(monkeypatch)
        ora = yaw.autocorrelate(config, cats["ref"], cats["ref_rand"])
        _check_samples7(dev, ora)
    finally:
        for cat in cats.values():
            cat.drop_layouts()
