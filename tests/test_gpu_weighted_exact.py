"""The weighted launch of every reachable count-kernel variant: exact sums for signed and one-sided weights.

The table of tests/test_gpu_count_variants.py takes its bit-exact counts from the unweighted instantiation of a variant and
holds the weighted one -- another kernel, with its own guard-band lines and its own flush -- to 1e-10 relative on positive
weights over six decades: a pair in the wrong bin, a dropped lane or a sentinel counted with a small weight can hide in that,
and for a signed slot that cancels a relative tolerance on the sum means nothing. Here every case of the table runs again on
the weight columns of tests/weight_cases.py (same positions, so the same variants):

``ww``         signed dyadic weights on both sides (the "kk" shape of the scalar-field correlations). Every float64 sum of
               their products is exact in any order (tests/test_weight_cases.py checks the conditions on the oracle), so counts
               AND sums must equal the oracle's bit for bit, from the call that returns both and from the call that returns the
               sums alone -- k_count with one histogram shared by four waves included: exact sums have no order.
``wu``, ``uw`` the dyadic column on one side, no weights on the other: the weighted launch that fills the missing side with
               1.0 (staged weights of the band kernels, the lane objects' own weight, the ``c1.w`` / ``c2.w`` tests of k_count and
               k_count_merged; with swapped sides the roles change). The planner looks at the weights of a count only through
               "one side has some", so the variant is the one the case names. Bit for bit.
``real``       signed weights over six decades, not exactly summable: every slot within 1e-10 of its cancellation-free
               magnitude, the same bits on a repeat (k_count with one shared histogram: the rule again).

The float32 cases must still send the engineered partners to the exact predicate in the weighted launch."""
from __future__ import annotations

import numpy as np
import pytest

import weight_cases as wc
from test_gpu_count_variants import (B, CASES, ENTRY_CASES, JOBS, PAIRS, _apply, _dense_of, _Device, _restore, thresholds)

pytestmark = pytest.mark.gpu
WEIGHTINGS = ("dyadic", "none", "real")


def _all_catalogues() -> dict:
    """The table's three catalogues under each weighting, by "<name>/<weighting>"."""
    return {f"{name}/{weighting}": cat for weighting in WEIGHTINGS for name, cat in wc.catalogues(weighting).items()}


def _sides(d, pair: str, placement: str):
    a, b = PAIRS[pair]
    first, second = wc.PLACEMENTS[placement]
    return d.dev[f"{a}/{first}"], d.dev[f"{b}/{second}"]


@pytest.fixture(scope="module")
def device():
    d = _Device(0, _all_catalogues())
    yield d
    d.close()


def _shared_histogram(case) -> bool:
    """k_count<..., PRIV = false, ...>: four waves add into one histogram in the order they arrive."""
    return case.reach[1].startswith("k_count<") and ", false, " in case.reach[1]


def _run_case(d, case):
    from yet_another_wizz_amd import _lib

    t = thresholds(case.grid)
    try:
        _apply(d.ctx, {"seg_strips_min_run": 1, **case.options})  # as the table applies them
        for extra in ({}, *case.alt):
            _apply(d.ctx, extra)
            # ---- signed dyadic weights on both sides
            key = f"{case.id} {extra} ww"
            exp_c, exp_s = wc.reference(case.pair, case.grid, "ww")
            c1, c2 = _sides(d, case.pair, "ww")
            counts, sums, st = _lib.count_pairs(d.ctx, c1, c2, JOBS, t, want_counts=True, want_sums=True)
            assert st.variants == set(case.reach), (key, st.variants)
            assert np.array_equal(counts, exp_c), key
            wc.check_exact(key, sums, exp_s, exp_c)
            _, sums2, st2 = _lib.count_pairs(d.ctx, c1, c2, JOBS, t, want_counts=False, want_sums=True)
            assert st2.variants == {case.reach[1]}, (key, st2.variants)
            wc.check_exact(key + " (sums alone)", sums2, exp_s, exp_c)
            if case.reevaluates:  # the guard-band lines of the weighted instantiation
                assert st.exact_reevaluations > 0 and st2.exact_reevaluations > 0, key
            # ---- one side without weights
            for placement in wc.placements(case.pair):
                if placement not in ("wu", "uw"):
                    continue
                key = f"{case.id} {extra} {placement}"
                exp_c, exp_s = wc.reference(case.pair, case.grid, placement)
                c1, c2 = _sides(d, case.pair, placement)
                assert c1.weighted != c2.weighted
                _, sums, st = _lib.count_pairs(d.ctx, c1, c2, JOBS, t, want_counts=False, want_sums=True)
                assert st.variants == {case.reach[1]}, (key, st.variants)
                wc.check_exact(key, sums, exp_s, exp_c)
                if case.reevaluates:
                    assert st.exact_reevaluations > 0, key
            # ---- signed weights over six decades
            key = f"{case.id} {extra} real"
            exp_s = wc.reference(case.pair, case.grid, "real")[1]
            mag = wc.reference(case.pair, case.grid, "real", magnitude=True)[1]
            c1, c2 = _sides(d, case.pair, "real")
            _, sums, st = _lib.count_pairs(d.ctx, c1, c2, JOBS, t, want_counts=False, want_sums=True)
            assert st.variants == {case.reach[1]}, (key, st.variants)
            wc.check_signed(key, sums, exp_s, mag)
            _, sums2, _ = _lib.count_pairs(d.ctx, c1, c2, JOBS, t, want_counts=False, want_sums=True)
            if _shared_histogram(case):
                wc.check_signed(key + " (repeat)", sums2, exp_s, mag)
            else:
                assert np.array_equal(sums2, sums), key
    finally:
        _restore(d.ctx)


@pytest.mark.parametrize("case", CASES, ids=[c.id for c in CASES])
def test_weighted_variant_is_exact(device, case):
    _run_case(device, case)


def test_dense_batch_is_exact(device):
    """yawhip_count_pairs_dense_batch, one scale over all fine bins and no separation weights: the per-scale sums and the
    scatter are exact on dyadic sums, so both requests give the dense tensor of the oracle's sums bit for bit."""
    from yet_another_wizz_amd import _lib

    for case in ENTRY_CASES:
        t = thresholds(case.grid)
        slices = np.tile(np.array([[0, t.shape[1] - 1]], dtype=np.int32), (B, 1, 1))
        c1, c2 = _sides(device, case.pair, "ww")
        try:
            _apply(device.ctx, {"seg_strips_min_run": 1, **case.options})
            out = _lib.count_pairs_dense_batch(device.ctx, [(c1, c2, JOBS, False), (c1, c2, JOBS[::-1].copy(), False)], t, slices, None)
        finally:
            _restore(device.ctx)
        want = _dense_of(wc.reference(case.pair, case.grid, "ww")[1])
        for dense, st in out:
            assert st.count_variant == 0 and st.variants == {case.reach[1]}, case.id
            assert np.array_equal(dense, want), case.id


def test_three_streams_give_the_bits_of_one(device):
    """A context of three streams on one device splits the job list: the same variants and the same (exact) bits."""
    from yet_another_wizz_amd import _lib

    cats = {key: cat for key, cat in _all_catalogues().items() if key.endswith("/dyadic")}
    d = _Device([0, 0, 0], cats)
    try:
        for case in ENTRY_CASES:
            t = thresholds(case.grid)
            results = []
            for dev in (d, device):
                try:
                    _apply(dev.ctx, {"seg_strips_min_run": 1, **case.options})
                    results.append(_lib.count_pairs(dev.ctx, *_sides(dev, case.pair, "ww"), JOBS, t, want_counts=True, want_sums=True))
                finally:
                    _restore(dev.ctx)
            (counts, sums, st), (counts1, sums1, st1) = results
            assert st.variants == st1.variants == set(case.reach), (case.id, st.variants)
            exp_c, exp_s = wc.reference(case.pair, case.grid, "ww")
            assert np.array_equal(counts, exp_c) and np.array_equal(counts, counts1), case.id
            wc.check_exact(case.id, sums, exp_s, exp_c)
            assert np.array_equal(sums, sums1), case.id
    finally:
        d.close()
