"""The conditions under which tests/test_gpu_weighted_exact.py means something, on the CPU oracle alone (no GPU needed).

For every (pair, grid) a case of the count-variant table counts, and every placement of the weights:

* dyadic columns (``ww``, ``wu``, ``uw``): every oracle sum is a multiple of 2^-8, the cancellation-free magnitude of every
  slot stays below 2^40 -- a factor 2^5 under the 2^45 at which a sum of multiples of 2^-8 stops being exact in float64 -- and
  the oracle gives the same bits with one thread and with its default. The oracle's weighted sums are then exact, and so must
  be those of every kernel;
* slots of both signs in every input, and slots that hold pairs whose sum is exactly 0.0 somewhere in the table;
* the ``real`` columns cancel (some slot is below 1 % of its magnitude), and the oracle's own dependence on the order of its
  additions -- the rows of every segment permuted -- is at most 1e-12 of the magnitude, a hundredth of the 1e-10 the GPU result
  is held to (measured: 2.2e-15);
* the fresh columns leave positions, segment order and offsets of the table's catalogues untouched, so every case still
  reaches the variants it names."""
import numpy as np
import pytest

import test_gpu_count_variants as table
import weight_cases as wc

KEY_IDS = [f"{pair}-{grid}" for pair, grid in wc.KEYS]


def test_columns_are_what_they_claim():
    base = table._catalogues()[0]
    for weighting in ("dyadic", "none", "real"):
        for magnitude in (False, True):
            cats = wc.catalogues(weighting, magnitude)
            assert set(cats) == set(base) == set(wc.NAMES)
            for name, cat in cats.items():
                for k in ("x", "y", "z", "off"):
                    assert np.array_equal(cat[k], base[name][k]), (weighting, name, k)
                assert cat["nb"] == base[name]["nb"]
                assert (cat["w"] is None) == (weighting == "none")
                assert cat["w"] is None or (len(cat["w"]) == len(cat["x"]) and np.all(np.isfinite(cat["w"])))
                assert not (magnitude and cat["w"] is not None and np.any(cat["w"] < 0))
    for name, w in wc._columns("dyadic").items():
        m = w * 16.0
        assert np.array_equal(m, np.round(m)) and m.min() == -64 and m.max() == 64, name
        assert 0.005 < np.mean(w == 0.0) < 0.03 and np.mean(w < 0) > 0.4 and np.mean(w > 0) > 0.4, name
    for name, w in wc._columns("real").items():
        a = np.abs(w[w != 0])
        assert np.mean(w < 0) > 0.4 and np.mean(w > 0) > 0.4 and a.max() / a.min() > 1e6, name
    # the catalogues of a permutation hold the same segments
    for name, cat in wc.permuted("real").items():
        ref = wc.catalogues("real")[name]
        assert np.array_equal(cat["off"], ref["off"]) and not np.array_equal(cat["w"], ref["w"])
        for s in range(len(ref["off"]) - 1):
            lo, hi = ref["off"][s], ref["off"][s + 1]
            assert np.array_equal(np.sort(cat["w"][lo:hi]), np.sort(ref["w"][lo:hi])), (name, s)


def test_keys_cover_the_table():
    assert set(wc.KEYS) == {(c.pair, c.grid) for c in table.CASES}
    assert {c.pair for c in table.CASES} == set(table.PAIRS)
    for pair in table.PAIRS:
        assert wc.placements(pair) == (("ww", "real") if pair == "self" else ("ww", "wu", "uw", "real"))


@pytest.mark.parametrize("key", wc.KEYS, ids=KEY_IDS)
def test_dyadic_sums_are_exact_in_the_oracle(key):
    pair, grid = key
    for placement in wc.placements(pair):
        if placement not in wc.DYADIC:
            continue
        counts, sums = wc.reference(pair, grid, placement)
        where = (pair, grid, placement)
        assert counts.sum() > 10000 and np.count_nonzero(counts == 0) > 0, where  # real pairs, and empty slots
        assert np.array_equal(sums * 256.0, np.round(sums * 256.0)), where
        mag = wc.reference(pair, grid, placement, magnitude=True)[1]
        assert np.all(np.abs(sums) <= mag) and mag.max() < wc.EXACT_LIMIT, (where, mag.max())
        print(f"{where}: largest cancellation-free slot sum {mag.max():.4g} = 2^{np.log2(mag.max()):.1f}")
        assert np.all(sums[counts == 0] == 0.0) and not np.any(np.signbit(sums[counts == 0])), where
        one = wc.reference(pair, grid, placement, threads=1)
        assert np.array_equal(one[0], counts) and np.array_equal(one[1], sums), where
        assert np.any(sums < 0) and np.any(sums > 0), where  # slots of both signs
        # the counts do not depend on the weights: those of the table
        assert np.array_equal(counts, wc.reference(pair, grid, "real")[0]), where


def test_some_slot_holds_pairs_that_sum_to_zero():
    n = 0
    for pair, grid in wc.KEYS:
        for placement in wc.placements(pair):
            if placement in wc.DYADIC:
                counts, sums = wc.reference(pair, grid, placement)
                n += np.count_nonzero((counts > 0) & (sums == 0.0))
    print(f"{n} slots hold pairs whose signed sum is exactly 0")
    assert n > 0


@pytest.mark.parametrize("key", wc.KEYS, ids=KEY_IDS)
def test_real_weights_cancel_and_the_reference_is_far_below_the_rule(key):
    pair, grid = key
    counts, exp = wc.reference(pair, grid, "real")
    mag = wc.reference(pair, grid, "real", magnitude=True)[1]
    assert np.any(exp < 0) and np.any(exp > 0) and np.all(np.abs(exp) <= mag), key
    assert np.all((mag > 0) == (counts > 0)), key
    ratio = np.abs(exp[mag > 0]) / mag[mag > 0]
    assert ratio.min() < 1e-2, (key, ratio.min())  # the cancellation is real
    c_perm, s_perm = wc.reference(pair, grid, "real", rows="permuted")
    assert np.array_equal(c_perm, counts), key
    order = float(np.max(np.abs(s_perm - exp)[mag > 0] / mag[mag > 0]))
    print(f"{key}: strongest cancellation {ratio.min():.2e}, order dependence of the oracle {order:.2e} of the magnitude")
    assert np.all(np.abs(s_perm - exp) <= 1e-12 * mag), (key, order)


def test_the_rules_reject_what_they_should():
    counts = np.array([[3, 0], [1, 2]])
    exp = np.array([[0.25, 0.0], [-1.5, 0.0]])
    wc.check_exact("ok", exp.copy(), exp, counts)
    with pytest.raises(AssertionError):
        wc.check_exact("one ulp", np.nextafter(exp, 1.0), exp, counts)
    with pytest.raises(AssertionError):
        wc.check_exact("minus zero in an empty slot", np.array([[0.25, -0.0], [-1.5, 0.0]]), exp, counts)
    mag = np.array([[1.0, 0.0], [2.0, 4.0]])
    assert wc.check_signed("ok", exp + 0.5e-10 * mag, exp, mag) <= 1e-10
    with pytest.raises(AssertionError):
        wc.check_signed("beyond the rule", exp + 2e-10 * mag, exp, mag)
    with pytest.raises(AssertionError):
        wc.check_signed("no magnitude, no error", exp + np.array([[0.0, 1e-300], [0.0, 0.0]]), exp, mag)
