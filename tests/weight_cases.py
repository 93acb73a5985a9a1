"""Weight columns for the catalogues of the count-variant table, and the two rules their sums are held to (no GPU needed).

The table of tests/test_gpu_count_variants.py reaches every compiled count kernel, with positive weights over six decades and a
relative tolerance. The scalar-field correlations send ``kappa * w`` -- both signs -- through the same weighted kernels, and a
weighted launch may have one side without weights. Here the table's catalogues ``c1``, ``c2u`` and ``c2b`` keep their positions,
segment order and offsets and get other weight columns:

``dyadic``     ``w = m / 16`` with integer ``m`` in [-64, 64], about 1 % of the objects exactly 0.0. Every product of two such
               weights is a multiple of 2^-8 of magnitude at most 16, so while the sum of the magnitudes of a slot stays below
               2^45 (2^-8 x 2^53) every partial sum of every subset of the slot's products is a float64 number: the sum is exact
               in any order -- per-lane cumulative accumulators and their differences, LDS atomics, the reductions over chunks
               and slots, the C oracle. Every kernel must give the oracle's sums BIT FOR BIT, signed or not (``check_exact``).
``none``       no weight column (``w = None``): with ``dyadic`` on the other side a weighted launch with one unweighted side
               (placements ``wu`` and ``uw``; products are multiples of 2^-4 then).
``real``       ``normal(0, 1) * 10 ** uniform(-3, 3)``: signed, six decades, not exactly summable. Held to the rule of
               DESIGN.md section 11 (``check_signed``): 1e-10 of the slot's cancellation-free magnitude.

``reference`` is the oracle's result per (pair, grid, placement), computed once per process and shared by
tests/test_weight_cases.py (which checks, on the oracle alone, the conditions the argument above needs) and
tests/test_gpu_weighted_exact.py."""
from __future__ import annotations

import functools

import numpy as np

from oracle import oracle
from test_gpu_count_variants import CASES, JOBS, PAIRS, _catalogues, thresholds

SEEDS = {"dyadic": 20261020, "real": 20261021, "permuted": 20261022}
NAMES = ("c1", "c2u", "c2b")
# placement -> weighting of the first and of the second catalogue
PLACEMENTS = {"ww": ("dyadic", "dyadic"), "wu": ("dyadic", "none"), "uw": ("none", "dyadic"), "real": ("real", "real")}
DYADIC = ("ww", "wu", "uw")
EXACT_LIMIT = 2.0 ** 40   # sum of magnitudes of a slot: a margin of 2^5 to the 2^45 at which exactness would end
RTOL_SIGNED = 1e-10
KEYS = sorted({(c.pair, c.grid) for c in CASES})  # every (pair, grid) a case of the table counts


def placements(pair: str) -> tuple:
    """The placements of a pair: a self count is one handle against itself and keeps ``ww``."""
    return ("ww", "real") if pair == "self" else ("ww", "wu", "uw", "real")


def _dyadic(rng, n):
    m = rng.integers(-64, 65, n)
    m[rng.random(n) < 0.01] = 0
    return m / 16.0


def _real(rng, n):
    return rng.normal(0.0, 1.0, n) * 10.0 ** rng.uniform(-3.0, 3.0, n)


@functools.lru_cache(maxsize=None)
def _columns(weighting: str) -> dict:
    """One weight column per catalogue, in the row order of ``_catalogues()``."""
    rng = np.random.default_rng(SEEDS[weighting])
    draw = {"dyadic": _dyadic, "real": _real}[weighting]
    return {name: draw(rng, len(_catalogues()[0][name]["x"])) for name in NAMES}


@functools.lru_cache(maxsize=None)
def catalogues(weighting: str, magnitude: bool = False) -> dict:
    """The table's three catalogues under a weighting (``magnitude``: with ``|w|``). Only ``w`` differs from the table's."""
    out = {}
    for name in NAMES:
        cat = dict(_catalogues()[0][name])
        if weighting == "none":
            cat["w"] = None
        else:
            w = _columns(weighting)[name]
            cat["w"] = np.abs(w) if magnitude else w.copy()
            cat["w"].setflags(write=False)
        out[name] = cat
    return out


@functools.lru_cache(maxsize=None)
def permuted(weighting: str) -> dict:
    """The catalogues of a weighting with the rows of every (patch, bin) segment permuted: the same slots hold the same
    pairs, the oracle adds them in another order."""
    rng = np.random.default_rng(SEEDS["permuted"])
    out = {}
    for name, cat in catalogues(weighting).items():
        off = cat["off"]
        order = np.concatenate([off[s] + rng.permutation(off[s + 1] - off[s]) for s in range(len(off) - 1)])
        out[name] = {**cat, **{k: cat[k][order] for k in ("x", "y", "z", "w")}}
    return out


@functools.lru_cache(maxsize=None)
def reference(pair: str, grid: str, placement: str, magnitude: bool = False, threads=None, rows: str = "table"):
    """Oracle (counts, sums) of a table input under a placement, computed once. ``magnitude``: with ``|w|`` on both sides (the
    cancellation-free sum of every slot); ``rows="permuted"``: the rows of every segment in another order."""
    a, b = PAIRS[pair]
    first, second = PLACEMENTS[placement]
    if rows == "permuted":
        assert first == second and not magnitude
        cats = permuted(first)
        c1, c2 = cats[a], cats[b]
    else:
        c1, c2 = catalogues(first, magnitude)[a], catalogues(second, magnitude)[b]
    counts, sums = oracle.count_jobs(c1, c2, JOBS, thresholds(grid), threads=threads)
    counts.setflags(write=False)
    sums.setflags(write=False)
    return counts, sums


# --------------------------------------------------------------------------------------------------------------- the rules
def check_exact(key, got, exp_sums, exp_counts) -> None:
    """Exactly summable weights: the oracle's sums bit for bit; a slot in which the oracle counts no pair is +0.0."""
    assert got.shape == exp_sums.shape == exp_counts.shape, key
    if not np.array_equal(got, exp_sums):
        bad = np.argwhere(got != exp_sums)
        at = tuple(int(i) for i in bad[0])
        raise AssertionError(f"{key}: {len(bad)} of {got.size} slots differ from the exact sum, first at {at}: "
                             f"{float(got[at])!r} != {float(exp_sums[at])!r} ({int(exp_counts[at])} pairs)")
    assert not np.any(np.signbit(got[exp_counts == 0])), key


def check_signed(key, got, exp, mag) -> float:
    """``|got - exp| <= 1e-10 * mag`` in every slot, ``mag`` the oracle's sum of the same slot with
    ``|w|`` on both sides; exactly 0 where ``mag == 0``. Prints and returns the worst ``|got - exp| / mag``."""
    assert got.shape == exp.shape == mag.shape, key
    err = np.abs(got - exp)
    worst = float(np.max(err / np.where(mag > 0, mag, 1.0)))
    print(f"{key}: worst |ours - oracle| / abs = {worst:.3e} over {np.count_nonzero(mag)} slots")
    assert np.all(err <= RTOL_SIGNED * mag), (key, worst)
    assert np.all(got[mag == 0] == 0.0), key
    return worst
