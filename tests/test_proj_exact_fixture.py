"""CPU: the exact reference of the two projected counts, tests/golden/proj_exact.npz (tools/make_golden_proj_exact.py: mpmath,
``R2 = ((d_a + d_b) / 2)^2 (2 asin(chord / 2))^2`` against the radius edges and ``p = |c_a - c_b|`` against the cut and the pi
edges, no series), and the mirror oracles of the contract (tests/proj_oracle.py, tests/proj_pi_oracle.py) against it. The
conditions the tool asserts are asserted again from the stored arrays, without mpmath: they say that no pair is left out of
any comparison and that the file tells a kernel that bins by another quantity from a right one -- shown here on three wrong
variants of the oracle. The kernels meet the same file in tests/test_gpu_proj_exact.py."""
import functools
import os
import sys

import numpy as np
import pytest

import proj_exact as pe
import proj_oracle as oracle
import proj_pi_oracle as pi_oracle
import proj_scenes
from conftest import ROOT

ARCSEC = np.pi / 180.0 / 3600.0
DEG = np.pi / 180.0
EDGE_MARGIN = {"as": 1e-6, "wide": 1e-9}
N_SITES = {"as": 5, "wide": 4}
PER_SEGMENT = {"as": 14, "wide": 20}
CASES = [(name, fold, two) for name in pe.SCENES for fold in (False, True) for two in (False, True)]
IDS = [f"{name}-{'nb=1' if fold else 'nb=2'}-{'two' if two else 'one'}" for name, fold, two in CASES]


def handles(fx, name, fold, two, weighted):
    a = pe.scene(fx, name, "a", fold, weighted)
    return a, (pe.scene(fx, name, "b", fold, weighted) if two else a)


@functools.lru_cache(maxsize=None)
def oracle_planes(name, fold, two):
    """The mirror oracles' weighted ``W`` and every ``W_pi`` of a case: computed once, shared, never modified."""
    fx = pe.fixture()
    a, b = handles(fx, name, fold, two, True)
    cells, r2 = pe.cells(fx, name, fold, two), fx[f"{name}.r2"]
    out = {None: oracle.proj_cells(a, b, cells, r2, float(fx["pmax"]))[:2]}
    for edges in pe.PI_SETS:
        out[edges] = pi_oracle.proj_pi_cells(a, b, cells, r2, fx[f"pi.{edges}"])[:2]
    for planes in out.values():
        for arr in planes:
            arr.setflags(write=False)
    return out


def bins_of(R2, rows):
    """The fine bin of ``R2`` in its row ``f64[n, E]``, -1 outside."""
    e = (R2[:, None] > rows).sum(axis=1) - 1
    return np.where((R2 > rows[:, 0]) & (R2 <= rows[:, -1]), e, -1)


def every_pair(fx, name, two):
    """``(first, second, i, j, row)`` of every pair of the cells of a site as uploaded, in the tool's order of a pair: of one handle the
    object with the larger index comes first."""
    first, second = handles(fx, name, False, two, False)
    i_all, j_all, row_all = [], [], []
    for sa, sb, row, diagonal in pe.cells(fx, name, False, two)[:-2]:  # (the last two: between sites)
        i, j = np.meshgrid(np.arange(first["off"][sa], first["off"][sa + 1]), np.arange(second["off"][sb], second["off"][sb + 1]), indexing="ij")
        keep = (i > j) if diagonal else np.ones(i.shape, dtype=bool)
        i, j = i[keep], j[keep]
        if not two:
            i, j = np.maximum(i, j), np.minimum(i, j)
        i_all.append(i), j_all.append(j), row_all.append(np.full(len(i), row))
    return first, second, np.concatenate(i_all), np.concatenate(j_all), np.concatenate(row_all)


def sentinel_floats(fx, listed):
    """``(s2, theta2, DD, p)`` of sentinel records ``(two, i, j, ...)`` in float64."""
    a, b = handles(fx, "wide", False, True, False)
    out = np.empty((4, len(listed)))
    for two in (0, 1):
        rows = listed[:, 0] == two
        out[:, rows] = pe.pair_floats(a, b if two else a, listed[rows, 1], listed[rows, 2])
    return out


def test_the_file_and_its_pi_edges():
    fx = pe.fixture()
    assert os.path.getsize(os.path.join(ROOT, "tests", "golden", "proj_exact.npz")) < 300 * 1024
    pmax = float(fx["pmax"])
    assert pmax == 40.0 and fx["eps"] == pe.EPS
    assert np.array_equal(fx["pi.one"], [0.0, pmax]) and np.array_equal(fx["pi.four"], np.linspace(0.0, pmax, 5))
    uneven = fx["pi.uneven"]
    assert len(uneven) - 1 >= 8 and uneven[0] == 0.0 and 0.0 < uneven[1] < 1e-3 and uneven[-1] == pmax and np.all(np.diff(uneven) > 0)
    assert np.diff(uneven).min() < 1e-3 * pmax
    # every plane of the uneven set holds a pair in some scene
    held = sum(pe.counts_pi(fx, name, False, two, "uneven").sum(axis=(1, 2)) for name in pe.SCENES for two in (False, True))
    print(f"pairs per plane of the uneven set: {held.astype(int)}")
    assert np.all(held > 0)
    assert 1.0 <= fx["K"] <= 64.0 and fx["K"] >= 4.0 * fx["K_measured"] and fx["K_measured"] <= 10.0
    assert np.log2(float(fx["K"])) % 1.0 == 0.0 and fx["K"] < 8.0 * fx["K_measured"]
    keys = {f"{p}.{plane}" for name, fold, two in CASES for p in [pe.prefix(name, fold, two)]
            for plane in ["N", "W", "A"] + [f"{kind}.{edges}" for kind in ("N_pi", "W_pi") for edges in pe.PI_SETS]}
    assert keys <= set(fx.files) and not any("pair" in key for key in fx.files)  # per-pair records: the sentinels only


@pytest.mark.parametrize("name", pe.SCENES)
def test_the_fixture_is_what_the_issue_asks_for(name):
    fx = pe.fixture()
    r2, n_sites, pmax = fx[f"{name}.r2"], int(fx[f"{name}.n_sites"]), float(fx["pmax"])
    assert n_sites == N_SITES[name] and r2.shape == (2, 7) and np.all(np.diff(r2, axis=1) > 0)
    ratio = r2[:, 1:] / r2[:, :-1]
    np.testing.assert_allclose(ratio, ratio[:, :1] * np.ones(6), rtol=1e-12)  # log-spaced
    for cat in "ab":
        off, w = fx[f"{name}.{cat}.off"], fx[f"{name}.{cat}.w"]
        assert len(off) == 4 * n_sites + 1 and np.all(np.diff(off) == PER_SEGMENT[name]) and np.all(w > 0)
    margin, pi_margin = np.inf, np.inf
    for fold in (False, True):
        nb = 1 if fold else 2
        for two in (False, True):
            cells = pe.cells(fx, name, fold, two)
            base = (proj_scenes.cells_two_handles if two else proj_scenes.cells_one_handle)(nb, n_sites)
            assert np.array_equal(cells, pe.cell_lists(n_sites, fold, two)) and len(cells) == len(base) * (2 if fold else 1) + 2
            assert np.array_equal(cells[:len(base)], base) and len(np.unique(cells, axis=0)) == len(cells)
            site = lambda seg: seg // (2 * nb)  # noqa: E731
            assert np.all(site(cells[:-2, 0]) == site(cells[:-2, 1])) and np.all(site(cells[-2:, 0]) != site(cells[-2:, 1]))
            N = pe.counts(fx, name, fold, two)
            assert N.shape == (len(cells), 6) and np.all(N == np.rint(N)) and N.sum() > 1000
            assert not np.any(N[-2:]) and np.all(N[:-2].sum(axis=1) > 0)  # the cells between sites hold nothing, every other some
            W, A = pe.expected(fx, name, fold, two)
            assert np.array_equal(W, A) and np.array_equal(A > 0, N > 0)  # (every weight is > 0)
            for edges in pe.PI_SETS:
                N_pi = pe.counts_pi(fx, name, fold, two, edges)
                assert N_pi.shape == (len(fx[f"pi.{edges}"]) - 1, len(cells), 6) and np.all(N_pi == np.rint(N_pi))
                assert np.array_equal(N_pi.sum(axis=0), N)  # the planes sum to N as integers
                W_pi = pe.expected(fx, name, fold, two, edges)[0]
                assert np.array_equal(W_pi > 0, N_pi > 0)
                np.testing.assert_allclose(W_pi.sum(axis=0), W, rtol=1e-14, atol=0)
            assert np.array_equal(pe.counts_pi(fx, name, fold, two, "one")[0], N)
            if fold:  # the margins again in float64 from all pairs and both rows (1e-6 / 1e-9 against errors of 1e-10 / 1e-13)
                a, b = handles(fx, name, fold, two, False)
                margin = min(margin, oracle.nearest_margin(a, b, cells[:-2], r2, pmax)[0])
                pi_margin = min([pi_margin] + [pi_oracle.nearest_pi_margin(a, b, cells[:-2], fx[f"pi.{edges}"])[0] for edges in pe.PI_SETS])
                assert N.sum() > 1.3 * pe.counts(fx, name, False, two).sum()  # folded, a pair is binned by both rows and across bins
    assert margin >= EDGE_MARGIN[name] and fx[f"{name}.margin"] >= EDGE_MARGIN[name] and margin == pytest.approx(float(fx[f"{name}.margin"]), rel=1e-3)
    assert pi_margin >= 1e-9 and fx[f"{name}.pi_margin"] >= 1e-9 and pi_margin == pytest.approx(float(fx[f"{name}.pi_margin"]), rel=1e-3)
    # the stored counts are those of float64 arcsin, and D follows the pair: d_a alone moves a quarter of the member pairs
    n_member, n_moved = 0, 0
    for two in (False, True):
        first, second, i, j, row = every_pair(fx, name, two)
        s2, theta2, DD, p = pe.pair_floats(first, second, i, j)
        e = bins_of(DD * theta2, r2[row])
        member = (e >= 0) & (p <= pmax)
        assert member.sum() == pe.counts(fx, name, False, two).sum()
        n_member += member.sum()
        n_moved += np.count_nonzero(bins_of(first["d"][i] ** 2 * theta2, r2[row])[member] != e[member])
    assert n_moved / n_member >= 0.25 and n_moved / n_member == pytest.approx(float(fx[f"{name}.moved"]), abs=0.002)
    print(f"{name}: {n_member} member pairs, nearest radius edge {fx[f'{name}.margin']:.2e} away, nearest edge in p {fx[f'{name}.pi_margin']:.2e}, "
          f"d_a alone moves {n_moved / n_member:.3f} of them; drawn {int(fx[f'{name}.draws'])} times")


def test_the_arcsecond_scene():
    fx = pe.fixture()
    for cat in "ab":
        h = pe.scene(fx, "as", cat)
        dec = np.rad2deg(fx[f"as.{cat}.dec"])
        for site in (0.0, 60.0, 89.99, -89.99):
            assert np.any(np.abs(dec - site) < 1e-2)
        ra = fx[f"as.{cat}.ra"][h["off"][16]:]  # the site at the wrap: objects on both sides of it
        assert min(np.sum(ra < 1.0), np.sum(ra > 5.0)) >= 10
        assert 600.0 <= h["d"].min() < 700.0 and 2400.0 < h["d"].max() <= 2500.0 and 0.0 <= h["c"].min() and h["c"].max() <= 120.5
        for axis in "xyz":  # neighbours in any sort order differ widely in d
            for lo, hi in zip(h["off"][:-1], h["off"][1:]):
                d = h["d"][lo:hi][np.argsort(h[axis][lo:hi], kind="stable")]
                assert np.max(np.maximum(d[1:] / d[:-1], d[:-1] / d[1:])) > 1.5
        ratios = [h["d"][lo:hi].max() / h["d"][lo:hi].min() for lo, hi in zip(h["off"][:-1], h["off"][1:])]
        assert max(ratios) > 3.5 and min(ratios) > 1.8
    first, second, i, j, _ = every_pair(fx, "as", True)
    s2, theta2, _, _ = pe.pair_floats(first, second, i, j)
    assert np.sqrt(theta2.max()) < 61.0 * ARCSEC and 0.0 < np.sqrt(theta2.min())
    assert fx["as.outside"].shape == (5, 2, 2) and np.all(fx["as.outside"] > 0)  # both end edges of both rows cut through the pairs of every site


def test_the_wide_scene_and_its_sentinels():
    fx = pe.fixture()
    r2, pmax = fx["wide.r2"], float(fx["pmax"])
    for cat in "ab":
        h = pe.scene(fx, "wide", cat)
        ra, dec, off = fx[f"wide.{cat}.ra"], np.rad2deg(fx[f"wide.{cat}.dec"]), h["off"]
        for site in (0.0, 60.0, 86.0):
            assert np.any(np.abs(dec - site) < 0.2)
        pole, wrap = slice(off[8], off[12]), slice(off[12], off[16])
        assert np.any(np.cos(ra[pole] - 3.3) < 0.0)  # a ring over the pole
        assert min(np.sum(ra[wrap] < 1.0), np.sum(ra[wrap] > 5.0)) >= 10
        for k in range(2):  # a few near objects within 2 % of the bin's least d, the others 1.3 to 4 times farther
            d = np.concatenate([h["d"][off[s]:off[s + 1]] for s in range(k, 16, 2)])
            near = d <= 1.02 * d.min()
            assert 0.0095 < r2[k, -1] / d.min() ** 2 < 0.00999 and 4 <= near.sum() <= 80
            assert np.all(d[~near] >= 1.3 * d.min() * (1.0 - 1e-12)) and np.all(d <= 4.0 * 1.02 * d.min())
    # the call is accepted AT the cap, per row and folded, one handle and two, by the library's own rule
    for fold in (False, True):
        for two in (False, True):
            a, b = handles(fx, "wide", fold, two, False)
            smax = oracle.reach(a, b, pe.cells(fx, "wide", fold, two), r2)
            assert np.all((smax > 0.0095) & (smax <= pe.S2_CAP)), smax
    first, second, i, j, _ = every_pair(fx, "wide", True)
    s2, theta2, _, _ = pe.pair_floats(first, second, i, j)
    assert np.sqrt(theta2.max()) > 5.73 * DEG and np.count_nonzero(s2 > 0.003) > 1000
    # the sentinels, again in float64 (they sit half a term from their edge: 1e-8 at the least)
    for key, wrong in (("by_chord", lambda s: s), ("by_cut", lambda s: s * (1.0 + s / 12.0))):
        listed = fx[f"wide.{key}"]
        s2, theta2, DD, p = sentinel_floats(fx, listed)
        rows = r2[listed[:, 3]]
        assert len(listed) >= 8 and np.all(p <= pmax) and np.all(listed[:, 4] >= 0)
        assert np.all(bins_of(DD * theta2, rows) == listed[:, 4]) and np.all(bins_of(DD * wrong(s2), rows) == listed[:, 5])
        assert np.all(listed[:, 4] != listed[:, 5]) and np.count_nonzero(s2 >= 0.002) >= 8  # ... at wide angles
        assert min(np.sum(listed[:, 0] == 0), np.sum(listed[:, 0] == 1)) >= 4  # of one handle and of two
    beyond = fx["wide.not_capped"]
    s2, theta2, DD, p = sentinel_floats(fx, beyond)
    last = r2[beyond[:, 3], -1]
    assert np.all(DD * s2 <= last) and np.all(DD * theta2 > last) and np.array_equal(p <= pmax, beyond[:, 4] == 1)
    for inside in (0, 1):
        for two in (0, 1):
            assert np.all(np.bincount(beyond[(beyond[:, 4] == inside) & (beyond[:, 0] == two), 3], minlength=2) >= 2)
        assert np.all(np.bincount(beyond[beyond[:, 4] == inside, 3], minlength=2) >= 4)
    assert np.all(np.bincount(beyond[:, 3], minlength=2) >= 8)
    print(f"wide: {len(fx['wide.by_chord'])} by chord, {len(fx['wide.by_cut'])} by cut, not capped per row {np.bincount(beyond[:, 3])}")


@pytest.mark.parametrize("name,fold,two", CASES, ids=IDS)
def test_the_mirror_oracles_hold_the_file(name, fold, two):
    """``N`` and every ``N_pi`` exactly (unit weights); ``|oracle - exact| <= K 2^-53 A`` per element of ``W`` and every ``W_pi``."""
    fx = pe.fixture()
    a, b = handles(fx, name, fold, two, False)
    cells, r2, K = pe.cells(fx, name, fold, two), fx[f"{name}.r2"], float(fx["K"])
    W, A, N = oracle.proj_cells(a, b, cells, r2, float(fx["pmax"]))
    assert np.array_equal(N, pe.counts(fx, name, fold, two)) and np.array_equal(W, N) and np.array_equal(A, N)
    for edges in pe.PI_SETS:
        W, _, N = pi_oracle.proj_pi_cells(a, b, cells, r2, fx[f"pi.{edges}"])
        assert np.array_equal(N, pe.counts_pi(fx, name, fold, two, edges)) and np.array_equal(W, N)
    worst = 0.0
    for edges, (W, A) in oracle_planes(name, fold, two).items():
        exp_w, exp_a = pe.expected(fx, name, fold, two, edges)
        np.testing.assert_allclose(A, exp_a, rtol=1e-12, atol=0)  # the oracle's A is the file's
        worst = max(worst, pe.check(f"{pe.prefix(name, fold, two)} {edges or 'single'}", W, exp_w, exp_a, K))
    assert worst <= float(fx["K_measured"])


def test_the_worst_ratio_is_the_one_k_was_made_from():
    fx = pe.fixture()
    worst = 0.0
    for name, fold, two in CASES:
        for edges, (W, _) in oracle_planes(name, fold, two).items():
            worst = max(worst, pe.worst_ratio(W, *pe.expected(fx, name, fold, two, edges)))
    assert worst == pytest.approx(float(fx["K_measured"]), rel=1e-12)


def d_a_alone(a, b, i, j):
    """``proj_oracle.pair_terms`` with the pair's ``D`` replaced by the ``d`` of its first object."""
    dx, dy, dz = b["x"][j] - a["x"][i], b["y"][j] - a["y"][i], b["z"][j] - a["z"][i]
    R2 = (a["d"][i] * a["d"][i]) * oracle.squared_angle((dx * dx + dy * dy) + dz * dz)
    return R2 + 0.0 * b["d"][j], np.abs(b["c"][j] - a["c"][i]), 1.0


@pytest.mark.parametrize("variant", ["the chord", "cut after s2 / 12", "D = d_a"])
def test_a_wrong_oracle_fails_the_counts(variant, monkeypatch):
    """The fixture bites: an oracle that bins by ``DD s2``, by a series without its ``s2^2 / 90``, or by the distance of one end
    counts other pairs than ``N`` on ``wide`` -- the first two in the cells of the sentinels at the least -- and the first two
    still count the same pairs on ``as``, where the terms are 1e-8 and less: that is what the two scenes are for."""
    fx = pe.fixture()
    if variant == "D = d_a":
        monkeypatch.setattr(oracle, "pair_terms", d_a_alone)
        monkeypatch.setattr(pi_oracle, "pair_terms", d_a_alone)
    else:
        wrong = {"the chord": lambda s2: np.asarray(s2, dtype=np.float64) * 1.0, "cut after s2 / 12": lambda s2: s2 * (1.0 + s2 * (1.0 / 12.0))}[variant]
        monkeypatch.setattr(oracle, "squared_angle", wrong)
    for name in ("wide", "as"):
        for fold in (False, True):
            for two in (False, True):
                a, b = handles(fx, name, fold, two, False)
                cells, r2 = pe.cells(fx, name, fold, two), fx[f"{name}.r2"]
                N = oracle.proj_cells(a, b, cells, r2, float(fx["pmax"]))[2]
                N_pi = pi_oracle.proj_pi_cells(a, b, cells, r2, fx["pi.uneven"])[2]
                differ = np.abs(N - pe.counts(fx, name, fold, two)).sum()
                if name == "as" and variant != "D = d_a":
                    assert differ == 0 and np.array_equal(N_pi, pe.counts_pi(fx, name, fold, two, "uneven"))
                    continue
                print(f"{variant}, {name} {'folded' if fold else 'two bins'} {'two handles' if two else 'one handle'}: {differ:.0f} pairs counted elsewhere")
                assert differ >= 8 and not np.array_equal(N, pe.counts(fx, name, fold, two))
                assert not np.array_equal(N_pi, pe.counts_pi(fx, name, fold, two, "uneven"))


def test_every_sentinel_is_the_tools():
    """The stored sentinels derived again with the tool's functions: radius bin, wrong bin and the side of the cut."""
    pytest.importorskip("mpmath")
    from mpmath import mpf

    sys.path.insert(0, os.path.join(ROOT, "tools"))
    try:
        import make_golden_proj_exact as tool
    finally:
        sys.path.pop(0)
    fx = pe.fixture()
    for name in pe.SCENES:
        assert np.array_equal(fx[f"{name}.r2"], tool.radii2(name))
    assert all(np.array_equal(fx[f"pi.{edges}"], tool.PI_SETS[edges]) for edges in pe.PI_SETS)
    a, b = ({c: fx[f"wide.{cat}.{c}"] for c in pe.COLUMNS} for cat in "ab")
    pairs = tool.Pairs("wide", a, b, fx["wide.r2"])
    n_checked = 0
    for key, wrong in (("by_chord", lambda c2: c2), ("by_cut", lambda c2: c2 * (1 + c2 / 12)), ("not_capped", None)):
        for record in fx[f"wide.{key}"]:
            two, i, j, row = (int(v) for v in record[:4])
            R2, c2, DD, _, p, bins, planes, inside, _ = pairs.get(two, i, j)
            if wrong is None:
                assert DD * c2 <= pairs.edges[row][-1] < R2 and bins[row] is None and bool(inside) == bool(record[4])
            else:
                other = tool.bin_of(DD * wrong(c2), pairs.edges[row])
                assert inside and bins[row] == record[4] and (-1 if other is None else other) == record[5]
                assert planes["one"] == 0 and p <= mpf(40)
            n_checked += 1
    assert pairs.violations == 0 and n_checked >= 8 * 4
