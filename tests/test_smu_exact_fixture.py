"""CPU: the exact reference of the two redshift-space counts, tests/golden/smu_exact.npz (tools/make_golden_smu_exact.py: mpmath,
``S2 = ((d_a + d_b) / 2)^2 (2 asin(chord / 2))^2 + (c_b - c_a)^2`` against the s edges, ``m2[k] S2 < P2`` and ``sm2[k] S2 < sign(ps) P2``
against the squares of the mu edges, no series), and the mirror oracles of the contract (tests/smu_oracle.py,
tests/smu_signed_oracle.py) against it. The conditions the tool asserts are asserted again from the stored arrays, without
mpmath: they say that no pair is left out of any comparison and that the file tells a kernel that bins by another quantity
from a right one -- shown here on four wrong variants of the oracles. The kernels meet the same file in
tests/test_gpu_smu_exact.py."""
import os
import re
import sys

import numpy as np
import pytest

import proj_oracle
import proj_scenes
import smu_exact as se
import smu_oracle
import smu_scenes
import smu_signed_oracle as sso
from conftest import ROOT
from test_proj_exact_fixture import ARCSEC, DEG, EDGE_MARGIN, N_SITES, PER_SEGMENT, bins_of, d_a_alone

CASES = [(name, fold, two) for name in se.SCENES for fold in (False, True) for two in (False, True)]
IDS = [f"{name}-{'nb=1' if fold else 'nb=2'}-{'two' if two else 'one'}" for name, fold, two in CASES]


def edge_sets(two):
    """``(signed, name)`` of every edge set a list has planes for."""
    return [(False, name) for name in se.MU_SETS] + ([(True, name) for name in se.SIGNED_SETS] if two else [])


def oracle_planes(fx, name, fold, two, weighted, signed, edges):
    a, b = se.handles(fx, name, fold, two, weighted)
    count = sso.smu_signed_cells if signed else smu_oracle.smu_cells
    return count(a, b, se.cells(fx, name, fold, two), fx[f"{name}.s2"], se.squares(fx, edges, signed))


def sentinel_floats(fx, name, listed):
    """``(S2, P2, ps, s2, DD)`` of sentinel records ``(two, i, j, ...)`` in float64, the angle by ``arcsin``."""
    a, b = se.handles(fx, name, False, True, False)
    out = np.empty((5, len(listed)))
    for two in (0, 1):
        rows = listed[:, 0] == two
        second = b if two else a
        s2, theta2, DD, p = se.pair_floats(a, second, listed[rows, 1], listed[rows, 2])
        out[:, rows] = DD * theta2 + p * p, p * p, second["c"][listed[rows, 2]] - a["c"][listed[rows, 1]], s2, DD
    return out


def test_the_file_its_mu_edges_and_its_k():
    fx = se.fixture()
    assert os.path.getsize(os.path.join(ROOT, "tests", "golden", "smu_exact.npz")) < 300 * 1024
    assert fx["eps"] == se.EPS and np.array_equal(fx["mu.one"], [0.0, 1.0])
    for edges, mu in smu_scenes.MU_SETS.items():
        assert np.array_equal(fx[f"mu.{edges}"], mu) and np.array_equal(fx[f"smu.{edges}"], se.mirrored(mu))
        assert fx[f"smu.{edges}"][len(mu) - 1] == 0.0  # 0 is an edge of every mirrored set
    assert np.array_equal(fx["smu.asymmetric"], [-1.0, -0.4, 0.1, 0.25, 1.0]) and len(smu_scenes.MU_30) == 31
    assert 1.0 <= fx["K"] <= 64.0 and fx["K"] >= 4.0 * fx["K_measured"] and np.log2(float(fx["K"])) % 1.0 == 0.0 and fx["K"] < 8.0 * fx["K_measured"]
    design = open(os.path.join(ROOT, "DESIGN.md"), encoding="utf-8").read()
    marked = re.search(r"<!-- smu-exact-K -->`K` = ([0-9.e+]+) \(worst measured ratio of the mirror oracles ([0-9.]+)\)<!-- /smu-exact-K -->", design)
    assert marked and float(marked.group(1)) == fx["K"] and float(marked.group(2)) == pytest.approx(float(fx["K_measured"]), abs=6e-4)
    keys = {f"{se.prefix(name, fold, two)}.N_{'smu' if signed else 'mu'}.{edges}" for name, fold, two in CASES for signed, edges in edge_sets(two)}
    keys |= {f"{se.prefix(name, fold, two)}.W_mu.{edges}" for name, fold, two in CASES for edges in ("one", "uniform4", "uneven")}
    assert keys <= set(fx.files) and not any("pair" in key for key in fx.files)  # per-pair records: the sentinels only
    assert not any(".N_smu." in key or ".W_smu." in key for key in fx.files if ".one." in key)  # a signed count has no diagonal cell


@pytest.mark.parametrize("name", se.SCENES)
def test_the_fixture_is_what_the_issue_asks_for(name):
    fx = se.fixture()
    s2, n_sites = fx[f"{name}.s2"], int(fx[f"{name}.n_sites"])
    assert n_sites == N_SITES[name] and s2.shape == (2, 7) and np.all(np.diff(s2, axis=1) > 0)
    ratio = s2[:, 1:] / s2[:, :-1]
    np.testing.assert_allclose(ratio, ratio[:, :1] * np.ones(6), rtol=1e-12)  # log-spaced
    for cat in "ab":
        off, w, c = fx[f"{name}.{cat}.off"], fx[f"{name}.{cat}.w"], fx[f"{name}.{cat}.c"]
        assert len(off) == 4 * n_sites + 1 and np.all(np.diff(off) == PER_SEGMENT[name]) and np.all(w > 0) and np.all(c >= 0)
    every_m2 = np.unique(np.concatenate([np.abs(se.squares(fx, edges, signed)) for signed, edges in edge_sets(True)]))
    assert every_m2[0] == 0.0 and every_m2[-1] == 1.0 and len(every_m2) >= 33  # the 30-bin set's and a few more
    margin, mu_margin = np.inf, np.inf
    for fold in (False, True):
        nb = 1 if fold else 2
        for two in (False, True):
            cells = se.cells(fx, name, fold, two)
            base = (proj_scenes.cells_two_handles if two else proj_scenes.cells_one_handle)(nb, n_sites)
            assert np.array_equal(cells, se.pe.cell_lists(n_sites, fold, two)) and len(cells) == len(base) * (2 if fold else 1) + 2
            one = se.counts(fx, name, fold, two, "one")
            assert one.shape == (1, len(cells), 6) and one.sum() > 1000 and np.all(one.sum(axis=(0, 1)) > 0)  # every s bin holds pairs
            assert not np.any(one[0, -2:]) and np.all(one[0, :-2].sum(axis=1) > 0)  # the cells between sites hold nothing, every other some
            for signed, edges in edge_sets(two):
                N = se.counts(fx, name, fold, two, edges, signed)
                assert fx[f"{se.prefix(name, fold, two)}.N_{'smu' if signed else 'mu'}.{edges}"].dtype == np.int32
                assert N.shape == (len(fx[f"{'smu' if signed else 'mu'}.{edges}"]) - 1, len(cells), 6)
                assert np.array_equal(N.sum(axis=0), one[0]) and np.all(N.sum(axis=(1, 2)) > 0)  # the planes sum to the one; each holds a pair
                W, A = se.expected(name, fold, two, edges, signed)
                assert W is A and np.array_equal(W > 0, N > 0)  # (every weight is > 0)
                np.testing.assert_allclose(W.sum(axis=0), se.expected(name, fold, two, "one")[0][0], rtol=1e-13, atol=0)
                if signed and edges != "asymmetric":  # the mirrors fold onto the unsigned planes, and are not symmetric themselves
                    assert np.array_equal(se.fold_planes(N), se.counts(fx, name, fold, two, edges)) and N[:len(N) // 2].sum() != N[len(N) // 2:].sum()
            if fold:  # the margins again in float64 from all pairs and both rows (1e-6 / 1e-9 against errors of 1e-10 / 1e-13)
                a, b = se.handles(fx, name, fold, two, False)
                in_s, in_mu = smu_oracle.nearest_margins(a, b, cells[:-2], s2, every_m2)
                margin, mu_margin = min(margin, in_s), min(mu_margin, in_mu)
                assert one.sum() > 1.3 * se.counts(fx, name, False, two, "one").sum()  # folded, a pair is binned by both rows and across bins
    for ours, stored in ((margin, fx[f"{name}.margin"]), (mu_margin, fx[f"{name}.mu_margin"])):
        assert ours >= EDGE_MARGIN[name] and stored >= EDGE_MARGIN[name] and ours == pytest.approx(float(stored), rel=1e-3)
    # the stored counts are those of float64 arcsin, and D follows the pair: d of the first object alone moves a quarter of them
    m2 = se.squares(fx, "uniform30")
    n_member, n_moved = 0, 0
    for two in (False, True):
        first, second, i, j, row = se_every_pair(fx, name, two)
        s2c, theta2, DD, p = se.pair_floats(first, second, i, j)
        S2 = DD * theta2 + p * p
        e, plane = bins_of(S2, s2[row]), smu_oracle.mu_plane(S2, p * p, m2)
        member = e >= 0
        assert member.sum() == se.counts(fx, name, False, two, "one").sum()
        assert np.array_equal(np.bincount(plane[member], minlength=30), se.counts(fx, name, False, two, "uniform30").sum(axis=(1, 2)))
        wrong = first["d"][i] ** 2 * theta2 + p * p
        n_member += member.sum()
        n_moved += np.count_nonzero((bins_of(wrong, s2[row]) != e)[member] | (smu_oracle.mu_plane(wrong, p * p, m2) != plane)[member])
    assert n_moved / n_member >= 0.25 and n_moved / n_member == pytest.approx(float(fx[f"{name}.moved"]), abs=0.002)
    print(f"{name}: {n_member} member pairs, nearest s edge {fx[f'{name}.margin']:.2e} away, nearest m2 S2 to P2 {fx[f'{name}.mu_margin']:.2e}, "
          f"d of the first object alone moves {n_moved / n_member:.3f} of them; drawn {int(fx[f'{name}.draws'])} times")


def se_every_pair(fx, name, two):
    """``test_proj_exact_fixture.every_pair`` on this file: ``(first, second, i, j, row)`` of every pair of the cells of a site."""
    first, second = se.handles(fx, name, False, two, False)
    i_all, j_all, row_all = [], [], []
    for sa, sb, row, diagonal in se.cells(fx, name, False, two)[:-2]:
        i, j = np.meshgrid(np.arange(first["off"][sa], first["off"][sa + 1]), np.arange(second["off"][sb], second["off"][sb + 1]), indexing="ij")
        keep = (i > j) if diagonal else np.ones(i.shape, dtype=bool)
        i, j = i[keep], j[keep]
        if not two:
            i, j = np.maximum(i, j), np.minimum(i, j)
        i_all.append(i), j_all.append(j), row_all.append(np.full(len(i), row))
    return first, second, np.concatenate(i_all), np.concatenate(j_all), np.concatenate(row_all)


def test_the_scenes_are_those_of_the_proj_file_with_c_scaled():
    fx = se.fixture()
    proj = se.pe.fixture()
    for name, scale in (("as", 2.0**-10), ("wide", 2.0**-6)):
        assert np.array_equal(fx[f"{name}.s2"], proj[f"{name}.r2"])  # the same two rows, read as edges of s
        for cat in "ab":
            h = se.scene(fx, name, cat)
            ordinary = h["c"] <= 120.0 * scale
            assert ordinary.mean() > 0.8 and h["c"][ordinary].max() > 100.0 * scale  # the 0 ... 120 draw times an exact power of two
    a = se.scene(fx, "as", "a")
    assert 600.0 <= a["d"].min() < 700.0 and 2400.0 < a["d"].max() <= 2500.0
    dec = np.rad2deg(fx["as.a.dec"])
    assert all(np.any(np.abs(dec - site) < 1e-2) for site in (0.0, 60.0, 89.99, -89.99))
    first, second, i, j, _ = se_every_pair(fx, "as", True)
    s2c, theta2, _, _ = se.pair_floats(first, second, i, j)
    assert np.sqrt(theta2.max()) < 61.0 * ARCSEC and np.count_nonzero(theta2 == 0.0) >= 5  # ... and the pairs at one sky position
    for fold in (False, True):  # wide: the call is accepted AT the cap, per row and folded, one handle and two, by the library's own rule
        for two in (False, True):
            a, b = se.handles(fx, "wide", fold, two, False)
            smax = proj_oracle.reach(a, b, se.cells(fx, "wide", fold, two), fx["wide.s2"])
            assert np.all((smax > 0.0095) & (smax <= se.S2_CAP)), smax
    first, second, i, j, _ = se_every_pair(fx, "wide", True)
    s2c, theta2, _, _ = se.pair_floats(first, second, i, j)
    assert np.sqrt(theta2.max()) > 5.73 * DEG and np.count_nonzero(s2c > 0.003) > 1000


def test_the_sentinels_of_the_wide_scene():
    """Each listed pair really is misbinned by the wrong formula and rightly binned by float64 arcsin arithmetic (the pairs sit
    half a term from their edge: 4e-8 at the least)."""
    fx = se.fixture()
    s2e, m2 = fx["wide.s2"], se.squares(fx, "uniform30")
    for key, wrong in (("by_chord", lambda s: s), ("by_cut", lambda s: s * (1.0 + s / 12.0))):
        listed = fx[f"wide.{key}"]
        S2, P2, _, s2c, DD = sentinel_floats(fx, "wide", listed)
        rows = s2e[listed[:, 3]]
        assert len(listed) >= 8 and np.all(listed[:, 4] >= 0) and np.array_equal(P2 > 0, listed[:, 6] == 1) and 2 * np.count_nonzero(P2 > 0) >= len(listed)
        assert np.all(bins_of(S2, rows) == listed[:, 4]) and np.all(bins_of(DD * wrong(s2c) + P2, rows) == listed[:, 5])
        assert np.all(listed[:, 4] != listed[:, 5]) and np.count_nonzero(s2c >= 0.002) >= 8  # ... at wide angles
        assert min(np.sum(listed[:, 0] == 0), np.sum(listed[:, 0] == 1)) >= 4  # of one handle and of two
    listed = fx["wide.by_chord_mu"]
    S2, P2, _, s2c, DD = sentinel_floats(fx, "wide", listed)
    rows = s2e[listed[:, 3]]
    assert len(listed) >= 8 and np.all(bins_of(S2, rows) == listed[:, 4]) and np.all(bins_of(DD * s2c + P2, rows) == listed[:, 4])
    assert np.all(smu_oracle.mu_plane(S2, P2, m2) == listed[:, 5]) and np.all(smu_oracle.mu_plane(DD * s2c + P2, P2, m2) == listed[:, 6])
    assert np.all(listed[:, 6] == listed[:, 5] + 1) and len(np.unique(listed[:, 5])) >= 3  # one plane up, at several edges
    beyond = fx["wide.not_capped"]
    S2, P2, _, s2c, DD = sentinel_floats(fx, "wide", beyond)
    last = s2e[beyond[:, 3], -1]
    assert np.all(DD * s2c + P2 <= last) and np.all(S2 > last)  # past the outer test fl(fl(DD s2) + P2), and in no bin
    assert np.array_equal(beyond[:, 4], np.where(P2 == 0, 0, np.where(2 * P2 > S2, 2, 1)))
    for row in range(2):
        kinds = np.bincount(beyond[beyond[:, 3] == row, 4], minlength=3)
        assert kinds.sum() >= 8 and kinds[0] >= 3 and kinds[2] >= 3, kinds
    print(f"wide: {len(fx['wide.by_chord'])} by chord, {len(fx['wide.by_cut'])} by cut, {len(fx['wide.by_chord_mu'])} by chord in mu, "
          f"not capped per row {np.bincount(beyond[:, 3])}")


@pytest.mark.parametrize("name", se.SCENES)
def test_the_sentinels_of_both_scenes(name):
    fx = se.fixture()
    s2e = fx[f"{name}.s2"]
    a, b = se.handles(fx, name, False, True, False)
    far = fx[f"{name}.far"]
    S2, P2, _, _, _ = sentinel_floats(fx, name, far)
    last = s2e[far[:, 3], -1]
    assert len(far) >= 8 and np.all(S2 - P2 <= last) and np.all(P2 > last)  # near on the sky, beyond the last edge in c alone
    tied = fx[f"{name}.zero_ps"]
    S2, P2, ps, _, _ = sentinel_floats(fx, name, tied)
    assert np.all(tied[:, 0] == 1) and np.all(ps == 0.0) and not np.any(np.signbit(ps)) and np.all(P2 == 0.0)
    assert np.array_equal(a["c"][tied[:, 1]].view(np.int64), b["c"][tied[:, 2]].view(np.int64))  # bit for bit
    assert np.all(bins_of(S2, s2e[tied[:, 3]]) == tied[:, 4]) and np.all(tied[:, 4] >= 0) and np.bincount(tied[:, 3], minlength=2).min() >= 8
    for edges in se.SIGNED_SETS:  # the plane whose upper edge is 0; (-0.4, 0.1] of the asymmetric set
        sm2 = se.squares(fx, edges, True)
        plane = sso.signed_mu_plane(S2, np.copysign(P2, ps), sm2)
        assert np.all(plane == (1 if edges == "asymmetric" else len(sm2) // 2 - 1))
        assert edges == "asymmetric" or (sm2[plane[0] + 1] == 0.0 and sm2[plane[0]] < 0.0)
    sky = fx[f"{name}.one_sky"]
    S2, P2, ps, s2c, _ = sentinel_floats(fx, name, sky)
    assert len(sky) >= 4 and np.all(s2c == 0.0) and np.all(S2 == P2) and np.all(P2 > 0) and np.array_equal(np.sign(ps), sky[:, 5])
    assert np.all(bins_of(S2, s2e[sky[:, 3]]) == sky[:, 4]) and np.all(sky[:, 4] >= 0)
    assert {0, 1} <= set(sky[:, 0]) and {-1, 1} <= set(sky[:, 5])
    for edges in se.MU_SETS:  # R2 == 0: the last plane; of the signed sets plane 0 if ps < 0
        assert np.all(smu_oracle.mu_plane(S2, P2, se.squares(fx, edges)) == len(fx[f"mu.{edges}"]) - 2)
    for edges in se.SIGNED_SETS:
        plane = sso.signed_mu_plane(S2, np.copysign(P2, ps), se.squares(fx, edges, True))
        assert np.array_equal(plane, np.where(ps < 0, 0, len(fx[f"smu.{edges}"]) - 2))
    print(f"{name}: {len(far)} far along the line of sight, ps == 0 per row {np.bincount(tied[:, 3])}, {len(sky)} at one sky position")


@pytest.mark.parametrize("name,fold,two", CASES, ids=IDS)
def test_the_mirror_oracles_hold_the_file(name, fold, two):
    """``N_mu`` and ``N_smu`` exactly (unit weights); ``|oracle - exact| <= K 2^-53 A`` per element of every weighted plane."""
    fx = se.fixture()
    K, worst = float(fx["K"]), 0.0
    for signed, edges in edge_sets(two):
        W, A, N = oracle_planes(fx, name, fold, two, False, signed, edges)
        assert np.array_equal(N, se.counts(fx, name, fold, two, edges, signed)) and np.array_equal(W, N) and np.array_equal(A, N)
        W, A, _ = oracle_planes(fx, name, fold, two, True, signed, edges)
        exp_w, exp_a = se.expected(name, fold, two, edges, signed)
        np.testing.assert_allclose(A, exp_a, rtol=1e-12, atol=0)  # the oracle's A is the file's
        worst = max(worst, se.check(f"{se.prefix(name, fold, two)} {'signed ' if signed else ''}{edges}", W, exp_w, exp_a, K))
    assert worst <= float(fx["K_measured"]) * (1.0 + 1e-12)
    if (name, fold, two) == ("as", True, True):
        assert worst == pytest.approx(float(fx["K_measured"]), rel=1e-12)  # the case K was made from


def above_the_edge(S2, sP2, sm2):
    """``signed_mu_plane`` with the edges closed BELOW: a pair at ``ps == 0`` then lies above the edge 0."""
    return (np.asarray(sm2, dtype=np.float64)[1:-1] * np.asarray(S2)[..., None] <= np.asarray(sP2)[..., None]).sum(axis=-1)


@pytest.mark.parametrize("variant", ["the chord", "cut after s2 / 12", "D = d_a", "ps == 0 above the edge"])
def test_a_wrong_oracle_fails_the_counts(variant, monkeypatch):
    """The fixture bites: an oracle that bins by ``DD s2 + P2``, by a series without its ``s2^2 / 90``, by the distance of one
    end, or that puts ``ps == 0`` above the edge 0 counts other pairs than the file -- the first two on ``wide`` only, in the s
    bins and, at unchanged s bins, in the planes; on ``as``, where the terms are 1e-8 and less, they still count the same pairs."""
    fx = se.fixture()
    if variant == "D = d_a":
        monkeypatch.setattr(smu_oracle, "pair_terms", d_a_alone)
    elif variant == "ps == 0 above the edge":
        monkeypatch.setattr(sso, "signed_mu_plane", above_the_edge)
    else:
        wrong = {"the chord": lambda s2: np.asarray(s2, dtype=np.float64) * 1.0, "cut after s2 / 12": lambda s2: s2 * (1.0 + s2 * (1.0 / 12.0))}[variant]
        monkeypatch.setattr(proj_oracle, "squared_angle", wrong)
    for name in ("wide", "as"):
        for fold in (False, True):
            if variant == "ps == 0 above the edge":
                tied = fx[f"{name}.zero_ps"]
                for edges in se.SIGNED_SETS:
                    N = oracle_planes(fx, name, fold, True, False, True, edges)[2]
                    differ = np.abs(N - se.counts(fx, name, fold, True, edges, True)).sum()
                    assert differ == 0 if edges == "asymmetric" else differ >= 2 * len(tied), (name, fold, edges, differ)
                continue
            for two in (False, True):
                one = oracle_planes(fx, name, fold, two, False, False, "one")[2]
                fine = oracle_planes(fx, name, fold, two, False, False, "uniform30")[2]
                differ = np.abs(one - se.counts(fx, name, fold, two, "one")).sum()
                differ_mu = np.abs(fine - se.counts(fx, name, fold, two, "uniform30")).sum()
                if name == "as" and variant != "D = d_a":
                    assert differ == 0 and differ_mu == 0
                    continue
                print(f"{variant}, {name} {'folded' if fold else 'two bins'} {'two handles' if two else 'one handle'}: {differ:.0f} pairs in another s bin, "
                      f"{differ_mu:.0f} in another element of the 30 planes")
                assert differ >= 8 and differ_mu >= differ + (16 if variant == "the chord" else 0)  # (a pair moved is two elements changed)


def test_every_sentinel_is_the_tools():
    """The stored sentinels derived again with the tool's functions: s bin, wrong bin, planes and the side of the cap."""
    pytest.importorskip("mpmath")
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    try:
        import make_golden_smu_exact as tool
    finally:
        sys.path.pop(0)
    fx = se.fixture()
    unsigned, signed = tool.mu_sets()
    assert all(np.array_equal(fx[f"mu.{edges}"], mu) for edges, mu in unsigned.items()) and all(np.array_equal(fx[f"smu.{edges}"], mu) for edges, mu in signed.items())
    assert tuple(unsigned) == se.MU_SETS and tuple(signed) == se.SIGNED_SETS
    a, b = ({c: fx[f"wide.{cat}.{c}"] for c in se.COLUMNS} for cat in "ab")
    assert np.array_equal(fx["wide.s2"], tool.radii2("wide"))
    pairs = tool.Pairs("wide", a, b, fx["wide.s2"])
    n_checked = 0
    for key in ("by_chord", "by_cut", "by_chord_mu", "not_capped", "zero_ps", "one_sky"):
        for record in fx[f"wide.{key}"]:
            two, i, j, row = (int(v) for v in record[:4])
            rec = pairs.get(two, i, j)
            chord = rec.DD * rec.c2 + rec.P2
            if key == "not_capped":
                assert chord <= pairs.edges[row][-1] < rec.S2 and rec.bins[row] is None
            elif key == "by_chord_mu":
                assert rec.bins[row] == record[4] == tool.bin_of(chord, pairs.edges[row]) and rec.planes["uniform30"] == record[5]
            elif key in ("by_chord", "by_cut"):
                other = tool.bin_of(chord if key == "by_chord" else rec.DD * (rec.c2 * (1 + rec.c2 / 12)) + rec.P2, pairs.edges[row])
                assert rec.bins[row] == record[4] and (-1 if other is None else other) == record[5]
            elif key == "zero_ps":
                assert rec.sign == 0 and rec.P2 == 0 and rec.bins[row] == record[4] and rec.splanes["uniform4"] == 3 and rec.splanes["asymmetric"] == 1
            else:
                assert rec.c2 == 0 and rec.R2 == 0 and rec.bins[row] == record[4] and rec.planes["uniform30"] == 29
            n_checked += 1
    assert n_checked >= 8 * 6
