"""CPU: the numpy oracle of the projected shape-shape count -- the contract's float64 algebra at both ends of a pair -- against
the exact reference of tests/golden/proj_shape_exact.npz (tools/make_golden_proj_shape_exact.py: mpmath at 50 digits, exact
angles, radii and bearings from the float64 ``(ra, dec)``), from arcseconds to the cap of 5.73 degrees, next to the poles and
across the wrap of the right ascension; the known answer of isolated pairs; and four wrong pair terms, which the file must
tell from the right one. The rule and ``K`` are those of tests/proj_shape_exact.py; the kernel meets the same file in
tests/test_gpu_proj_shape_exact.py."""
import os
import sys

import numpy as np
import pytest

import proj_oracle
import proj_shape_exact as pse
import proj_shape_oracle
import shear_oracle
import yet_another_wizz_amd as yaw
from conftest import ROOT

CASES = [(scene, which, edges) for scene in pse.SCENES for which in pse.LISTS for edges in pse.PI_SETS]
PAIR_CASES = [("pairs", variant, edges) for variant in pse.VARIANTS for edges in pse.PI_SETS]
MUTATIONS = ("both ends by the angle at a", "sB negated", "PP and XX exchanged", "PX negated")
DEG = np.pi / 180.0


def handles(fx, scene, which, weighted=True):
    """The oracle's ``(a, b)`` of a cell list: two catalogues, or ONE dict twice."""
    if scene == "pairs":
        a = pse.catalogue(fx, scene, which, weighted)
        return a, a
    a = pse.catalogue(fx, scene, "a", weighted)
    return a, (pse.catalogue(fx, scene, "b", weighted) if which == "two" else a)


def oracle_planes(fx, scene, which, edges, weighted=True):
    a, b = handles(fx, scene, which, weighted)
    return proj_shape_oracle.proj_shape_cells(a, b, pse.cells(fx, scene, which), fx[f"{scene}.r2"], fx[f"pi.{edges}"])


def unit_vectors(fx, prefix):
    ra, dec = fx[f"{prefix}.ra"], fx[f"{prefix}.dec"]
    return np.array([np.cos(dec) * np.cos(ra), np.cos(dec) * np.sin(ra), np.sin(dec)]).T


# --------------------------------------------------------------------------- 1. the fixture states what it claims
def test_the_fixture_is_what_the_issue_asks_for():
    fx = pse.fixture()
    assert fx["margin"] == 1e-6 and fx["eps"] == pse.EPS and fx["pmax"] == 40.0
    for scene in pse.SCENES + ("pairs",):
        assert min(fx[f"{scene}.margin"], fx[f"{scene}.pi_margin"]) >= 1e-6  # measured at 50 digits: no pair next to an edge
    for scene in pse.SCENES:
        n_sites = int(fx[f"{scene}.n_sites"])
        for cat in "ab":
            assert np.all(fx[f"{scene}.{cat}.w"] > 0) and np.all(fx[f"{scene}.{cat}.d"] > 0)
            assert np.array_equal(np.diff(fx[f"{scene}.{cat}.off"]), np.full(4 * n_sites, 14))  # two patches per site, two bins per patch
        for which in pse.LISTS:
            cells = pse.cells(fx, scene, which)
            assert len(cells) == {"two": 8, "one": 6}[which] * n_sites + 2
            diagonal = cells[:, 3] != 0
            assert np.array_equal(diagonal, (cells[:, 0] == cells[:, 1]) & (which == "one"))
            for edges in pse.PI_SETS:
                exp = pse.expected(fx, scene, which, edges)
                n_pi = len(fx[f"pi.{edges}"]) - 1
                assert all(exp[plane].shape == (n_pi, len(cells), 6) and exp[plane].dtype == np.float64 for plane in pse.PLANES)
                assert np.array_equal(exp["N"], np.round(exp["N"])) and np.all(exp["N"].sum(axis=(1, 2)) > 0)  # every pi bin holds pairs
                assert np.all(exp["N"][:, -2:] == 0)  # the cells between sites are empty
                assert np.array_equal(exp["A"] > 0, exp["N"] > 0) and np.array_equal(exp["Ath"] > 0, exp["N"] > 0) and np.array_equal(exp["W"] > 0, exp["N"] > 0)
                assert np.array_equal(exp["N"].sum(axis=0), fx[f"{scene}.{which}.one.N"][0])  # the planes of a set sum to the cylinder
                for plane in pse.SIGNED:
                    assert not exp[plane][exp["N"] == 0].any() and np.all(np.abs(exp[plane]) <= exp["A"])
            N = fx[f"{scene}.{which}.one.N"]
            assert N.sum() > 1000
            assert which == "two" or (N[:, diagonal].sum() > 0 and N[:, ~diagonal].sum() > 0)  # diagonal and off-diagonal cells hold pairs
    dec = fx["as.a.dec"] / DEG
    for site in (0.0, 60.0, 89.99, -89.99):
        assert np.any(np.abs(dec - site) < 1e-2)
    for scene in pse.SCENES:  # partners on both sides of the wrap
        ra = np.concatenate([fx[f"{scene}.a.ra"], fx[f"{scene}.b.ra"]])
        assert min(np.sum(ra < 1e-3 if scene == "as" else ra < 0.2), np.sum(ra > 6.0)) >= 10
    assert np.any(np.cos(fx["wide.a.ra"] - 3.3) < 0.0) and fx["wide.a.dec"].max() > 88.0 * DEG  # a ring over the pole
    # arcseconds to the cap: the smallest radius at the largest d, and a reach next to 0.01 in both bins and both lists
    assert np.sqrt(fx["as.r2"].min()) / fx["as.a.d"].max() < 2.0 * DEG / 3600
    for which in pse.LISTS:
        a, b = handles(fx, "wide", which)
        reach = proj_oracle.reach(a, b, pse.cells(fx, "wide", which), fx["wide.r2"])
        assert np.all((reach > 0.0095) & (reach <= 0.01))
    assert 1.0 <= fx["K"] <= 64.0 and fx["K_measured"] <= 20.0 and 4.0 * fx["K_measured"] <= fx["K"] < 8.0 * fx["K_measured"]
    assert os.path.getsize(os.path.join(ROOT, "tests", "golden", "proj_shape_exact.npz")) < 2**20


def test_the_known_answer_is_isolated_pairs_along_their_great_circles():
    fx = pse.fixture()
    xyz, off = unit_vectors(fx, "pairs"), fx["pairs.off"]
    assert list(off) == [0, 12, 24] and np.array_equal(fx["pairs.cells"], [(0, 0, 0, 1), (1, 1, 1, 1)]) and fx["pairs.amplitude"] == 0.1
    angle = np.arccos(np.clip(xyz @ xyz.T, -1.0, 1.0))
    partners = angle[np.arange(0, 24, 2), np.arange(1, 24, 2)]
    assert np.all((partners > 0.5 * DEG) & (partners < 5.5 * DEG))
    largest = np.sqrt(fx["pairs.r2"].max()) / fx["pairs.d"].min()  # the largest radius as an angle, at the least d
    assert largest <= 0.1
    for lo in (0, 12):  # objects of different pairs of a segment never meet
        block = angle[lo:lo + 12, lo:lo + 12]
        others = block[(np.arange(12)[:, None] // 2) != (np.arange(12)[None, :] // 2)]
        assert others.min() > largest
    dec = fx["pairs.dec"] / DEG
    assert np.sum(dec == 0.0) == 2 and np.sum(np.abs(dec - 60.0) < 1e-12) == 2
    normal = np.cross(xyz[4], xyz[5])  # the pole pair: its great circle passes within 0.1 degree of the pole
    assert np.arcsin(abs(normal[2]) / np.linalg.norm(normal)) < 0.1 * DEG and dec[4:6].min() > 87.0
    assert fx["pairs.ra"][6] > 6.0 and fx["pairs.ra"][7] < 0.1  # the wrap pair
    g1, g2 = fx["pairs.along.g1"], fx["pairs.along.g2"]
    np.testing.assert_allclose(np.hypot(g1, g2), 0.1, rtol=1e-15, atol=0)
    phi = shear_oracle.position_angle(fx["pairs.ra"], fx["pairs.dec"], fx["pairs.ra"][np.arange(24) ^ 1], fx["pairs.dec"][np.arange(24) ^ 1])
    np.testing.assert_allclose(np.column_stack([g1, g2]), 0.1 * np.column_stack([np.cos(2 * phi), np.sin(2 * phi)]), rtol=0, atol=1e-12)
    first = np.arange(24) % 2 == 0
    assert np.array_equal(fx["pairs.both.g1"], -g2) and np.array_equal(fx["pairs.both.g2"], g1)
    assert np.array_equal(fx["pairs.one.g1"], np.where(first, -g2, g1)) and np.array_equal(fx["pairs.one.g2"], np.where(first, g1, g2))
    for edges in pse.PI_SETS:  # the exact planes ARE the known answer: e^2 W in one plane, nothing in the other two
        for variant, plane in zip(pse.VARIANTS, pse.SIGNED):
            exp = pse.expected(fx, "pairs", variant, edges)
            known = 0.01 * exp["W"]
            assert exp["N"].sum() == 12 and np.array_equal(exp["N"].sum(axis=(0, 2)), [6, 6])
            for other in pse.SIGNED:
                assert np.all(np.abs(exp[other] - (known if other == plane else 0.0)) <= 1e-15 * known), (variant, edges, other)
    assert np.all(pse.expected(fx, "pairs", "one", "one")["PX"][pse.expected(fx, "pairs", "one", "one")["N"] > 0] > 0.0)  # the sign of the tool's docstring


# --------------------------------------------------------------------------- 2. the numpy oracle against the fixture
@pytest.mark.parametrize("scene, which, edges", CASES + PAIR_CASES)
def test_the_oracle_counts_the_exact_pairs_and_holds_the_rule(scene, which, edges):
    fx = pse.fixture()
    exp = pse.expected(fx, scene, which, edges)
    unit = oracle_planes(fx, scene, which, edges, weighted=False)
    assert np.array_equal(unit[5], exp["N"]) and np.array_equal(unit[3], exp["N"])  # membership: the file's integers
    got = oracle_planes(fx, scene, which, edges)
    np.testing.assert_allclose(got[4], exp["A"], rtol=1e-12, atol=0)  # the oracle's A is the file's
    worst = pse.check(f"{scene} {which} {edges}", got[:4], exp, float(fx["K"]))
    assert worst <= float(fx["K_measured"]) * (1 + 1e-12)  # the figure K was made from


def test_the_worst_ratio_is_the_one_k_was_made_from():
    fx = pse.fixture()
    worst = 0.0
    for scene, which, edges in CASES + PAIR_CASES:
        got, exp = oracle_planes(fx, scene, which, edges), pse.expected(fx, scene, which, edges)
        worst = max(worst, *(pse.worst_ratio(got[c], exp[plane], exp["Ath"]) for c, plane in enumerate(pse.SIGNED)))
    assert worst == pytest.approx(float(fx["K_measured"]), rel=1e-12)
    assert float(fx["K"]) == 2.0 ** np.ceil(np.log2(4.0 * worst))


# --------------------------------------------------------------------------- 3. the known answer
def corrfunc(planes):
    """``ShapeShapeCorrFunc`` of the one pi bin ``[0, 40]`` from ``(PP, XX, PX, W)`` [1, 2 cells, nf]: the two diagonal cells are
    the two redshift bins of patch 0; a second patch holds nothing."""
    binning = yaw.Binning([0.1, 0.5, 0.9])
    sums = yaw.PatchedSumWeights(binning, np.ones((2, 2)), np.ones((2, 2)), auto=True)
    counts = {}
    for name, plane in zip(("pp", "xx", "px", "w"), planes):
        tensor = np.zeros((2, 2, 2))
        tensor[:, 0, 0] = plane[0].sum(axis=1)
        counts[name] = yaw.NormalisedCounts(yaw.PatchedCounts(binning, tensor, auto=True), sums)
    return yaw.ShapeShapeCorrFunc([0.0, 40.0], [counts])


@pytest.mark.parametrize("edges", pse.PI_SETS)
def test_the_oracle_gives_the_known_answer_of_isolated_pairs(edges):
    """``along``: PP = sum w_a w_b e^2; both ends turned by 45 degrees: XX; one end turned: PX, with the stored (positive)
    sign. The other two planes hold nothing but rounding. Per element against ``e^2 W`` of the file, and in total against the
    weights of the pairs themselves."""
    fx = pse.fixture()
    K = float(fx["K"])
    w = fx["pairs.w"]
    total = 0.01 * np.array([(w[lo:lo + 12:2] * w[lo + 1:lo + 12:2]).sum() for lo in (0, 12)])
    for variant, plane in zip(pse.VARIANTS, pse.SIGNED):
        exp = pse.expected(fx, "pairs", variant, edges)
        got = oracle_planes(fx, "pairs", variant, edges)
        known, bound = 0.01 * exp["W"], pse.bound(exp, K)
        for c, other in enumerate(pse.SIGNED):
            assert np.all(np.abs(got[c] - (known if other == plane else 0.0)) <= bound), (variant, other)
            per_cell = got[c].sum(axis=(0, 2))
            assert np.all(np.abs(per_cell - (total if other == plane else 0.0)) <= bound.sum(axis=(0, 2))), (variant, other)
        assert np.all(got[pse.SIGNED.index(plane)][exp["N"] > 0] > 0.0)


def test_the_host_class_reports_the_sign_of_the_product_in_e_plus_and_e_cross():
    """``e+ = -t``: a shape along the great circle has ``e+ = +e``, turned by +45 degrees ``ex = x = -e``; the ``+x`` product of
    a turned and an unturned shape is ``-e^2``, PX is ``+e^2`` and ``sample("plus_cross")`` flips it once."""
    fx = pse.fixture()
    for variant, component, sign in (("along", "plus", 1.0), ("both", "cross", 1.0), ("one", "plus_cross", -1.0)):
        cf = corrfunc(oracle_planes(fx, "pairs", variant, "one")[:4])
        for other in ("plus", "cross", "plus_cross"):  # 2 dpi (sum / W) = 80 e^2, or nothing
            np.testing.assert_allclose(cf.sample(other).data, sign * 0.8 if other == component else 0.0, rtol=1e-12, atol=1e-12)
    stored = corrfunc([pse.expected(fx, "pairs", "one", "one")[plane] for plane in ("PP", "XX", "PX", "W")])
    assert np.all(stored.sample("plus_cross").data < 0.0) and np.all(pse.expected(fx, "pairs", "one", "one")["PX"].sum(axis=(0, 2)) > 0.0)


# --------------------------------------------------------------------------- 4. the fixture tells a wrong rotation from a right one
def mutated_planes(monkeypatch, fx, scene, which, edges, mutation):
    """The oracle's planes with one slip in its pair term. The two that touch the rotation replace ``projection`` in the
    oracle's namespace: the oracle calls it once for end ``a`` and then once for end ``b`` of every batch of member pairs."""
    calls = []

    def projection(*xyz):
        calls.append(shear_oracle.projection(*xyz))
        c, s, den = calls[-1]
        if len(calls) % 2 == 0 and mutation == MUTATIONS[0]:
            return calls[-2]  # the angle at a, again
        if len(calls) % 2 == 0 and mutation == MUTATIONS[1]:
            return c, -s, den
        return c, s, den

    with monkeypatch.context() as patch:
        patch.setattr(proj_shape_oracle, "projection", projection)
        PP, XX, PX, W, A, N = oracle_planes(fx, scene, which, edges)
    assert len(calls) > 0 and len(calls) % 2 == 0
    if mutation == MUTATIONS[2]:
        PP, XX = XX, PP
    if mutation == MUTATIONS[3]:
        PX = -PX
    return PP, XX, PX, W, A, N


@pytest.mark.parametrize("mutation", MUTATIONS)
def test_a_wrong_pair_term_misses_the_rule_on_wide(monkeypatch, mutation):
    """Each slip leaves membership, ``W`` and ``A`` alone and must break the rule on ``wide``, in both cell lists. What it does on
    ``as`` is printed: at arcseconds the bearing at ``b`` is the bearing at ``a`` plus pi up to the convergence of the meridians."""
    fx = pse.fixture()
    K = float(fx["K"])
    factors = {}
    for scene in pse.SCENES:
        for which in pse.LISTS:
            exp = pse.expected(fx, scene, which, "four")
            got = mutated_planes(monkeypatch, fx, scene, which, "four", mutation)
            assert np.array_equal(got[5], exp["N"])
            np.testing.assert_allclose(got[3], exp["W"], rtol=pse.RTOL_W, atol=0)
            held = exp["N"] > 0
            missed = np.zeros(exp["N"].shape, dtype=bool)
            for c, plane in enumerate(pse.SIGNED):
                missed |= np.abs(got[c] - exp[plane]) > pse.bound(exp, K)
            excess = max(float(np.max(np.abs(got[c] - exp[plane])[held] / pse.bound(exp, K)[held])) for c, plane in enumerate(pse.SIGNED))
            factors[scene, which] = (excess, missed[held].mean())
            if scene == "wide":
                assert missed[held].mean() > 0.9 and excess > 1e6, (mutation, which, excess)
                with pytest.raises(AssertionError):
                    pse.check(f"wide {which} {mutation}", got[:4], exp, K)
    for (scene, which), (excess, share) in factors.items():
        print(f"{mutation}: {scene} {which}: worst |mutant - exact| / bound = {excess:.3e}, {share:.3f} of the elements with pairs miss the rule")
    right = oracle_planes(fx, "wide", "two", "four")  # the patch is gone: the oracle is itself again
    pse.check("wide two four, unpatched", right[:4], pse.expected(fx, "wide", "two", "four"), K)


# --------------------------------------------------------------------------- 5. the file is the product of its tool
def test_two_cells_are_the_tools():
    """The first cell of each list of each scene, summed again pair by pair by the tool: every plane of the file, bit for bit
    (the whole file takes the tool a quarter of a minute)."""
    pytest.importorskip("mpmath")
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    try:
        import make_golden_proj_shape_exact as tool
    finally:
        sys.path.pop(0)
    fx = pse.fixture()
    assert all(np.array_equal(fx[f"pi.{name}"], pe) for name, pe in tool.PI_SETS.items())
    for scene in pse.SCENES:
        a, b = ({c: fx[f"{scene}.{cat}.{c}"] for c in ("ra", "dec", "w", "d", "c", "g1", "g2", "off")} for cat in "ab")
        points = {id(a): tool.mp_points(a), id(b): tool.mp_points(b)}
        for which in pse.LISTS:
            second = b if which == "two" else a
            planes, violations, _, _ = tool.exact_cells(a, second, points[id(a)], points[id(second)], pse.cells(fx, scene, which)[:1], fx[f"{scene}.r2"], 0)
            assert violations == 0
            for (edges, plane), value in planes.items():
                stored = fx[f"{scene}.{which}.{edges}.{plane}"][:, :1]
                assert np.array_equal(value, stored) and (plane != "N" or edges != "one" or value.sum() > 20), (scene, which, edges, plane)
