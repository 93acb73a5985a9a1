"""CPU: the numpy oracle of the projected position-shape count -- the contract's float64 algebra -- against the exact
reference of tests/golden/proj_shear_exact.npz (tools/make_golden_proj_shear_exact.py: mpmath at 50 digits, exact angles, radii
and bearings from the float64 ``(ra, dec)``), from arcseconds to the cap of 5.73 degrees, next to the poles and across the
wrap of the right ascension. The rule and ``K`` are those of tests/proj_shear_exact.py; the kernel meets the same file in
tests/test_gpu_proj_shear_exact.py."""
import os
import sys

import numpy as np
import pytest

import proj_oracle
import proj_shear_exact as pse
import proj_shear_oracle
from conftest import ROOT

CASES = [(scene, edges) for scene in pse.SCENES for edges in pse.PI_SETS]


def oracle_planes(fx, scene, edges, weighted=True, variant=None):
    dens, shapes = (pse.catalogue(fx, scene, cat, weighted) for cat in ("dens", "shapes"))
    return proj_shear_oracle.proj_shear_cells(dens, shapes, fx[f"{scene}.cells"], fx[f"{scene}.r2"], fx[f"pi.{edges}"], variant)


def test_the_fixture_is_what_the_issue_asks_for():
    fx = pse.fixture()
    assert fx["margin"] == 1e-6 and fx["eps"] == pse.EPS
    for scene in pse.SCENES:
        assert min(fx[f"{scene}.margin"], fx[f"{scene}.pi_margin"]) > 1e-6  # measured at 50 digits: no pair next to an edge
        assert fx[f"{scene}.one.N"].sum() > 1000 and np.all(fx[f"{scene}.uneven.N"].sum(axis=(1, 2)) > 0)  # every pi bin holds pairs
        N = fx[f"{scene}.four.N"]
        assert np.array_equal(N.sum(axis=0), fx[f"{scene}.one.N"][0]) and np.all(N[:, -2:] == 0)  # the cells between sites are empty
        assert np.all(fx[f"{scene}.shapes.w"] > 0) and np.all(fx[f"{scene}.dens.d"] > 0)
    dec = np.rad2deg(fx["as.shapes.dec"])
    for site in (0.0, 60.0, 89.99, -89.99):
        assert np.any(np.abs(dec - site) < 1e-2)
    for scene in pse.SCENES:  # partners on both sides of the wrap
        ra = np.concatenate([fx[f"{scene}.dens.ra"], fx[f"{scene}.shapes.ra"]])
        assert min(np.sum(ra < 1e-3 if scene == "as" else ra < 0.2), np.sum(ra > 6.0)) >= 10
    assert np.any(np.cos(fx["wide.shapes.ra"] - 3.3) < 0.0) and fx["wide.shapes.dec"].max() > np.deg2rad(88.0)  # a ring over the pole
    # arcseconds to the cap: the smallest radius at the largest d, and a reach next to 0.01 in both bins
    smallest = np.sqrt(fx["as.r2"].min()) / fx["as.dens.d"].max()
    assert smallest < 2.0 * np.pi / 180 / 3600
    dens, shapes = (pse.catalogue(fx, "wide", cat) for cat in ("dens", "shapes"))
    reach = proj_oracle.reach(dens, shapes, fx["wide.cells"], fx["wide.r2"])
    assert np.all((reach > 0.0095) & (reach <= 0.01))
    assert 1.0 <= fx["K"] <= 64.0 and fx["K"] >= 4.0 * fx["K_measured"] and fx["K"] < 8.0 * fx["K_measured"]
    assert os.path.getsize(os.path.join(ROOT, "tests", "golden", "proj_shear_exact.npz")) <= os.path.getsize(
        os.path.join(ROOT, "tests", "golden", "proj_exact.npz"))


@pytest.mark.parametrize("scene, edges", CASES)
def test_the_oracle_counts_the_exact_pairs_and_holds_the_rule(scene, edges):
    fx = pse.fixture()
    exp = pse.expected(fx, scene, edges)
    unit = oracle_planes(fx, scene, edges, weighted=False)
    assert np.array_equal(unit[4], exp["N"]) and np.array_equal(unit[2], exp["N"])  # membership: the file's integers
    got = oracle_planes(fx, scene, edges)
    np.testing.assert_allclose(got[3], exp["A"], rtol=1e-12, atol=0)  # the oracle's A is the file's
    worst = pse.check(f"{scene} {edges}", got[:3], exp, float(fx["K"]))
    assert worst <= float(fx["K_measured"]) * (1 + 1e-12)  # the figure K was made from


def test_the_worst_ratio_is_the_one_k_was_made_from():
    fx = pse.fixture()
    worst = 0.0
    for scene, edges in CASES:
        got, exp = oracle_planes(fx, scene, edges), pse.expected(fx, scene, edges)
        worst = max(worst, *(pse.worst_ratio(got[c], exp[plane], exp["Ath"]) for c, plane in enumerate("TX")))
    assert worst == pytest.approx(float(fx["K_measured"]), rel=1e-12)


@pytest.mark.parametrize("variant", ["sign", "end"])
def test_a_wrong_rotation_misses_the_rule(variant):
    """The sine of the double angle with the wrong sign, or the position angle taken at the density object instead of at the
    shape: the membership is untouched, and T or X leave the bound by orders of magnitude in every scene."""
    fx = pse.fixture()
    for scene in pse.SCENES:
        exp = pse.expected(fx, scene, "four")
        got = oracle_planes(fx, scene, "four", variant=variant)
        assert np.array_equal(got[4], exp["N"])
        bound = float(fx["K"]) * pse.EPS * exp["Ath"] + pse.ORDER_TERM * exp["A"]
        missed = [np.abs(got[c] - exp[plane]) > bound for c, plane in enumerate("TX")]
        assert (missed[0] | missed[1])[exp["N"] > 0].mean() > 0.9
        with pytest.raises(AssertionError):
            pse.check(f"{scene} {variant}", got[:3], exp, float(fx["K"]))
        ratio = max(pse.worst_ratio(got[c], exp[plane], exp["Ath"]) for c, plane in enumerate("TX"))
        print(f"{scene} {variant}: worst ratio {ratio:.3e} against K = {float(fx['K']):g}")
        assert ratio > 1e6 * float(fx["K"]) * (1e-3 if scene == "wide" else 1.0)


def test_two_cells_are_the_tools():
    """The T of the first two cells of each scene, summed again pair by pair with the tool's functions: the file is the product
    of its tool (a whole scene takes the tool a minute)."""
    pytest.importorskip("mpmath")
    import proj_exact

    sys.path.insert(0, os.path.join(ROOT, "tools"))
    try:
        import make_golden_proj_shear_exact as tool
    finally:
        sys.path.pop(0)
    fx = pse.fixture()
    for scene in pse.SCENES:
        dens = {c: fx[f"{scene}.dens.{c}"] for c in ("ra", "dec", "w", "d", "c", "off")}
        shapes = {c: fx[f"{scene}.shapes.{c}"] for c in ("ra", "dec", "w", "d", "c", "g1", "g2", "off")}
        cells, r2 = fx[f"{scene}.cells"], fx[f"{scene}.r2"]
        assert np.array_equal(cells, proj_exact.cell_lists(int(fx[f"{scene}.n_sites"]), False, True))
        wg1, wg2 = tool.products(shapes["w"], shapes["g1"], shapes["g2"])
        for n in (0, 1):
            sa, sb, row, _ = cells[n]
            edges = [tool.mpf(float(v)) for v in r2[row]]
            T = [tool.mpf(0)] * (r2.shape[1] - 1)
            for i in range(int(dens["off"][sa]), int(dens["off"][sa + 1])):
                for j in range(int(shapes["off"][sb]), int(shapes["off"][sb + 1])):
                    a, b = tool.Point(dens["ra"][i], dens["dec"][i]), tool.Point(shapes["ra"][j], shapes["dec"][j])
                    theta = tool.separation(tool.chord2(a, b))
                    DD = ((tool.mpf(float(dens["d"][i])) + tool.mpf(float(shapes["d"][j]))) / 2) ** 2
                    e = tool.bin_of(DD * theta * theta, edges)
                    if e is None or abs(tool.mpf(float(dens["c"][i])) - tool.mpf(float(shapes["c"][j]))) > tool.PMAX:
                        continue
                    T[e] += tool.tangential_terms(dens["w"][i], wg1[j], wg2[j], *tool.double_angle(b, a))[0]
            assert np.any(fx[f"{scene}.one.N"][0, n] > 0) and [float(v) for v in T] == list(fx[f"{scene}.one.T"][0, n]), (scene, n)
