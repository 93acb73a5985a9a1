"""The exact reference of the projected position-shape count (``yawhip_proj_count_shear``): tests/golden/proj_shear_exact.npz,
written by tools/make_golden_proj_shear_exact.py (mpmath at 50 digits from the float64 ``(ra, dec)`` and columns: the exact
angle ``2 asin(chord / 2)``, ``R2 = ((d_a + d_b) / 2)^2 theta^2`` and ``p = |c_a - c_b|`` against the float64 edges taken
exactly, the exact bearing of spherical trigonometry for the rotation -- never the contract's series or its algebra). Shared
by the CPU test of the numpy oracle (tests/test_proj_shear_exact_fixture.py), the GPU test of the kernel
(tests/test_gpu_proj_shear_exact.py) and the tool, which measures ``K`` with ``worst_ratio`` below.

Scenes ``as`` (arcseconds; sites at dec 0, 60 and +-89.99 degrees and across the wrap of the right ascension) and ``wide``
(3 arcmin to 5.6 degrees, reaches next to the cap of 5.73 degrees; a ring over the pole, one across the wrap). Each has a
density catalogue ``dens`` and a shape catalogue ``shapes`` of two patches per site and two redshift bins per patch, and the
cells ``proj_scenes.cells_two_handles`` with two more between different sites, which hold nothing.

The rule per pi bin, cell and fine bin is the project's for a signed sum:
``|ours - exact| <= K * EPS * A_theta + 1e-13 * A`` with ``A = sum |w_a w_b| (|g1| + |g2|)`` over the member pairs, ``A_theta`` the
same sum with every pair divided by its angle, and ``EPS = 2^-52``. ``K`` is stored in the file. ``W`` holds to 1e-10; membership
``N`` is an integer and must be equal."""
import functools

import numpy as np

from conftest import load_golden
from yet_another_wizz_amd.coordinates import radec_to_xyz

SCENES = ("as", "wide")
PI_SETS = ("one", "four", "uneven")
EPS = 2.0**-52
ORDER_TERM = 1e-13
RTOL_W = 1e-10
PLANES = ("T", "X", "W", "A", "Ath", "N")


@functools.lru_cache(maxsize=None)
def fixture():
    return load_golden("proj_shear_exact.npz")


def catalogue(fx, scene, cat, weighted=True):
    """``dens`` or ``shapes`` of the scene as the dict of tests/proj_shear_oracle.py."""
    cols = {c: fx[f"{scene}.{cat}.{c}"] for c in ("ra", "dec", "w", "d", "c") + (("g1", "g2") if cat == "shapes" else ())}
    x, y, z = radec_to_xyz(cols.pop("ra"), cols.pop("dec"))
    if not weighted:
        cols["w"] = None
    return dict(cols, x=x, y=y, z=z, nb=2, off=fx[f"{scene}.{cat}.off"].astype(np.int64))


def expected(fx, scene, edges):
    """``{plane: f64[n_pi, n_cells, nf]}`` of the edge set ``edges`` (a name of PI_SETS), for the stored weights."""
    return {plane: fx[f"{scene}.{edges}.{plane}"] for plane in PLANES}


def worst_ratio(ours, exact, Ath):
    """Worst ``|ours - exact| / (EPS * A_theta)`` over the elements that hold a pair (0 where there are none)."""
    held = Ath > 0
    return float(np.max(np.abs(ours - exact)[held] / (EPS * Ath[held]))) if held.any() else 0.0


def check(key, got, exp, K):
    """The rule of the module docstring for ``got = (T, X, W)`` against ``exp = expected(...)``; prints the worst ratio of each
    signed plane and returns the larger."""
    worst = 0.0
    for name, ours in zip("TX", got):
        assert ours.shape == exp[name].shape, (key, name)
        ratio = worst_ratio(ours, exp[name], exp["Ath"])
        print(f"{key} {name}: worst |ours - exact| / (eps A_theta) = {ratio:.3f} (K = {K:g}) over {np.count_nonzero(exp['A'])} elements with pairs")
        assert np.all(np.abs(ours - exp[name]) <= K * EPS * exp["Ath"] + ORDER_TERM * exp["A"]), (key, name, ratio)
        assert np.all(ours[exp["N"] == 0] == 0.0) and not np.any(np.signbit(ours[exp["N"] == 0])), (key, name)
        worst = max(worst, ratio)
    W = got[2]
    assert np.all(W[exp["N"] == 0] == 0.0) and not np.any(np.signbit(W[exp["N"] == 0])), key
    np.testing.assert_allclose(W, exp["W"], rtol=RTOL_W, atol=0, err_msg=key)
    return worst
