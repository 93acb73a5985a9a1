"""The exact reference of the two projected counts (``yawhip_proj_count``, ``yawhip_proj_count_pi``): tests/golden/proj_exact.npz,
written by tools/make_golden_proj_exact.py (mpmath at 50 digits from the float64 ``(ra, dec)`` and columns: the exact angle
``2 asin(chord / 2)``, ``R2 = ((d_a + d_b) / 2)^2 theta^2`` against the float64 radius edges and ``p = |c_a - c_b|`` against the
cut and the pi edges, all taken exactly -- never the contract's series). Shared by the CPU test of the mirror oracles
(tests/test_proj_exact_fixture.py), the GPU test of the kernels (tests/test_gpu_proj_exact.py) and the tool. ``K`` of the rule
``|ours - exact| <= K 2^-53 A`` is the one stored in THIS file.

Scenes ``as`` (arcseconds, five sites, ``d`` a factor 4 apart between neighbours) and ``wide`` (3 arcmin to 5.6 degrees, reaches
at the cap). Each has two catalogues ``a`` and ``b`` of two patches per site and two redshift bins per patch, and two cell
lists: ``one`` (``a`` with itself: ``proj_scenes.cells_one_handle``) and ``two`` (``a`` with ``b``: ``cells_two_handles``), each
with two more cells between different sites, which hold nothing. The planes exist for the bins as uploaded and for the bins
folded into one under both rows (``fold``: every cell of ``nb = 1`` once per row)."""
import functools

import numpy as np

from conftest import load_golden
from yet_another_wizz_amd.coordinates import radec_to_xyz

SCENES = ("as", "wide")
PI_SETS = ("one", "four", "uneven")
S2_CAP = 0.01
EPS = 2.0**-53
COLUMNS = ("ra", "dec", "w", "d", "c")


@functools.lru_cache(maxsize=None)
def fixture():
    return load_golden("proj_exact.npz")


def prefix(name, fold=False, two=False):
    """The key prefix of the planes of a scene and cell list."""
    return name + (".fold" if fold else "") + (".two" if two else ".one")


def from_columns(cols, fold=False, weighted=True):
    """The dict tests/proj_oracle.py takes from ``ra, dec, w, d, c, off`` of two bins per patch."""
    x, y, z = radec_to_xyz(np.asarray(cols["ra"]), np.asarray(cols["dec"]))
    off = np.asarray(cols["off"]).astype(np.int64)
    return dict(x=x, y=y, z=z, w=np.asarray(cols["w"]) if weighted else None, d=np.asarray(cols["d"]), c=np.asarray(cols["c"]),
                nb=1 if fold else 2, off=off[::2].copy() if fold else off)


def scene(fx, name, cat, fold=False, weighted=True):
    """Catalogue ``cat`` ("a" or "b") of the scene as the dict of tests/proj_oracle.py."""
    return from_columns({c: fx[f"{name}.{cat}.{c}"] for c in COLUMNS + ("off",)}, fold, weighted)


def cell_lists(n_sites, fold, two):
    """The cells of a scene of ``n_sites``: those of tests/proj_scenes.py -- folded, once per row -- and two between sites."""
    import proj_scenes

    nb = 1 if fold else 2
    cells = (proj_scenes.cells_two_handles if two else proj_scenes.cells_one_handle)(nb, n_sites)
    if fold:
        cells = np.concatenate([cells, cells + np.array([0, 0, 1, 0], dtype=np.int32)])
    last = 2 * n_sites - 1  # (patch 0 and patch 2: sites 0 and 1; the last patch and the last of the site before)
    between = [(0, 2 * nb, 0, 0), (last * nb + nb - 1, (last - 2) * nb + nb - 1, 1, 0)]
    return np.concatenate([cells, np.array(between, dtype=np.int32)])


def cells(fx, name, fold=False, two=False):
    return fx[f"{name}{'.fold' if fold else ''}.cells.{'two' if two else 'one'}"]


def counts(fx, name, fold=False, two=False):
    """``N`` f64[n_cells, nf]: the integer member pairs inside the cut."""
    return fx[f"{prefix(name, fold, two)}.N"]


def counts_pi(fx, name, fold, two, edges):
    """``N_pi`` f64[n_pi, n_cells, nf] of the edge set ``edges`` (a name of PI_SETS)."""
    return fx[f"{prefix(name, fold, two)}.N_pi.{edges}"]


def expected(fx, name, fold, two, edges=None):
    """``(W, A)`` of the stored weights: of the single cylinder, or of the planes of the edge set ``edges``. Every stored weight
    is > 0 (tests/test_proj_exact_fixture.py), so ``A = sum |w_a w_b|`` of a plane is its ``W_pi``: the file holds it once."""
    p = prefix(name, fold, two)
    return (fx[f"{p}.W"], fx[f"{p}.A"]) if edges is None else (fx[f"{p}.W_pi.{edges}"], fx[f"{p}.W_pi.{edges}"])


def worst_ratio(got, exp, A):
    """The largest ``|got - exp| / (2^-53 A)`` over the elements that hold a pair."""
    held = A > 0
    return float(np.max(np.abs(got - exp)[held] / (EPS * A[held]))) if held.any() else 0.0


def check(key, got, exp, A, K):
    """The rule of the weighted planes: ``|got - exp| <= K 2^-53 A`` per element and exact ``+0.0`` where the reference is
    empty. Prints and returns the worst ratio."""
    got = np.asarray(got)
    assert got.shape == exp.shape, (key, got.shape, exp.shape)
    empty = A == 0
    assert np.all(got[empty] == 0.0) and not np.any(np.signbit(got[empty])), f"{key}: an empty element is not +0.0"
    worst = worst_ratio(got, exp, A)
    print(f"{key}: worst |ours - exact| / (2^-53 A) = {worst:.3f} (K = {K:g})")
    assert np.all(np.abs(got - exp) <= K * EPS * A), (key, worst)
    return worst


def pair_floats(first, second, i, j):
    """``(s2, theta2, DD, p)`` of the pairs in float64; the angle by ``arcsin``, not by the series."""
    d = [second[c][j] - first[c][i] for c in "xyz"]
    s2 = (d[0] * d[0] + d[1] * d[1]) + d[2] * d[2]
    D = 0.5 * (second["d"][j] + first["d"][i])
    return s2, (2.0 * np.arcsin(0.5 * np.sqrt(s2))) ** 2, D * D, np.abs(second["c"][j] - first["c"][i])
