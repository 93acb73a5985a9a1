"""The exact reference of the two redshift-space counts (``yawhip_proj_count_smu``, ``yawhip_proj_count_smu_signed``):
tests/golden/smu_exact.npz, written by tools/make_golden_smu_exact.py (mpmath at 50 digits from the float64 ``(ra, dec)`` and
columns: the exact angle ``2 asin(chord / 2)``, ``S2 = ((d_a + d_b) / 2)^2 theta^2 + (c_b - c_a)^2`` against the float64 s edges and
``m2[k] S2 < P2`` / ``sm2[k] S2 < sign(ps) P2`` against the float64 squares of the mu edges, all taken exactly -- never the
contract's series). Shared by the CPU test of the mirror oracles (tests/test_smu_exact_fixture.py), the GPU test of the kernels
(tests/test_gpu_smu_exact.py) and the tool. ``K`` of the rule ``|ours - exact| <= K 2^-53 A`` is the one stored in THIS file.

Scenes, catalogues, cell lists and folding are those of tests/proj_exact.py, whose ``from_columns``, ``cells``, ``prefix``,
``check`` and ``worst_ratio`` serve here. The integer planes ``N_mu.<set>`` (and ``N_smu.<set>`` for the list ``two``) are the
file's for every set. The exact weighted planes are the file's for the sets it stores them for; for the 30-bin set and its
mirror ``summed`` adds the exact products ``w_a w_b`` as integers over the mirror oracle's member pairs and rounds once --
exact because those member pairs, element for element, are as many as the file's (asserted on every call) and the scene stays
off every edge by a margin a thousand times the oracle's error. The tool asserts that this reproduces its own sums bit for bit."""
import functools

import numpy as np

import proj_exact as pe
import smu_oracle
import smu_scenes
import smu_signed_oracle
from conftest import load_golden
from proj_exact import EPS, S2_CAP, cells, check, pair_floats, prefix, worst_ratio  # noqa: F401 (shared with the proj file)
from proj_signed_oracle import fold as fold_planes, mirrored  # noqa: F401

SCENES = ("as", "wide")
MU_ASYMMETRIC = np.array([-1.0, -0.4, 0.1, 0.25, 1.0])
MU_SETS = ("one",) + tuple(smu_scenes.MU_SETS)
SIGNED_SETS = tuple(smu_scenes.MU_SETS) + ("asymmetric",)
COLUMNS = pe.COLUMNS


@functools.lru_cache(maxsize=None)
def fixture():
    return load_golden("smu_exact.npz")


def scene(fx, name, cat, fold=False, weighted=True):
    """Catalogue ``cat`` ("a" or "b") of the scene as the dict of tests/proj_oracle.py."""
    return pe.from_columns({c: fx[f"{name}.{cat}.{c}"] for c in COLUMNS + ("off",)}, fold, weighted)


def handles(fx, name, fold, two, weighted):
    a = scene(fx, name, "a", fold, weighted)
    return a, (scene(fx, name, "b", fold, weighted) if two else a)


def squares(fx, edges, signed=False):
    """What the engine hands the library for the edge set ``edges``: ``mu * mu``, signed ``copysign(mu * mu, mu)``."""
    return smu_signed_oracle.signed_squares(fx[f"smu.{edges}"]) if signed else smu_scenes.squares(fx[f"mu.{edges}"])


def counts(fx, name, fold, two, edges, signed=False):
    """``N`` f64[n_mu, n_cells, nf] of the edge set ``edges``: the integer member pairs per plane, cell and fine bin."""
    return fx[f"{prefix(name, fold, two)}.N_{'smu' if signed else 'mu'}.{edges}"].astype(np.float64)


def member_pairs(a, b, cells_, s2, sq, signed):
    """Per cell ``(i, j, plane, e)`` of the mirror oracle's member pairs, in the oracles' own terms (``smu_oracle.smu_terms``,
    ``mu_plane`` and their signed siblings)."""
    for sa, sb, row, diagonal in np.asarray(cells_).reshape(-1, 4):
        i = np.arange(int(a["off"][sa]), int(a["off"][sa + 1]))[:, None]
        j = np.arange(int(b["off"][sb]), int(b["off"][sb + 1]))[None, :]
        if signed:
            S2, P2, _, _ = smu_signed_oracle.signed_smu_terms(a, b, i, j)
        else:
            S2, P2, _ = smu_oracle.smu_terms(a, b, i, j)
        member = (S2 > s2[row, 0]) & (S2 <= s2[row, -1])
        if diagonal:
            member &= i > j
        ii, jj = np.nonzero(member)
        e = (S2[ii, jj][:, None] > s2[row][None, :]).sum(axis=1) - 1
        plane = (smu_signed_oracle.signed_mu_plane if signed else smu_oracle.mu_plane)(S2[ii, jj], P2[ii, jj], sq)
        yield i[ii, 0], j[0, jj], plane, e


def summed(fx, name, fold, two, edges, signed=False):
    """The exact ``W`` of the stored weights, rounded once: integer sums of ``(w_a 2^62) (w_b 2^62)`` over the member pairs."""
    a, b = handles(fx, name, fold, two, True)
    wa, wb = ([int(w * 2.0**62) for w in h["w"]] for h in (a, b))
    assert all(np.array_equal(np.array(ints, dtype=np.float64) * 2.0**-62, h["w"]) for ints, h in ((wa, a), (wb, b)))  # nothing cut off
    N = counts(fx, name, fold, two, edges, signed)
    W, seen = np.zeros(N.shape), np.zeros(N.shape)
    for c, (i, j, plane, e) in enumerate(member_pairs(a, b, cells(fx, name, fold, two), fx[f"{name}.s2"], squares(fx, edges, signed), signed)):
        sums = {}
        for i_, j_, slot in zip(i.tolist(), j.tolist(), zip(plane.tolist(), e.tolist())):
            sums[slot] = sums.get(slot, 0) + wa[i_] * wb[j_]
        for (plane_, e_), total in sums.items():
            W[plane_, c, e_] = float(total) * 2.0**-124
        np.add.at(seen, (plane, c, e), 1.0)
    assert np.array_equal(seen, N), "the mirror oracle's member pairs are not the file's"
    return W


@functools.lru_cache(maxsize=None)
def _expected(name, fold, two, edges, signed):
    fx = fixture()
    key = f"{prefix(name, fold, two)}.W_{'smu' if signed else 'mu'}.{edges}"
    W = fx[key] if key in fx.files else summed(fx, name, fold, two, edges, signed)
    W.setflags(write=False)
    return W


def expected(name, fold, two, edges, signed=False):
    """``(W, A)`` of the stored weights over the planes of the edge set ``edges``, computed once and never modified. Every
    stored weight is > 0 (tests/test_smu_exact_fixture.py), so ``A = sum |w_a w_b|`` of an element is its ``W``."""
    W = _expected(name, bool(fold), bool(two), edges, bool(signed))
    return W, W
