"""numpy brute force of the redshift-space count with a SIGNED ``mu`` (``yawhip_proj_count_smu_signed``, include/yawhip.h;
DESIGN.md section 27) over a cell list of two handles. ``S2``, ``P2`` and ``w_a w_b`` are those of tests/smu_oracle.py
(``smu_terms``), the loop, the chunks and the order of the pairs those of its ``smu_cells``; what is new is

    ps = c_b - c_a;   sP2 = copysign(P2, ps)                object of the SECOND handle minus object of the first
    j  = the number of inner edges k = 1 .. n - 1 with sm2[k]*S2 < sP2,   sm2[k] = copysign(mu_k*mu_k, mu_k)
    W[j][cell][e] += w_a*w_b                                plane 0 is mu in [-1, mu_1], plane j (mu_j, mu_j+1]; no cut

No cell is diagonal. Small inputs only: every pair of a cell is evaluated."""
import numpy as np

from dsigma_radial_oracle import S2_CAP
from proj_oracle import as_handle, reach
from proj_signed_oracle import fold, mirrored  # noqa: F401 (the mirrored edge sets and their fold, shared)
from shear_oracle import CHUNK_PAIRS
from smu_oracle import smu_terms


def signed_squares(mu_edges):
    """What the engine hands the library: ``copysign(mu * mu, mu)`` of the float64 products."""
    mu_edges = np.asarray(mu_edges, dtype=np.float64)
    return np.copysign(mu_edges * mu_edges, mu_edges)


def signed_smu_terms(a, b, i, j):
    """``(S2, sP2, ps, ww)``: ``smu_terms`` with the sign of ``ps = c_b - c_a`` on ``P2``."""
    S2, P2, ww = smu_terms(a, b, i, j)
    ps = b["c"][j] - a["c"][i]
    return S2, np.copysign(P2, ps), ps, ww


def signed_mu_plane(S2, sP2, sm2):
    """The plane of a pair (any shape): the number of INNER edges ``sm2[1 : n]`` with ``fl(sm2[k] S2) < sP2``."""
    sm2 = np.asarray(sm2, dtype=np.float64)
    return (sm2[1:-1] * np.asarray(S2)[..., None] < np.asarray(sP2)[..., None]).sum(axis=-1)


def smu_signed_cells(a, b, cells, s2, sm2):
    """``smu_oracle.smu_cells`` with the signed squared mu edges ``sm2`` f64[n + 1]. Returns ``(W, A, N)``, [n, n_cells, E-1]
    each: the sums of ``w_a w_b``, of ``|w_a w_b|`` and the number of member pairs per signed mu bin, cell and fine bin."""
    s2 = np.asarray(s2, dtype=np.float64)
    sm2 = np.asarray(sm2, dtype=np.float64)
    n_mu, nf = len(sm2) - 1, s2.shape[1] - 1
    assert n_mu >= 1 and sm2[0] == -1.0 and sm2[-1] == 1.0 and np.all(np.diff(sm2) > 0.0)
    cells = np.asarray(cells).reshape(-1, 4)
    out = np.zeros((3, n_mu, len(cells), nf), dtype=np.float64)
    for n, (sa, sb, row, diagonal) in enumerate(cells):
        assert not diagonal and not (a is b and sa == sb), "a signed count has no cell of a segment against itself"
        a0, a1 = int(a["off"][sa]), int(a["off"][sa + 1])  # streamed: along the rows
        b0, b1 = int(b["off"][sb]), int(b["off"][sb + 1])  # in the lanes: along the columns
        if a1 == a0 or b1 == b0:
            continue
        rows = max(1, CHUNK_PAIRS // (b1 - b0))
        j = np.arange(b0, b1)[None, :]
        for lo in range(a0, a1, rows):
            i = np.arange(lo, min(lo + rows, a1))[:, None]
            S2, sP2, _, ww = signed_smu_terms(a, b, i, j)
            ii, jj = np.nonzero((S2 > s2[row, 0]) & (S2 <= s2[row, -1]))
            if len(ii) == 0:
                continue
            e = (S2[ii, jj][:, None] > s2[row][None, :]).sum(axis=1) - 1  # s2[e] < S2 <= s2[e+1]
            slot = signed_mu_plane(S2[ii, jj], sP2[ii, jj], sm2) * nf + e
            v = np.broadcast_to(ww, S2.shape)[ii, jj]
            for c, term in enumerate((v, np.abs(v), np.ones(len(v)))):
                out[c, :, n] += np.bincount(slot, weights=term, minlength=n_mu * nf).reshape(n_mu, nf)
    return tuple(out)


def nearest_signed_mu_margin(a, b, cells, sm2):
    """``(margin, least |ps|)``: the smallest ``|fl(sm2[k] S2) / sP2 - 1|`` over ALL pairs of the cells with ``ps != 0`` --
    inside the s range or not -- and the inner edges (``inf`` without inner edges; an edge at 0 is as far as it can be from
    a pair with ``ps != 0``), and the smallest ``|ps|`` itself."""
    inner = np.asarray(sm2, dtype=np.float64)[1:-1]
    worst, least = np.inf, np.inf
    for sa, sb, _, _ in np.asarray(cells).reshape(-1, 4):
        i = np.arange(int(a["off"][sa]), int(a["off"][sa + 1]))[:, None]
        j = np.arange(int(b["off"][sb]), int(b["off"][sb + 1]))[None, :]
        if i.size == 0 or j.size == 0:
            continue
        S2, sP2, ps, _ = signed_smu_terms(a, b, i, j)
        least = min(least, float(np.abs(ps).min()))
        keep = sP2 != 0
        if len(inner) and keep.any():
            worst = min(worst, float(np.min(np.abs(inner[None, :] * S2[keep][:, None] / sP2[keep][:, None] - 1.0))))
    return worst, least


def count_smu_signed_fine(layout_a, layout_b, cells, s2, *, mu_edges, cosmology, unit, sort_axis=2):
    """Stand-in for ``yet_another_wizz_amd.engine.count_smu_signed_fine`` built on the brute force, as
    ``smu_oracle.count_smu_fine`` stands in for the unsigned seam: the engine's columns, its signed squares of the mu edges,
    and its refusal of a reach beyond the cap."""
    from yet_another_wizz_amd import engine
    from yet_another_wizz_amd._lib import CountStats

    assert layout_b is not layout_a
    a = as_handle(layout_a, *engine.proj_columns(layout_a, cosmology, unit))
    b = as_handle(layout_b, *engine.proj_columns(layout_b, cosmology, unit))
    if np.any(reach(a, b, cells, s2) > S2_CAP):
        engine.check_projected_reach((layout_a, layout_b), cosmology, unit, s2)
        raise AssertionError("the engine's reach check passes what the library's rule refuses")
    W, _, _ = smu_signed_cells(a, b, cells, s2, signed_squares(mu_edges))
    return W, CountStats(candidate_pairs=0)
