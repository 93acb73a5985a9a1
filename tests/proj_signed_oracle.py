"""numpy brute force of the pi-binned projected count with a SIGNED line of sight (``yawhip_proj_count_pi_signed``,
include/yawhip.h) over a cell list of two handles. The pair terms are those of tests/proj_oracle.py
(``pair_terms``), the loop, the chunks and the order of the pairs those of ``proj_pi_oracle.proj_pi_cells``; what is new is

    ps = c_b - c_a                                          object of the SECOND handle minus object of the first
    the pair counts iff pe[0] <= ps <= pe[n];   j = the number of inner edges pe[1 .. n - 1] that are < ps
    W[j][cell][e] += w_a*w_b                                plane 0 is [pe[0], pe[1]], plane j is (pe[j], pe[j + 1]]

``|ps|`` is ``pair_terms``' ``p`` bit for bit: the same float64 difference with its sign cleared. No cell is diagonal. Small
inputs only: every pair of a cell is evaluated."""
import numpy as np

from dsigma_radial_oracle import S2_CAP
from proj_oracle import as_handle, pair_terms, reach
from shear_oracle import CHUNK_PAIRS


def mirrored(edges):
    """The signed edge set whose fold is ``edges`` (from 0): ``[-e_n .. -e_1, 0, e_1 .. e_n]``."""
    edges = np.asarray(edges, dtype=np.float64)
    return np.concatenate([-edges[::-1], edges[1:]])


def fold(planes):
    """The planes [2 n, ...] of a mirrored edge set folded onto the unsigned ones [n, ...]: positive side plus negative side
    mirrored."""
    n = len(planes) // 2
    return planes[n:] + planes[:n][::-1]


def signed_terms(a, b, i, j):
    """``(R2, ps, ww)``: ``pair_terms`` with the signed ``ps = c_b - c_a`` in the place of ``p``."""
    R2, p, ww = pair_terms(a, b, i, j)
    ps = b["c"][j] - a["c"][i]
    assert np.array_equal(np.abs(ps), p)
    return R2, ps, ww


def signed_pi_bin(ps, pi_edges):
    """The plane of ``ps`` (any shape): the number of inner edges below it; ``n`` where the pair does not count."""
    pe = np.asarray(pi_edges, dtype=np.float64)
    ps = np.asarray(ps)
    plane = (ps[..., None] > pe[1:-1]).sum(axis=-1)
    return np.where((ps >= pe[0]) & (ps <= pe[-1]), plane, len(pe) - 1)


def member_pairs(a, b, cells, r2, pi_edges):
    """Per cell the member pairs as ``(i, j, plane, e)`` index arrays (``i`` into ``a``, ``j`` into ``b``), in the order of the
    loop."""
    r2 = np.asarray(r2, dtype=np.float64)
    pe = np.asarray(pi_edges, dtype=np.float64)
    n_pi = len(pe) - 1
    assert n_pi >= 1 and np.all(np.isfinite(pe)) and np.all(np.diff(pe) > 0.0)
    out = []
    for sa, sb, row, diagonal in np.asarray(cells).reshape(-1, 4):
        assert not diagonal and not (a is b and sa == sb), "a signed count has no cell of a segment against itself"
        a0, a1 = int(a["off"][sa]), int(a["off"][sa + 1])  # streamed: along the rows
        b0, b1 = int(b["off"][sb]), int(b["off"][sb + 1])  # in the lanes: along the columns
        found = [np.zeros(0, dtype=np.int64)] * 4
        if a1 > a0 and b1 > b0:
            rows = max(1, CHUNK_PAIRS // (b1 - b0))
            j = np.arange(b0, b1)[None, :]
            parts = []
            for lo in range(a0, a1, rows):
                i = np.arange(lo, min(lo + rows, a1))[:, None]
                R2, ps, _ = signed_terms(a, b, i, j)
                plane = signed_pi_bin(ps, pe)
                ii, jj = np.nonzero((R2 > r2[row, 0]) & (R2 <= r2[row, -1]) & (plane < n_pi))
                e = (R2[ii, jj][:, None] > r2[row][None, :]).sum(axis=1) - 1  # r2[e] < R2 <= r2[e+1]
                parts.append((i[ii, 0], j[0, jj], plane[ii, jj], e))
            found = [np.concatenate(col) for col in zip(*parts)]
        out.append(tuple(found))
    return out


def proj_pi_signed_cells(a, b, cells, r2, pi_edges):
    """``proj_pi_oracle.proj_pi_cells`` with signed ``pi_edges`` f64[n + 1]. Returns ``(W, A, N)``, [n, n_cells, E-1] each: the
    sums of ``w_a w_b``, of ``|w_a w_b|`` and the number of member pairs per signed bin, cell and fine bin."""
    n_pi, nf = len(pi_edges) - 1, np.shape(r2)[1] - 1
    members = member_pairs(a, b, cells, r2, pi_edges)
    out = np.zeros((3, n_pi, len(members), nf), dtype=np.float64)
    for n, (i, j, plane, e) in enumerate(members):
        if len(i) == 0:
            continue
        v = (1.0 if b["w"] is None else b["w"][j]) * (1.0 if a["w"] is None else a["w"][i]) * np.ones(len(i))
        for c, term in enumerate((v, np.abs(v), np.ones(len(v)))):
            out[c, :, n] += np.bincount(plane * nf + e, weights=term, minlength=n_pi * nf).reshape(n_pi, nf)
    return tuple(out)


def nearest_signed_pi_margin(a, b, cells, pi_edges):
    """``(margin, least |ps|)``: the smallest ``|ps - pe_k|`` relative to ``max(|pe_k|, 1)`` over every pair of the cells --
    inside the radius range or not -- and every edge, and the smallest ``|ps|`` itself."""
    pe = np.asarray(pi_edges, dtype=np.float64)
    worst, least = np.inf, np.inf
    for sa, sb, _, _ in np.asarray(cells).reshape(-1, 4):
        i = np.arange(int(a["off"][sa]), int(a["off"][sa + 1]))[:, None]
        j = np.arange(int(b["off"][sb]), int(b["off"][sb + 1]))[None, :]
        if i.size == 0 or j.size == 0:
            continue
        ps = signed_terms(a, b, i, j)[1]
        worst = min(worst, float(np.min(np.abs(ps[..., None] - pe) / np.maximum(np.abs(pe), 1.0))))
        least = min(least, float(np.abs(ps).min()))
    return worst, least


def count_projected_pi_signed_fine(layout_a, layout_b, cells, r2, *, pi_edges, cosmology, unit, sort_axis=2):
    """Stand-in for ``yet_another_wizz_amd.engine.count_projected_pi_signed_fine`` built on the brute force, as
    ``proj_pi_oracle.count_projected_pi_fine`` stands in for the unsigned seam: the engine's columns, and its refusal of a
    reach beyond the cap."""
    from yet_another_wizz_amd import engine
    from yet_another_wizz_amd._lib import CountStats

    assert layout_b is not layout_a
    a = as_handle(layout_a, *engine.proj_columns(layout_a, cosmology, unit))
    b = as_handle(layout_b, *engine.proj_columns(layout_b, cosmology, unit))
    if np.any(reach(a, b, cells, r2) > S2_CAP):
        engine.check_projected_reach((layout_a, layout_b), cosmology, unit, r2)
        raise AssertionError("the engine's reach check passes what the library's rule refuses")
    W, _, _ = proj_pi_signed_cells(a, b, cells, r2, pi_edges)
    return W, CountStats(candidate_pairs=0)
