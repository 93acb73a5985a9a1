"""numpy brute force of the redshift-space pair count (``yawhip_proj_count_smu``, include/yawhip.h) over
a cell list. The pair terms are those of tests/proj_oracle.py (``pair_terms``: ``R2``, ``p = |c_a - c_b|`` and ``w_a w_b``,
every operation rounded on its own), the loop, the chunks and the order of the pairs those of
``proj_pi_oracle.proj_pi_cells``; what is new is what a pair is binned by:

    P2 = p*p;   S2 = R2 + P2;   fine bin e  iff  s2[row][e] < S2 <= s2[row][e + 1]
    j  = the number of inner edges k = 1 .. n_mu - 1 with m2[k]*S2 < P2      plane 0 is mu^2 in [0, m2[1]], plane j (m2[j], m2[j+1]]
    W[j][cell][e] += w_a*w_b                                                (no line-of-sight cut)

Small inputs only: every pair of a cell is evaluated."""
import numpy as np

from dsigma_radial_oracle import S2_CAP
from proj_oracle import as_handle, pair_terms, reach
from shear_oracle import CHUNK_PAIRS


def smu_terms(a, b, i, j):
    """``(S2, P2, ww)`` of the pairs (object ``i`` of handle ``a``, object ``j`` of handle ``b``), index arrays that broadcast."""
    R2, p, ww = pair_terms(a, b, i, j)
    P2 = p * p
    return R2 + P2, P2, ww


def mu_plane(S2, P2, m2):
    """The plane of a pair (any shape): the number of INNER edges ``m2[1 : n_mu]`` with ``fl(m2[k] S2) < P2``."""
    m2 = np.asarray(m2, dtype=np.float64)
    return (m2[1:-1] * np.asarray(S2)[..., None] < np.asarray(P2)[..., None]).sum(axis=-1)


def smu_cells(a, b, cells, s2, m2, same=None):
    """``proj_pi_oracle.proj_pi_cells`` with the rows ``s2`` f64[n_rows, E] of squared s edges and the squared mu edges ``m2``
    f64[n_mu + 1]. Returns ``(W, A, N)``, [n_mu, n_cells, E-1] each: the sums of ``w_a w_b``, of ``|w_a w_b|`` and the number
    of member pairs per mu bin, cell and fine bin, a diagonal cell holding every unordered pair once."""
    same = (a is b) if same is None else same
    s2 = np.asarray(s2, dtype=np.float64)
    m2 = np.asarray(m2, dtype=np.float64)
    n_mu, nf = len(m2) - 1, s2.shape[1] - 1
    assert n_mu >= 1 and m2[0] == 0.0 and m2[-1] == 1.0 and np.all(np.diff(m2) > 0.0)
    cells = np.asarray(cells).reshape(-1, 4)
    out = np.zeros((3, n_mu, len(cells), nf), dtype=np.float64)
    for n, (sa, sb, row, diagonal) in enumerate(cells):
        assert bool(diagonal) == (same and sa == sb), "a cell is diagonal iff it pairs a segment of one handle with itself"
        a0, a1 = int(a["off"][sa]), int(a["off"][sa + 1])  # streamed: along the rows
        b0, b1 = int(b["off"][sb]), int(b["off"][sb + 1])  # in the lanes: along the columns
        if a1 == a0 or b1 == b0:
            continue
        rows = max(1, CHUNK_PAIRS // (b1 - b0))
        j = np.arange(b0, b1)[None, :]
        for lo in range(a0, a1, rows):
            i = np.arange(lo, min(lo + rows, a1))[:, None]
            S2, P2, ww = smu_terms(a, b, i, j)
            member = (S2 > s2[row, 0]) & (S2 <= s2[row, -1])
            if diagonal:
                member &= i > j  # every unordered pair once: the streamed object has the larger index
            ii, jj = np.nonzero(member)
            if len(ii) == 0:
                continue
            e = (S2[ii, jj][:, None] > s2[row][None, :]).sum(axis=1) - 1  # s2[e] < S2 <= s2[e+1]
            slot = mu_plane(S2[ii, jj], P2[ii, jj], m2) * nf + e
            v = np.broadcast_to(ww, member.shape)[ii, jj]
            for c, term in enumerate((v, np.abs(v), np.ones(len(v)))):
                out[c, :, n] += np.bincount(slot, weights=term, minlength=n_mu * nf).reshape(n_mu, nf)
    return tuple(out)


def nearest_margins(a, b, cells, s2, m2, same=None):
    """``(margin in s, margin in mu)`` in float64: the smallest ``|S2 / edge - 1|`` over every pair of the cells and every
    edge > 0 of its row, and the smallest ``|fl(m2[k] S2) / P2 - 1|`` over ALL pairs with ``P2 > 0`` -- inside the s range or
    not -- and the inner edges (``inf`` without inner edges)."""
    same = (a is b) if same is None else same
    s2 = np.asarray(s2, dtype=np.float64)
    inner = np.asarray(m2, dtype=np.float64)[1:-1]
    worst_s, worst_mu = np.inf, np.inf
    for sa, sb, row, _ in np.asarray(cells).reshape(-1, 4):
        i = np.arange(int(a["off"][sa]), int(a["off"][sa + 1]))[:, None]
        j = np.arange(int(b["off"][sb]), int(b["off"][sb + 1]))[None, :]
        if i.size == 0 or j.size == 0:
            continue
        S2, P2, _ = smu_terms(a, b, i, j)
        keep = np.ones(S2.shape, dtype=bool)
        if same and sa == sb:
            keep &= i != j
        if not keep.any():
            continue
        edges = s2[row][s2[row] > 0]
        worst_s = min(worst_s, float(np.min(np.abs(S2[keep][:, None] / edges[None, :] - 1.0))))
        keep &= P2 > 0
        if len(inner) and keep.any():
            worst_mu = min(worst_mu, float(np.min(np.abs(inner[None, :] * S2[keep][:, None] / P2[keep][:, None] - 1.0))))
    return worst_s, worst_mu


def count_smu_fine(layout_a, layout_b, cells, s2, *, mu_edges, cosmology, unit, sort_axis=2):
    """Stand-in for ``yet_another_wizz_amd.engine.count_smu_fine`` built on the brute force, as
    ``proj_pi_oracle.count_projected_pi_fine`` stands in for the pi-binned seam: the engine's columns, its squares of the mu
    edges, and its refusal of a reach beyond the cap."""
    from yet_another_wizz_amd import engine
    from yet_another_wizz_amd._lib import CountStats

    a = as_handle(layout_a, *engine.proj_columns(layout_a, cosmology, unit))
    b = a if layout_b is layout_a else as_handle(layout_b, *engine.proj_columns(layout_b, cosmology, unit))
    if np.any(reach(a, b, cells, s2) > S2_CAP):
        engine.check_projected_reach((layout_a, layout_b), cosmology, unit, s2)
        raise AssertionError("the engine's reach check passes what the library's rule refuses")
    mu_edges = np.asarray(mu_edges, dtype=np.float64)
    W, _, _ = smu_cells(a, b, cells, s2, mu_edges * mu_edges)
    return W, CountStats(candidate_pairs=0)
