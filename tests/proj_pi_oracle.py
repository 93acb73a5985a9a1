"""numpy brute force of the pi-binned projected pair count (``yawhip_proj_count_pi``, include/yawhip.h)
over a cell list. The pair terms are those of tests/proj_oracle.py (``pair_terms``: ``R2``, ``p = |c_a - c_b|`` and
``w_a w_b``, every operation rounded on its own), the loop, the chunks and the order of the pairs those of its
``proj_cells``; what is new is the pair's plane:

    j = the number of edges pe[1 .. n_pi] that are < p      plane 0 is [0, pe[1]], plane j is (pe[j], pe[j + 1]]
    the pair counts iff j < n_pi;   W[j][cell][e] += w_a*w_b

Small inputs only: every pair of a cell is evaluated."""
import numpy as np

from dsigma_radial_oracle import S2_CAP
from proj_oracle import as_handle, pair_terms, reach
from shear_oracle import CHUNK_PAIRS

# the three edge sets of the tests (DESIGN.md section 22 has their margins on the shared scenes)
UNIFORM_4 = np.linspace(0.0, 40.0, 5)
UNIFORM_30 = np.linspace(0.0, 40.0, 31)
UNEVEN = np.array([0.0, 0.7, 3.1, 9.3, 22.9, 40.0])


def pi_bin(p, pi_edges):
    """The plane of ``p`` (any shape): the number of edges ``pe[1:]`` below it; ``n_pi`` where the pair does not count."""
    pe = np.asarray(pi_edges, dtype=np.float64)
    return (np.asarray(p)[..., None] > pe[1:]).sum(axis=-1)


def proj_pi_cells(a, b, cells, r2, pi_edges, same=None):
    """``proj_oracle.proj_cells`` with ``pi_edges`` f64[n_pi + 1] in the place of ``pmax``. Returns ``(W, A, N)``,
    [n_pi, n_cells, E-1] each: the sums of ``w_a w_b``, of ``|w_a w_b|`` and the number of member pairs per pi bin, cell
    and fine bin, a diagonal cell holding every unordered pair once."""
    same = (a is b) if same is None else same
    r2 = np.asarray(r2, dtype=np.float64)
    pe = np.asarray(pi_edges, dtype=np.float64)
    n_pi, nf = len(pe) - 1, r2.shape[1] - 1
    assert n_pi >= 1 and pe[0] == 0.0 and np.all(np.diff(pe) > 0.0)
    cells = np.asarray(cells).reshape(-1, 4)
    out = np.zeros((3, n_pi, len(cells), nf), dtype=np.float64)
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
            R2, p, ww = pair_terms(a, b, i, j)
            plane = pi_bin(p, pe)
            member = (R2 > r2[row, 0]) & (R2 <= r2[row, -1]) & (plane < n_pi)
            if diagonal:
                member &= i > j  # every unordered pair once: the streamed object has the larger index
            ii, jj = np.nonzero(member)
            if len(ii) == 0:
                continue
            e = (R2[ii, jj][:, None] > r2[row][None, :]).sum(axis=1) - 1  # r2[e] < R2 <= r2[e+1]
            slot = plane[ii, jj] * nf + e
            v = np.broadcast_to(ww, member.shape)[ii, jj]
            for c, term in enumerate((v, np.abs(v), np.ones(len(v)))):
                out[c, :, n] += np.bincount(slot, weights=term, minlength=n_pi * nf).reshape(n_pi, nf)
    return tuple(out)


def nearest_pi_margin(a, b, cells, pi_edges, same=None, skip=()):
    """``(margin, least p)``: the smallest ``|p / pe_j - 1|`` over every pair of the cells -- inside the radius range or not
    -- and every finite edge > 0, and the smallest ``p`` itself. ``skip``: pairs ``(index in a, index in b)`` left out (the
    engineered ones)."""
    same = (a is b) if same is None else same
    pe = np.asarray(pi_edges, dtype=np.float64)
    edges = pe[(pe > 0) & np.isfinite(pe)]
    skip = {(int(i), int(j)) for i, j in skip}
    worst, least = np.inf, np.inf
    for sa, sb, _, _ in np.asarray(cells).reshape(-1, 4):
        i = np.arange(int(a["off"][sa]), int(a["off"][sa + 1]))[:, None]
        j = np.arange(int(b["off"][sb]), int(b["off"][sb + 1]))[None, :]
        if i.size == 0 or j.size == 0:
            continue
        p = np.broadcast_to(pair_terms(a, b, i, j)[1], (i.size, j.size))
        keep = np.ones(p.shape, dtype=bool)
        if same and sa == sb:
            keep &= i != j
        for si, sj in skip:
            for u, v in ((si, sj), (sj, si)) if same else ((si, sj),):
                if i[0, 0] <= u <= i[-1, 0] and j[0, 0] <= v <= j[0, -1]:
                    keep[u - i[0, 0], v - j[0, 0]] = False
        if not keep.any():
            continue
        worst = min(worst, float(np.min(np.abs(p[keep][:, None] / edges[None, :] - 1.0))))
        least = min(least, float(p[keep].min()))
    return worst, least


def count_projected_pi_fine(layout_a, layout_b, cells, r2, *, pi_edges, cosmology, unit, sort_axis=2):
    """Stand-in for ``yet_another_wizz_amd.engine.count_projected_pi_fine`` built on the brute force, as
    ``proj_oracle.count_projected_fine`` stands in for the single-cylinder seam: the engine's columns, and its refusal of a
    reach beyond the cap."""
    from yet_another_wizz_amd import engine
    from yet_another_wizz_amd._lib import CountStats

    a = as_handle(layout_a, *engine.proj_columns(layout_a, cosmology, unit))
    b = a if layout_b is layout_a else as_handle(layout_b, *engine.proj_columns(layout_b, cosmology, unit))
    if np.any(reach(a, b, cells, r2) > S2_CAP):
        engine.check_projected_reach((layout_a, layout_b), cosmology, unit, r2)
        raise AssertionError("the engine's reach check passes what the library's rule refuses")
    W, _, _ = proj_pi_cells(a, b, cells, r2, pi_edges)
    return W, CountStats(candidate_pairs=0)
