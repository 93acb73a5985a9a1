"""numpy brute force of the projected pair count (``yawhip_proj_count``, include/yawhip.h) over a cell
list, in the operation order of the contract:

    s2  = ((ax - bx)^2 + (ay - by)^2) + (az - bz)^2
    D   = 0.5*(d_a + d_b);   DD = D*D
    q   = 1/16632;  q = 1/3150 + s2*q;  q = 1/560 + s2*q;  q = 1/90 + s2*q;  q = 1/12 + s2*q;  q = 1 + s2*q
    th2 = s2*q;   R2 = DD*th2;   fine bin e  iff  r2[row][e] < R2 <= r2[row][e + 1]
    p   = |c_a - c_b|;   the pair counts  iff  p <= pmax;   W[e] += w_a*w_b

every product and sum rounded on its own (numpy contracts nothing). The loop, the chunks and the order of the pairs are those
of tests/dsigma_radial_oracle.py: the streamed segment (of the first handle) in chunks of rows, the segment in the lanes (of
the second) along the columns. Small inputs only: every pair of a cell is evaluated."""
import numpy as np

from dsigma_radial_oracle import S2_CAP, squared_angle
from shear_oracle import CHUNK_PAIRS


def pair_terms(a, b, i, j):
    """``(R2, p, ww)`` of the pairs (object ``i`` of handle ``a``, object ``j`` of handle ``b``), index arrays that broadcast."""
    dx, dy, dz = b["x"][j] - a["x"][i], b["y"][j] - a["y"][i], b["z"][j] - a["z"][i]
    s2 = (dx * dx + dy * dy) + dz * dz
    D = 0.5 * (b["d"][j] + a["d"][i])
    R2 = (D * D) * squared_angle(s2)
    p = np.abs(b["c"][j] - a["c"][i])
    wa = 1.0 if a["w"] is None else a["w"][i]
    wb = 1.0 if b["w"] is None else b["w"][j]
    return R2, p, wb * wa


def proj_cells(a, b, cells, r2, pmax, same=None):
    """``a``, ``b`` = dict(x, y, z, w | None, d, c, nb, off[int64 P*nb+1]); cells int[n, 4] = (segment of a, segment of b, row,
    diagonal); r2 f64[n_rows, E]. ``same``: the two are one handle (default: ``a is b``); a cell is diagonal iff it then pairs a
    segment with itself, and its fourth entry must say so. Returns ``(W, A, N)``, [n_cells, E-1] each: the sums of
    ``w_a w_b``, of ``|w_a w_b|`` and the number of the cell's member pairs, a diagonal cell holding every unordered pair
    once."""
    same = (a is b) if same is None else same
    r2 = np.asarray(r2, dtype=np.float64)
    nf = r2.shape[1] - 1
    cells = np.asarray(cells).reshape(-1, 4)
    out = np.zeros((3, len(cells), nf), dtype=np.float64)
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
            member = (R2 > r2[row, 0]) & (R2 <= r2[row, -1]) & (p <= pmax)
            if diagonal:
                member &= i > j  # every unordered pair once: the streamed object has the larger index
            ii, jj = np.nonzero(member)
            if len(ii) == 0:
                continue
            e = (R2[ii, jj][:, None] > r2[row][None, :]).sum(axis=1) - 1  # r2[e] < R2 <= r2[e+1]
            v = np.broadcast_to(ww, member.shape)[ii, jj]
            for c, term in enumerate((v, np.abs(v), np.ones(len(v)))):
                out[c, n] += np.bincount(e, weights=term, minlength=nf)
    return tuple(out)


def reach(a, b, cells, r2):
    """``smax`` f64[n_rows] of the library's contract: per row the last edge over the squared least ``d`` of the redshift bins
    that the row's cells pair, times ``1 + 1e-12``; 0 where a row has no cell or a bin has no object."""
    r2 = np.asarray(r2, dtype=np.float64)

    def least_per_bin(h):
        least = np.full(h["nb"], np.inf)
        for seg in range(len(h["off"]) - 1):
            lo, hi = int(h["off"][seg]), int(h["off"][seg + 1])
            if hi > lo:
                least[seg % h["nb"]] = min(least[seg % h["nb"]], h["d"][lo:hi].min())
        return least

    least_a, least_b = least_per_bin(a), least_per_bin(b)
    least = np.zeros(len(r2))
    for sa, sb, row, _ in np.asarray(cells).reshape(-1, 4):
        da, db = least_a[sa % a["nb"]], least_b[sb % b["nb"]]
        if np.isinf(da) or np.isinf(db):
            continue
        least[row] = min(da, db) if least[row] == 0.0 else min(least[row], da, db)
    smax = np.zeros(len(r2))
    for k in np.flatnonzero(least):
        smax[k] = r2[k, -1] / (least[k] * least[k]) * (1.0 + 1e-12)
    return smax


def nearest_margin(a, b, cells, r2, pmax, same=None, skip=()):
    """The smallest ``|R2 / edge - 1|`` over every pair of the cells and every edge > 0 of its row, and the smallest
    ``|p / pmax - 1|`` (``inf`` for an infinite or zero ``pmax``): how far the scene stays off the edges and off the cut.
    ``skip``: pairs ``(index in a, index in b)`` left out (the engineered ones)."""
    same = (a is b) if same is None else same
    r2 = np.asarray(r2, dtype=np.float64)
    skip = {(int(i), int(j)) for i, j in skip}
    worst_r, worst_p = np.inf, np.inf
    for sa, sb, row, _ in np.asarray(cells).reshape(-1, 4):
        i = np.arange(int(a["off"][sa]), int(a["off"][sa + 1]))[:, None]
        j = np.arange(int(b["off"][sb]), int(b["off"][sb + 1]))[None, :]
        if i.size == 0 or j.size == 0:
            continue
        R2, p, _ = pair_terms(a, b, i, j)
        keep = np.ones(R2.shape, dtype=bool)
        if same and sa == sb:
            keep &= i != j
        for si, sj in skip:
            for u, v in ((si, sj), (sj, si)) if same else ((si, sj),):
                if i[0, 0] <= u <= i[-1, 0] and j[0, 0] <= v <= j[0, -1]:
                    keep[u - i[0, 0], v - j[0, 0]] = False
        if not keep.any():
            continue
        edges = r2[row][r2[row] > 0]
        worst_r = min(worst_r, float(np.min(np.abs(R2[keep][:, None] / edges[None, :] - 1.0))))
        if np.isfinite(pmax) and pmax > 0:
            worst_p = min(worst_p, float(np.min(np.abs(p[keep] / pmax - 1.0))))
    return worst_r, worst_p


def as_handle(layout, d, c):
    return dict(x=layout.x, y=layout.y, z=layout.z, w=layout.w, d=d, c=c, nb=layout.num_bins, off=layout.offsets)


def count_projected_fine(layout_a, layout_b, cells, r2, *, pi_max, cosmology, unit, sort_axis=2):
    """Stand-in for ``yet_another_wizz_amd.engine.count_projected_fine`` built on the brute force: lets the CPU suite exercise
    the host driver without a GPU. The columns are the engine's (``engine.proj_columns``), and so is the refusal of a reach
    beyond the cap."""
    from yet_another_wizz_amd import engine
    from yet_another_wizz_amd._lib import CountStats

    a = as_handle(layout_a, *engine.proj_columns(layout_a, cosmology, unit))
    b = a if layout_b is layout_a else as_handle(layout_b, *engine.proj_columns(layout_b, cosmology, unit))
    if np.any(reach(a, b, cells, r2) > S2_CAP):
        engine.check_projected_reach((layout_a, layout_b), cosmology, unit, r2)
        raise AssertionError("the engine's reach check passes what the library's rule refuses")
    W, _, _ = proj_cells(a, b, cells, r2, pi_max)
    return W, CountStats(candidate_pairs=0)
