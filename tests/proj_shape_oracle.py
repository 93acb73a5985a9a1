"""numpy brute force of the projected shape-shape count (``yawhip_proj_count_shapes``, include/yawhip.h)
over a cell list, in the operation order of the contract. With ``a`` the streamed shape and ``b`` the shape in the lanes,
membership is that of tests/proj_pi_oracle.py (``proj_oracle.pair_terms``: ``R2``, ``p = |c_a - c_b|``; ``pi_bin``), the
rotation that of tests/shear_oracle.py (``projection``) at BOTH ends -- each shape by the position angle of the other seen from
it -- and the pair term

    wg1 = w*g1;  wg2 = w*g2                                       (each rounded on its own, as the upload makes them)
    tA = -(wg1_a*cA + wg2_a*sA);  xA = wg1_a*sA - wg2_a*cA;  tB, xB the same of b with (cB, sB)
    PP[j][cell][e] += tA*tB;  XX[j][cell][e] += xA*xB;  PX[j][cell][e] += tA*xB + xA*tB;  W[j][cell][e] += w_a*w_b
                                                                  (denA == 0 or denB == 0: W only)

every product and sum rounded on its own (numpy contracts nothing). Every term is bit-symmetric under a <-> b, so it does not
matter which of the two the device keeps in a lane. Small inputs only: every pair of a cell is evaluated."""
import numpy as np

from dsigma_radial_oracle import S2_CAP
from proj_oracle import as_handle, pair_terms, reach
from proj_pi_oracle import pi_bin
from shear_oracle import CHUNK_PAIRS, projection


def weighted_shear(h):
    """``(w, w g1, w g2)`` of a shape handle as the upload makes them."""
    if h["w"] is None:
        return np.ones(len(h["x"])), h["g1"], h["g2"]
    return h["w"], h["w"] * h["g1"], h["w"] * h["g2"]


def proj_shape_cells(a, b, cells, r2, pi_edges, same=None):
    """``a``, ``b`` = dict(x, y, z, w | None, g1, g2, d, c, nb, off[int64 P*nb+1]); cells int[n, 4] = (segment of a, segment of
    b, row, diagonal); r2 f64[n_rows, E]; pi_edges f64[n_pi + 1]. ``same``: the two are one handle (default: ``a is b``); a cell
    is diagonal iff it then pairs a segment with itself, its fourth entry must say so, and it takes ``i < j`` only. Returns
    ``(PP, XX, PX, W, A, N)``, [n_pi, n_cells, E-1] each: the four planes, the cancellation-free magnitude
    ``A = sum |w_a w_b| (|g1_a| + |g2_a|) (|g1_b| + |g2_b|)`` and the number of member pairs."""
    same = (a is b) if same is None else same
    r2 = np.asarray(r2, dtype=np.float64)
    pe = np.asarray(pi_edges, dtype=np.float64)
    n_pi, nf = len(pe) - 1, r2.shape[1] - 1
    assert n_pi >= 1 and pe[0] == 0.0 and np.all(np.diff(pe) > 0.0)
    cells = np.asarray(cells).reshape(-1, 4)
    out = np.zeros((6, n_pi, len(cells), nf), dtype=np.float64)
    (wa, ag1, ag2), (wb, bg1, bg2) = weighted_shear(a), weighted_shear(b)
    mag_a, mag_b = np.abs(a["g1"]) + np.abs(a["g2"]), np.abs(b["g1"]) + np.abs(b["g2"])
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
            R2, p, _ = pair_terms(a, b, i, j)
            plane = pi_bin(p, pe)
            member = (R2 > r2[row, 0]) & (R2 <= r2[row, -1]) & (plane < n_pi)
            if diagonal:
                member &= i < j  # every unordered pair once
            ii, jj = np.nonzero(member)
            if len(ii) == 0:
                continue
            e = (R2[ii, jj][:, None] > r2[row][None, :]).sum(axis=1) - 1  # r2[e] < R2 <= r2[e+1]
            slot = plane[ii, jj] * nf + e
            ai, bj = i[ii, 0], j[0, jj]
            a_xyz, b_xyz = tuple(a[c][ai] for c in "xyz"), tuple(b[c][bj] for c in "xyz")
            cA, sA, denA = projection(*a_xyz, *b_xyz)  # the position angle of b seen from a
            cB, sB, denB = projection(*b_xyz, *a_xyz)  # ... and of a seen from b
            tA, xA = -(ag1[ai] * cA + ag2[ai] * sA), ag1[ai] * sA - ag2[ai] * cA
            tB, xB = -(bg1[bj] * cB + bg2[bj] * sB), bg1[bj] * sB - bg2[bj] * cB
            pole = (denA == 0) | (denB == 0)
            with np.errstate(invalid="ignore"):
                pp, xx, px = (np.where(pole, 0.0, v) for v in (tA * tB, xA * xB, tA * xB + xA * tB))
            ww = wa[ai] * wb[bj]
            av = np.abs(ww) * mag_a[ai] * mag_b[bj]
            for c, term in enumerate((pp, xx, px, ww, av, np.ones(len(ii)))):
                out[c, :, n] += np.bincount(slot, weights=term, minlength=n_pi * nf).reshape(n_pi, nf)
    return tuple(out)


def as_shapes(layout, d, c):
    return dict(as_handle(layout, d, c), g1=layout.g1, g2=layout.g2)


def count_projected_shapes_fine(layout_a, layout_b, cells, r2, *, pi_edges, cosmology, unit, sort_axis=2):
    """Stand-in for ``yet_another_wizz_amd.engine.count_projected_shapes_fine`` built on the brute force: the engine's columns
    (``engine.proj_columns``), its refusal of a layout without shear, of more pi bins than the cap and of a reach beyond the
    cap."""
    from yet_another_wizz_amd import engine
    from yet_another_wizz_amd._lib import CountStats

    engine._require_shear(layout_a, layout_b)
    engine.check_shape_pi_cap(len(pi_edges) - 1, np.shape(r2)[1])
    a = as_shapes(layout_a, *engine.proj_columns(layout_a, cosmology, unit))
    b = a if layout_b is layout_a else as_shapes(layout_b, *engine.proj_columns(layout_b, cosmology, unit))
    if np.any(reach(a, b, cells, r2) > S2_CAP):
        engine.check_projected_reach((layout_a, layout_b), cosmology, unit, r2)
        raise AssertionError("the engine's reach check passes what the library's rule refuses")
    PP, XX, PX, W, _, _ = proj_shape_cells(a, b, cells, r2, pi_edges)
    return (PP, XX, PX, W), CountStats(candidate_pairs=0)
