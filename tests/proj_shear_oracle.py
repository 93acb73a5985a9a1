"""numpy brute force of the projected position-shape count (``yawhip_proj_count_shear``, include/yawhip.h; DESIGN.md section
24) over a cell list, in the operation order of the contract. With ``a`` the shape (in the lanes) and ``b`` the density
object (streamed), membership is that of tests/proj_pi_oracle.py (``proj_oracle.pair_terms``: ``R2``, ``p = |c_a - c_b|``),
the rotation that of tests/shear_oracle.py (``projection``) and the pair term

    wg1 = w_a*g1;  wg2 = w_a*g2                                   (each rounded on its own, as the upload makes them)
    tv = -(wg1*c2 + wg2*s2p);  xv = wg1*s2p - wg2*c2
    T[j][cell][e] += w_b*tv;  X[j][cell][e] += w_b*xv;  W[j][cell][e] += w_b*w_a          (den == 0: W only)

every product and sum rounded on its own (numpy contracts nothing). Small inputs only: every pair of a cell is evaluated."""
import numpy as np

from dsigma_radial_oracle import S2_CAP
from proj_oracle import as_handle, pair_terms, reach
from proj_pi_oracle import pi_bin
from shear_oracle import CHUNK_PAIRS, projection


def proj_shear_cells(dens, shapes, cells, r2, pi_edges, variant=None):
    """``dens`` = dict(x, y, z, w | None, d, c, nb, off[int64 P*nb+1]), ``shapes`` the same with ``g1, g2``; cells int[n, 4] =
    (segment of dens, segment of shapes, row, 0); r2 f64[n_rows, E]; pi_edges f64[n_pi + 1]. Returns ``(T, X, W, A, N)``,
    [n_pi, n_cells, E-1] each: the three planes, the cancellation-free magnitude ``A = sum |w_a w_b| (|g1| + |g2|)`` and the
    number of member pairs. ``variant``: a deliberately wrong rotation for the tests of the rule -- "sign" flips the sine
    of the double angle, "end" takes the position angle at the density object instead of at the shape."""
    r2 = np.asarray(r2, dtype=np.float64)
    pe = np.asarray(pi_edges, dtype=np.float64)
    n_pi, nf = len(pe) - 1, r2.shape[1] - 1
    assert n_pi >= 1 and pe[0] == 0.0 and np.all(np.diff(pe) > 0.0)
    cells = np.asarray(cells).reshape(-1, 4)
    out = np.zeros((5, n_pi, len(cells), nf), dtype=np.float64)
    ones = np.ones(len(shapes["x"]))
    sw = ones if shapes["w"] is None else shapes["w"]
    wg1, wg2 = (shapes["g1"], shapes["g2"]) if shapes["w"] is None else (shapes["w"] * shapes["g1"], shapes["w"] * shapes["g2"])
    for n, (sa, sb, row, diagonal) in enumerate(cells):
        assert not diagonal, "two handles of different kinds never pair a segment with itself"
        a0, a1 = int(dens["off"][sa]), int(dens["off"][sa + 1])  # streamed: along the rows
        b0, b1 = int(shapes["off"][sb]), int(shapes["off"][sb + 1])  # in the lanes: along the columns
        if a1 == a0 or b1 == b0:
            continue
        rows = max(1, CHUNK_PAIRS // (b1 - b0))
        j = np.arange(b0, b1)[None, :]
        for lo in range(a0, a1, rows):
            i = np.arange(lo, min(lo + rows, a1))[:, None]
            R2, p, _ = pair_terms(dens, shapes, i, j)
            plane = pi_bin(p, pe)
            member = (R2 > r2[row, 0]) & (R2 <= r2[row, -1]) & (plane < n_pi)
            ii, jj = np.nonzero(member)
            if len(ii) == 0:
                continue
            e = (R2[ii, jj][:, None] > r2[row][None, :]).sum(axis=1) - 1  # r2[e] < R2 <= r2[e+1]
            slot = plane[ii, jj] * nf + e
            di, sj = i[ii, 0], j[0, jj]  # the density object and the shape of every member pair
            shape_xyz = tuple(shapes[c][sj] for c in "xyz")
            dens_xyz = tuple(dens[c][di] for c in "xyz")
            if variant == "end":
                c2, s2p, den = projection(*dens_xyz, *shape_xyz)
            else:
                c2, s2p, den = projection(*shape_xyz, *dens_xyz)
            if variant == "sign":
                s2p = -s2p
            wb = 1.0 if dens["w"] is None else dens["w"][di]
            pole = den == 0
            tv = np.where(pole, 0.0, wb * -(wg1[sj] * c2 + wg2[sj] * s2p))
            xv = np.where(pole, 0.0, wb * (wg1[sj] * s2p - wg2[sj] * c2))
            ww = wb * sw[sj]
            av = np.abs(ww) * (np.abs(shapes["g1"][sj]) + np.abs(shapes["g2"][sj]))
            for c, term in enumerate((tv, xv, ww, av, np.ones(len(ii)))):
                out[c, :, n] += np.bincount(slot, weights=term, minlength=n_pi * nf).reshape(n_pi, nf)
    return tuple(out)


def as_shapes(layout, d, c):
    return dict(as_handle(layout, d, c), g1=layout.g1, g2=layout.g2)


def count_projected_shear_fine(dens_layout, shape_layout, cells, r2, *, pi_edges, cosmology, unit, sort_axis=2):
    """Stand-in for ``yet_another_wizz_amd.engine.count_projected_shear_fine`` built on the brute force: the engine's columns
    (``engine.proj_columns``), its refusal of a layout without shear and of a reach beyond the cap."""
    from yet_another_wizz_amd import engine
    from yet_another_wizz_amd._lib import CountStats

    engine._require_shear(shape_layout)
    dens = as_handle(dens_layout, *engine.proj_columns(dens_layout, cosmology, unit))
    shapes = as_shapes(shape_layout, *engine.proj_columns(shape_layout, cosmology, unit))
    if np.any(reach(dens, shapes, cells, r2) > S2_CAP):
        engine.check_projected_reach((dens_layout, shape_layout), cosmology, unit, r2)
        raise AssertionError("the engine's reach check passes what the library's rule refuses")
    T, X, W, _, _ = proj_shear_cells(dens, shapes, cells, r2, pi_edges)
    return (T, X, W), CountStats(candidate_pairs=0)
