"""GPU: the projected shape-shape count (``yawhip_proj_count_shapes``) on the device against the exact reference of
tests/golden/proj_shape_exact.npz (tools/make_golden_proj_shape_exact.py: mpmath, the exact angle, radius and line-of-sight
separation for the membership and the exact bearing at BOTH ends for the rotation -- not the contract's series or its
algebra): a scene at 0.5 to 30 arcseconds at dec 0, 60, +-89.99 degrees and across the wrap of the right ascension, one from 3
arcmin to 5.6 degrees (over the pole, across the wrap) whose nearest objects reach the cap of 0.01, each between two handles
and on ONE handle with diagonal cells, and isolated pairs whose answer is known in closed form.

With unit weights ``W`` is the integer pair count ``N`` of the file, bit for bit, and ``yawhip_proj_count_pi``'s on the same
columns; with the file's weights ``PP``, ``XX`` and ``PX`` hold ``|ours - exact| <= K 2^-52 A_theta + 1e-13 A`` per pi bin, cell and
fine bin with the ``K`` of the file, and every plane is ``+0.0`` where the reference is empty. Every case prints its worst
ratio. A few hundred objects per call; nothing here reads mpmath."""
import numpy as np
import pytest

import proj_shape_exact as pse
from test_gpu_projected import upload
from test_gpu_projected_shear import upload_shapes
from yet_another_wizz_amd import _lib, engine

pytestmark = pytest.mark.gpu


def run(fx, scene, which, weighted=True, axis_a=2, axis_b=None, *, tie=False, swap=False, copy=False):
    """The count of the three edge sets on one upload -> ``{edge set: ((PP, XX, PX, W), stats, W_pi | None)}``. ``which``: the
    cell list -- ``two``: ``a`` with ``b``; ``one`` (and a set of shears of ``pairs``): ONE handle passed twice. ``tie``: also
    ``yawhip_proj_count_pi`` on the same columns as plain projected handles; ``swap``: ``b, a`` with the cell columns
    transposed; ``copy``: the handle against a second upload of itself, no cell diagonal -- every pair twice."""
    ctx = engine.get_context(0)
    cells, r2 = pse.cells(fx, scene, which), fx[f"{scene}.r2"]
    two = scene != "pairs" and which == "two"
    first = pse.catalogue(fx, scene, which if scene == "pairs" else "a", weighted)
    second = pse.catalogue(fx, scene, "b", weighted) if two else first
    axis_b = axis_a if axis_b is None else axis_b
    made = [upload_shapes(ctx, first, axis_a)]
    try:
        if two or copy:
            made.append(upload_shapes(ctx, second, axis_b))
        a, b = made[0], made[-1]
        if copy:
            cells = cells * np.array([1, 1, 1, 0], dtype=cells.dtype)
        if swap:
            a, b, cells = b, a, np.ascontiguousarray(cells[:, [1, 0, 2, 3]])
        plain = []
        if tie:
            plain = [upload(ctx, first, axis_a)] + ([upload(ctx, second, axis_b)] if two else [])
            made += plain
        out = {}
        for edges in pse.PI_SETS:
            planes, stats = _lib.proj_count_shapes(ctx, a, b, cells, r2, fx[f"pi.{edges}"])
            assert len(planes) == 4 and stats.n_workgroups == len(cells) and 0 < stats.evaluated_pairs <= stats.candidate_pairs
            W_pi = _lib.proj_count_pi(ctx, plain[0], plain[-1], cells, r2, fx[f"pi.{edges}"])[0] if tie else None
            out[edges] = (planes, stats, W_pi)
    finally:
        for handle in made:
            handle.free()
    return out


# --------------------------------------------------------------------------- 1. membership and sums
@pytest.mark.parametrize("which", pse.LISTS)
@pytest.mark.parametrize("sort_axis", [0, 1, 2])
@pytest.mark.parametrize("scene", pse.SCENES)
def test_membership_and_sums_are_the_exact_ones(scene, sort_axis, which):
    fx = pse.fixture()
    K = float(fx["K"])
    unit = run(fx, scene, which, False, sort_axis, tie=True)
    weighted = run(fx, scene, which, True, sort_axis)
    worst = 0.0
    for edges in pse.PI_SETS:
        exp = pse.expected(fx, scene, which, edges)
        (_, _, _, N), _, W_pi = unit[edges]
        assert exp["N"].sum() > 1000 and np.array_equal(N, exp["N"]), (scene, which, edges, np.abs(N - exp["N"]).sum())
        assert np.array_equal(N, W_pi)  # ... and the pi count's on the same columns
        worst = max(worst, pse.check(f"device {scene} {which} {edges} axis={sort_axis}", weighted[edges][0], exp, K))
    print(f"device {scene} {which} axis={sort_axis}: worst ratio {worst:.3f} (K_measured, the numpy oracle's: {float(fx['K_measured']):.3f}; K = {K:g})")


# --------------------------------------------------------------------------- 2. the sides swapped
def test_the_sides_swapped_give_the_same_members_and_hold_the_rule():
    """``b, a`` with the cell columns transposed on ``wide``: the streamed side and the lanes change places, and so do the ends
    ``a`` and ``b`` of every pair term. The diagonal rule rests on this."""
    fx = pse.fixture()
    ab, ba = run(fx, "wide", "two", False), run(fx, "wide", "two", False, swap=True)
    weighted = run(fx, "wide", "two", True, swap=True)
    for edges in pse.PI_SETS:
        exp = pse.expected(fx, "wide", "two", edges)
        assert np.array_equal(ba[edges][0][3], ab[edges][0][3]) and np.array_equal(ba[edges][0][3], exp["N"])
        pse.check(f"device wide two {edges} swapped", weighted[edges][0], exp, float(fx["K"]))


# --------------------------------------------------------------------------- 3. unwindowed
def test_the_whole_segment_streamed_gives_the_same_members_and_holds_the_rule():
    """``wide`` with the two handles on different sort axes: no window, every pair of a cell evaluated."""
    fx = pse.fixture()
    windowed, whole, unit = run(fx, "wide", "two", True, 2, 2), run(fx, "wide", "two", True, 2, 0), run(fx, "wide", "two", False, 2, 0)
    for edges in pse.PI_SETS:
        exp = pse.expected(fx, "wide", "two", edges)
        assert whole[edges][1].evaluated_pairs == whole[edges][1].candidate_pairs >= windowed[edges][1].evaluated_pairs > 0
        assert unit[edges][1].evaluated_pairs == unit[edges][1].candidate_pairs
        assert np.array_equal(unit[edges][0][3], exp["N"]) and np.array_equal(whole[edges][0][3] > 0, exp["N"] > 0)
        pse.check(f"device wide two {edges} unwindowed", whole[edges][0], exp, float(fx["K"]))


# --------------------------------------------------------------------------- 4. the known answer
@pytest.mark.parametrize("variant", pse.VARIANTS)
def test_isolated_pairs_give_the_known_answer(variant):
    """Shapes along the great circle that joins them (``along``: PP = sum w_a w_b e^2), both turned by 45 degrees (``both``: XX)
    or the first of the two (``one``: PX, positive), the pair next to the pole and the one across the wrap among them: held to
    the exact planes by the rule and to the closed form ``e^2 W`` within its bound, as diagonal cells and against an uploaded
    copy (every pair twice)."""
    fx = pse.fixture()
    K = float(fx["K"])
    holds = pse.SIGNED[pse.VARIANTS.index(variant)]
    diagonal, copied = run(fx, "pairs", variant), run(fx, "pairs", variant, copy=True)
    for edges in pse.PI_SETS:
        exp = pse.expected(fx, "pairs", variant, edges)
        for label, factor, got in (("diagonal", 1.0, diagonal[edges]), ("against a copy", 2.0, copied[edges])):
            planes, stats, _ = got
            scaled = {plane: factor * value for plane, value in exp.items()}
            assert stats.candidate_pairs == (2 * 12 * 11 // 2 if factor == 1.0 else 2 * 12 * 12)
            pse.check(f"device pairs {variant} {edges} {label}", planes, scaled, K)
            known, bound = 0.01 * scaled["W"], pse.bound(scaled, K)
            for ours, plane in zip(planes, pse.SIGNED):
                assert np.all(np.abs(ours - (known if plane == holds else 0.0)) <= bound), (variant, edges, label, plane)
            assert np.all(planes[pse.SIGNED.index(holds)][exp["N"] > 0] > 0.0) and exp["N"][:, 0].sum() == 6  # (the first cell holds the pole and the wrap)
