"""GPU: the projected position-shape count (``yawhip_proj_count_shear``) on the device against the exact reference of
tests/golden/proj_shear_exact.npz (tools/make_golden_proj_shear_exact.py: mpmath, the exact angle, radius and line-of-sight
separation for the membership and the exact bearing for the rotation -- not the contract's series or its algebra): a scene at
0.5 to 30 arcseconds at dec 0, 60, +-89.99 degrees and across the wrap of the right ascension, and one from 3 arcmin to 5.6
degrees (over the pole, across the wrap) whose nearest objects reach the cap of 0.01.

With unit weights ``W`` is the integer pair count ``N`` of the file, bit for bit; with the file's weights ``T`` and ``X`` hold
``|ours - exact| <= K 2^-52 A_theta + 1e-13 A`` per pi bin, cell and fine bin with the ``K`` of the file, and every plane is ``+0.0``
where the reference is empty. Every case prints its worst ratio. A few hundred objects per call; nothing here reads mpmath."""
import numpy as np
import pytest

import proj_shear_exact as pse
from test_gpu_projected import upload
from test_gpu_projected_shear import upload_shapes
from yet_another_wizz_amd import _lib, engine

pytestmark = pytest.mark.gpu


def run(fx, scene, weighted, axis_d, axis_s):
    """The count of the three edge sets on one upload -> ``{edge set: ((T, X, W), stats)}``."""
    ctx = engine.get_context(0)
    cells, r2 = fx[f"{scene}.cells"], fx[f"{scene}.r2"]
    dens = upload(ctx, pse.catalogue(fx, scene, "dens", weighted), axis_d)
    shapes = upload_shapes(ctx, pse.catalogue(fx, scene, "shapes", weighted), axis_s)
    try:
        out = {edges: _lib.proj_count_shear(ctx, dens, shapes, cells, r2, fx[f"pi.{edges}"]) for edges in pse.PI_SETS}
    finally:
        dens.free(), shapes.free()
    for _, stats in out.values():
        assert stats.n_workgroups == len(cells) and 0 < stats.evaluated_pairs <= stats.candidate_pairs
    return out


@pytest.mark.parametrize("sort_axis", [0, 1, 2])
@pytest.mark.parametrize("scene", pse.SCENES)
def test_membership_and_sums_are_the_exact_ones(scene, sort_axis):
    fx = pse.fixture()
    K = float(fx["K"])
    unit, weighted = run(fx, scene, False, sort_axis, sort_axis), run(fx, scene, True, sort_axis, sort_axis)
    worst = 0.0
    for edges in pse.PI_SETS:
        exp = pse.expected(fx, scene, edges)
        N = unit[edges][0][2]
        assert exp["N"].sum() > 1000 and np.array_equal(N, exp["N"]), (scene, edges, np.abs(N - exp["N"]).sum())
        worst = max(worst, pse.check(f"device {scene} {edges} axis={sort_axis}", weighted[edges][0], exp, K))
    print(f"device {scene} axis={sort_axis}: worst ratio {worst:.3f} (the numpy oracle's: {float(fx['K_measured']):.3f})")


def test_the_whole_segment_streamed_gives_the_windowed_bits():
    """``wide`` with the two handles on different sort axes: no window, every pair of a cell evaluated, the same members and the rule."""
    fx = pse.fixture()
    windowed, whole = run(fx, "wide", True, 2, 2), run(fx, "wide", True, 2, 0)
    for edges in pse.PI_SETS:
        assert whole[edges][1].evaluated_pairs == whole[edges][1].candidate_pairs >= windowed[edges][1].evaluated_pairs > 0
        assert np.array_equal(whole[edges][0][2] > 0, pse.expected(fx, "wide", edges)["N"] > 0)
        pse.check(f"device wide {edges} unwindowed", whole[edges][0], pse.expected(fx, "wide", edges), float(fx["K"]))
