"""CPU: the projected shape-shape correlation (``autocorrelate_alignment``, ``ShapeShapeCorrFunc``)
above the device seam -- the new name of the C ABI, the driver with ``engine.count_projected_shapes_fine`` replaced by the
oracle of tests/proj_shape_oracle.py against a brute force straight from the definitions (trigonometric angles and position
angles at both ends, one object at a time in numpy), the jackknife samples against leave-one-patch-out recomputation, the
error cases, the result class and the LDS formula of include/yawhip.h."""
import ctypes
import os
import re

import numpy as np
import pytest

import proj_oracle
import proj_pi_oracle
import proj_shape_oracle
import yet_another_wizz_amd as yaw
from conftest import ROOT
from helpers import use_oracle_engine
from shear_oracle import position_angle
from test_alignment_host import PI_EDGES, PI_MAX, RMAX, RMIN, RTOL_SUM, catalog, columns, config, leave_one_out, weight_sums
from test_projected_host import NEIGHBOURS, ZEDGES
from yet_another_wizz_amd import _lib, engine, parallel
from yet_another_wizz_amd.coordinates import radec_to_xyz


@pytest.fixture
def stand_in(monkeypatch):
    monkeypatch.setattr(engine, "count_projected_shapes_fine", proj_shape_oracle.count_projected_shapes_fine)
    monkeypatch.setattr(engine, "count_projected_pi_fine", proj_pi_oracle.count_projected_pi_fine)
    monkeypatch.setattr(engine, "count_projected_fine", proj_oracle.count_projected_fine)
    use_oracle_engine(monkeypatch)


def scenario(shape_rand=False):
    cols = dict(shapes=columns(3, 70, shear=True))
    if shape_rand:
        cols["shape_rand"] = columns(11, 100, weighted=False)
    return cols


# --------------------------------------------------------------------------- 1. ABI
def test_the_new_symbol_is_declared_bound_and_built_at_abi_6():
    text = open(os.path.join(ROOT, "include", "yawhip.h")).read()
    code = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    lib = ctypes.CDLL(_lib.LIB_PATH)
    assert "yawhip_proj_count_shapes" in _lib.ABI_SYMBOLS and hasattr(lib, "yawhip_proj_count_shapes")
    assert re.search(r"\bint yawhip_proj_count_shapes\s*\((.*?)\);", code, flags=re.S)
    assert re.search(r"#define YAWHIP_ABI_VERSION 6\b", text)
    bound = _lib.load_library()
    assert bound.yawhip_proj_count_shapes.argtypes == bound.yawhip_proj_count_pi.argtypes
    assert callable(_lib.proj_count_shapes) and callable(engine.count_projected_shapes_fine)
    assert callable(yaw.PatchLinkage.count_shape_pairs)
    for name in ("autocorrelate_alignment", "ShapeShapeCorrFunc"):
        assert name in yaw.__all__
    assert yaw.ShapeShapeCorrFunc is yaw.corrfunc.ShapeShapeCorrFunc


# --------------------------------------------------------------------------- 2. the driver against the definitions
def brute_force(cfg, shapes, pi_edges, centres=NEIGHBOURS):
    """``(PP, XX, PX, W, A)`` f64[S, n_pi, B, P, P] of every unordered pair of ``shapes`` from the definitions: the angle
    ``theta = 2 asin(chord / 2)``, ``r_p = (d_a + d_b) / 2 theta`` with the comoving transverse distance ``d = chi`` of the flat
    cosmology, ``pi = |chi_a - chi_b|``, at EITHER end the position angle ``phi`` of the partner seen from the shape by
    spherical trigonometry, ``e+ = g1 cos 2 phi + g2 sin 2 phi`` and ``ex = g1 sin 2 phi - g2 cos 2 phi``, and the products
    ``w_a w_b e+_a e+_b``, ``w_a w_b ex_a ex_b``, ``w_a w_b (e+_a ex_b + ex_a e+_b)``; redshift bins ``(z_k, z_k+1]``, an
    object in the patch of its nearest centre. A pair of the patches p, q sits in the slot ``[min, max]``: the upper triangle
    of an auto count. Without ``g1``: zeros (the pair counts of randoms are W)."""
    n_patches, centres = len(centres), np.stack(radec_to_xyz(*np.array(centres).T), axis=1)
    xyz = np.stack(radec_to_xyz(shapes["ra"], shapes["dec"]), axis=1)
    patch = np.argmin(((xyz[:, None, :] - centres[None]) ** 2).sum(axis=-1), axis=1)
    zbin = np.digitize(shapes["redshifts"], ZEDGES, right=True) - 1
    chi = np.asarray(cfg.cosmology.comoving_distance(shapes["redshifts"]), dtype=np.float64)
    w = shapes.get("weights", np.ones(len(xyz)))
    g1, g2 = shapes.get("g1", np.zeros(len(xyz))), shapes.get("g2", np.zeros(len(xyz)))
    ra, dec = shapes["ra"], shapes["dec"]
    out = np.zeros((5, len(RMIN), len(pi_edges) - 1, len(ZEDGES) - 1, n_patches, n_patches))
    for i in range(len(xyz) - 1):
        o = slice(i + 1, None)  # the partners with a larger index: every unordered pair once
        chord = np.sqrt(((xyz[o] - xyz[i]) ** 2).sum(axis=1))
        rp = 0.5 * (chi[o] + chi[i]) * 2.0 * np.arcsin(0.5 * chord)
        pi = np.abs(chi[o] - chi[i])
        phi_o = position_angle(ra[o], dec[o], ra[i], dec[i])  # of i seen from each partner
        phi_i = position_angle(ra[i], dec[i], ra[o], dec[o])  # of each partner seen from i
        plus_o, cross_o = g1[o] * np.cos(2 * phi_o) + g2[o] * np.sin(2 * phi_o), g1[o] * np.sin(2 * phi_o) - g2[o] * np.cos(2 * phi_o)
        plus_i, cross_i = g1[i] * np.cos(2 * phi_i) + g2[i] * np.sin(2 * phi_i), g1[i] * np.sin(2 * phi_i) - g2[i] * np.cos(2 * phi_i)
        ww = w[i] * w[o]
        terms = (ww * plus_i * plus_o, ww * cross_i * cross_o, ww * (plus_i * cross_o + cross_i * plus_o), ww,
                 ww * (np.abs(g1[i]) + np.abs(g2[i])) * (np.abs(g1[o]) + np.abs(g2[o])))
        j = (pi[:, None] > pi_edges[None, 1:]).sum(axis=1)
        lo, hi = np.minimum(patch[i], patch[o]), np.maximum(patch[i], patch[o])
        for s in range(len(RMIN)):
            keep = np.flatnonzero((zbin[o] == zbin[i]) & (j < len(pi_edges) - 1) & (rp > RMIN[s]) & (rp <= RMAX[s]))
            for c, term in enumerate(terms):
                np.add.at(out[c, s], (j[keep], zbin[i], lo[keep], hi[keep]), term[keep])
    return out


def auto_norm(sums):
    """[1 + P, 1, B] the normalisation of an auto count from the weight sums [B, P]: the upper triangle of their outer product
    with half the diagonal, for all patches and without each."""
    norm = np.triu(sums[:, :, None] * sums[:, None, :])
    idx = np.arange(norm.shape[-1])
    norm[:, idx, idx] *= 0.5
    return leave_one_out(norm)[:, None, :]


def check_driver(cols, centres=NEIGHBOURS, cats=None):
    """``autocorrelate_alignment`` on the catalogues of ``cols`` against ``brute_force``: every plane per slot under the
    weighted-sum rule, ``sample_xi`` and ``sample`` for the data and every jackknife sample under the bound that rule gives
    them. ``engine.count_projected_shapes_fine`` is whatever the caller left in place. Returns the result."""
    with_rand = "shape_rand" in cols
    cats = {name: catalog(c, centres) for name, c in cols.items()} if cats is None else cats
    cfg = config()
    result = yaw.autocorrelate_alignment(cfg, cats["shapes"], cats.get("shape_rand"), pi_max=PI_MAX, pi_bins=PI_EDGES)
    assert len(result) == len(RMIN)
    SS = brute_force(cfg, cols["shapes"], PI_EDGES, centres)
    n_ss = auto_norm(weight_sums(cols["shapes"], centres))
    if with_rand:
        RR = brute_force(cfg, cols["shape_rand"], PI_EDGES, centres)[3]
        n_rr = auto_norm(weight_sums(cols["shape_rand"], centres))
    for s, cf in enumerate(result):
        assert type(cf) is yaw.ShapeShapeCorrFunc and cf.num_pi == 3 and np.array_equal(cf.pi_edges, PI_EDGES)
        assert ("rr" in cf.pi_bins[0]) == with_rand
        for j, planes in enumerate(cf.pi_bins):
            assert all(planes[k].auto and planes[k].sum_weights is cf.pi_bins[0]["pp"].sum_weights for k in ("pp", "xx", "px", "w"))  # ONE normalisation
            assert np.count_nonzero(SS[4, s, j]) > 2 * len(centres)  # pairs across the patch borders
            assert not np.tril(SS[4, s, j], -1).any()  # the upper triangle
            for c, (plane, sign) in enumerate((("pp", 1.0), ("xx", 1.0), ("px", -1.0))):  # px holds et = -e+ once
                assert np.all(np.abs(sign * planes[plane].counts.counts - SS[c, s, j]) <= RTOL_SUM * SS[4, s, j]), (plane, s, j)
            np.testing.assert_allclose(planes["w"].counts.counts, SS[3, s, j], rtol=RTOL_SUM, atol=0)
            if with_rand:
                np.testing.assert_allclose(planes["rr"].counts.counts, RR[s, j], rtol=RTOL_SUM, atol=0)
        norm, n_norm = (leave_one_out(RR[s]), n_rr) if with_rand else (leave_one_out(SS[3, s]), n_ss)
        for component, c in (("plus", 0), ("cross", 1), ("plus_cross", 2)):
            xi = (leave_one_out(SS[c, s]) / n_ss) / (norm / n_norm)  # [1 + P, n_pi, B]
            w = 2.0 * np.tensordot(np.diff(PI_EDGES), xi, axes=(0, 1))
            # the numerator is held to RTOL_SUM of its magnitude A, the pair count to RTOL_SUM of itself
            bound_xi = 4.0 * RTOL_SUM * (leave_one_out(SS[4, s]) / n_ss) / (norm / n_norm)
            bound_w = 2.0 * np.tensordot(np.diff(PI_EDGES), bound_xi, axes=(0, 1))
            got_xi, got = cf.sample_xi(component), cf.sample(component)
            for j in range(3):
                assert np.all(np.abs(got_xi[j].data - xi[0, j]) <= bound_xi[0, j]) and np.all(np.abs(got_xi[j].samples - xi[1:, j]) <= bound_xi[1:, j])
            assert np.all(np.isfinite(w)) and np.all(np.abs(w[0]) > 100.0 * bound_w[0])  # a signal far above the bound
            assert np.all(np.abs(got.data - w[0]) <= bound_w[0]), (component, s)
            assert np.all(np.abs(got.samples - w[1:]) <= bound_w[1:]), (component, s)  # the jackknife: recomputed without a patch
    return result


@pytest.mark.parametrize("with_rand", [False, True])
def test_the_driver_gives_the_shape_shape_correlation_of_the_definitions(stand_in, with_rand):
    check_driver(scenario(with_rand))


def test_one_bin_is_the_default_and_a_rotation_by_45_degrees_swaps_the_components(stand_in):
    cols = scenario()["shapes"]
    cfg = config()
    run = lambda shapes, **kwargs: yaw.autocorrelate_alignment(cfg, catalog(shapes), pi_max=PI_MAX, **kwargs)  # noqa: E731
    base = run(cols)
    assert all(cf.num_pi == 1 and np.array_equal(cf.pi_edges, [0.0, PI_MAX]) for cf in base)
    assert base == run(cols, pi_bins=1) and base == run(cols, pi_bins=[0.0, PI_MAX])
    turned = run(dict(cols, g1=-cols["g2"], g2=cols["g1"]))  # (g1, g2) -> (-g2, g1) at both ends: e+' = -ex, ex' = e+
    for cf, rot in zip(base, turned):
        for got, exp, sign in (("plus", "cross", 1.0), ("cross", "plus", 1.0), ("plus_cross", "plus_cross", -1.0)):
            assert np.array_equal(rot.sample(got).data, sign * cf.sample(exp).data)  # the oracle's products are bit-symmetric too
            assert np.array_equal(rot.sample(got).samples, sign * cf.sample(exp).samples)
    # a second shape sample: all patch pairs, the same pairs as the auto count when it holds the same objects
    first, second = catalog(cols), catalog(cols)
    links = yaw.PatchLinkage.from_catalogs(cfg, first, second)
    for cat in (first, second):
        cat.build_trees(ZEDGES, with_shear=True, with_redshifts=True)
    auto = links.count_shape_pairs(first, pi_max=PI_MAX, pi_bins=PI_EDGES)
    cross = links.count_shape_pairs(first, second, pi_max=PI_MAX, pi_bins=PI_EDGES)
    for per_pi_auto, per_pi_cross in zip(auto, cross):
        for planes_auto, planes_cross in zip(per_pi_auto, per_pi_cross):
            for one, two in zip(planes_auto, planes_cross):
                assert one.auto and not two.auto
                total, both = one.counts.counts.sum(axis=(1, 2)), two.counts.counts.sum(axis=(1, 2))
                np.testing.assert_allclose(both, 2.0 * total, rtol=1e-9, atol=1e-18)  # every unordered pair twice; no pair with itself


# --------------------------------------------------------------------------- 3. refusals
def test_the_driver_refuses_what_it_cannot_measure(stand_in, monkeypatch):
    cols = scenario(shape_rand=True)
    shapes, rand = catalog(cols["shapes"]), catalog(cols["shape_rand"])
    cfg = config()
    call = lambda *cats, **kw: yaw.autocorrelate_alignment(cfg, *cats, **dict(dict(pi_max=PI_MAX), **kw))  # noqa: E731
    with pytest.raises(ValueError, match="radi|unit"):  # an angular unit has no radius
        yaw.autocorrelate_alignment(yaw.Configuration.create(rmin=1.0, rmax=10.0, unit="arcmin", edges=ZEDGES), shapes, rand, pi_max=PI_MAX)
    with pytest.raises(ValueError, match="redshift"):
        call(shapes, catalog(columns(11, 100, weighted=False, redshifts=False)))
    with pytest.raises(ValueError, match="redshift"):
        call(catalog(columns(3, 70, shear=True, redshifts=False)))
    with pytest.raises(ValueError, match="g1"):
        call(catalog(columns(3, 70)), rand)
    with pytest.raises(ValueError, match="separate Catalog"):
        call(shapes, shapes)
    with pytest.raises(TypeError):
        yaw.autocorrelate_alignment(cfg, shapes)  # pi_max has no default
    for bad in (dict(pi_max=0.0), dict(pi_max=np.inf), dict(pi_bins=0), dict(pi_bins=[0.0, 30.0]), dict(pi_bins=[1.0, PI_MAX])):
        with pytest.raises(ValueError):
            call(shapes, rand, **bad)
    links = yaw.PatchLinkage.from_catalogs(cfg, shapes, rand)
    shapes.build_trees(ZEDGES, with_redshifts=True)  # the layout without shear
    with pytest.raises(ValueError, match="with_shear"):
        links.count_shape_pairs(shapes, pi_max=PI_MAX)
    rand.build_trees(ZEDGES, with_redshifts=True)
    shapes.build_trees(ZEDGES, with_shear=True, with_redshifts=True)
    with pytest.raises(ValueError, match="with_shear"):  # either side
        links.count_shape_pairs(shapes, rand, pi_max=PI_MAX)
    with pytest.raises(ValueError, match="g1"):  # the seam itself, and the engine's own function before it touches a device
        proj_shape_oracle.count_projected_shapes_fine(shapes._active_layout, rand._active_layout, np.zeros((0, 4), dtype=np.int32),
                                                      np.array([[0.0, 1.0]]), pi_edges=PI_EDGES, cosmology=cfg.cosmology, unit=cfg.scales.scales.unit)
    monkeypatch.undo()
    with pytest.raises(ValueError, match="g1"):
        engine.count_projected_shapes_fine(shapes._active_layout, rand._active_layout, np.zeros((0, 4), dtype=np.int32),
                                           np.array([[0.0, 1.0]]), pi_edges=PI_EDGES, cosmology=cfg.cosmology, unit=cfg.scales.scales.unit)
    monkeypatch.setattr(parallel, "world", lambda: (0, 2))
    with pytest.raises(NotImplementedError):
        call(shapes, rand)
    with pytest.raises(NotImplementedError):
        links.count_shape_pairs(shapes, pi_max=PI_MAX)


def lds_bytes(n_edges, n_pi):
    """The formula of include/yawhip.h for yawhip_proj_count_shapes."""
    return 32768 + 8 * (((n_edges + 1) & ~1) + ((n_pi + 2) & ~1)) + 128 * n_pi * (n_edges - 1)


def test_the_lds_formula_of_the_header_gives_the_caps_it_quotes_and_the_engine_states_them(stand_in, monkeypatch):
    text = open(os.path.join(ROOT, "include", "yawhip.h")).read()
    contract = text[text.index("yawhip_proj_count_shapes  "):]
    assert "32768 + 8 (((n_edges + 1) & ~1) + ((n_pi + 2) & ~1)) + 128 n_pi (n_edges - 1) <= 65536" in contract
    quoted = re.search(r"n_pi <= (\d+) at 13 edges, <= (\d+) at 51, <= (\d+) at 241, <= (\d+) at 2;", contract)
    assert quoted and [int(v) for v in quoted.groups()] == [21, 5, 1, 240]
    for n_edges, cap in ((13, 21), (51, 5), (241, 1), (2, 240)):
        assert lds_bytes(n_edges, cap) <= 65536 < lds_bytes(n_edges, cap + 1) and engine.max_shape_pi_bins(n_edges) == cap
    assert lds_bytes(242, 1) > 65536 and engine.max_shape_pi_bins(242) == engine.max_shape_pi_bins(256) == 0

    # pi_bins over the cap: a ValueError with the cap in it from the driver (12 fine bins at this configuration's resolution) ...
    shapes = catalog(scenario()["shapes"])
    cfg = config()
    n_edges = np.shape(yaw.measurements.threshold_table(yaw.measurements.radial_plans(cfg)))[1]
    cap = engine.max_shape_pi_bins(n_edges)
    assert len(yaw.autocorrelate_alignment(cfg, shapes, pi_max=PI_MAX, pi_bins=cap)[0].pi_bins) == cap
    with pytest.raises(ValueError, match=f"{cap + 1} pi bins are too many for {n_edges} radius edges.*at most {cap} pi bins fit"):
        yaw.autocorrelate_alignment(cfg, shapes, pi_max=PI_MAX, pi_bins=cap + 1)
    # ... and from the engine's own function, before anything reaches the library or a device
    monkeypatch.undo()
    layout = shapes.build_trees(ZEDGES, with_shear=True, with_redshifts=True)
    monkeypatch.setattr(engine, "get_context", lambda *a, **k: pytest.fail("the cap is checked before the device is asked for"))
    monkeypatch.setattr(_lib, "proj_count_shapes", lambda *a, **k: pytest.fail("the cap is checked before the library is called"))
    kwargs = dict(cosmology=cfg.cosmology, unit=cfg.scales.scales.unit)
    with pytest.raises(ValueError, match="at most 21 pi bins fit"):
        engine.count_projected_shapes_fine(layout, layout, np.zeros((1, 4), dtype=np.int32), np.zeros((2, 13)), pi_edges=np.linspace(0.0, PI_MAX, 23), **kwargs)
    with pytest.raises(ValueError, match="at most 5 pi bins fit"):
        engine.count_projected_shapes_fine(layout, layout, np.zeros((1, 4), dtype=np.int32), np.zeros((2, 51)), pi_edges=np.linspace(0.0, PI_MAX, 7), **kwargs)
    with pytest.raises(ValueError, match="not even one pi bin fits above 241 radius edges"):
        engine.count_projected_shapes_fine(layout, layout, np.zeros((1, 4), dtype=np.int32), np.zeros((2, 256)), pi_edges=np.array([0.0, PI_MAX]), **kwargs)


def test_the_engine_passes_one_resident_shape_handle_twice_and_reuses_the_one_of_w_g_plus(monkeypatch):
    """The handles are those of ``count_projected_shear_fine`` (role "projected shapes <kind>"): same cache key, no second
    upload; one layout on both sides is ONE handle, and only then cells may be diagonal."""
    cols = scenario()
    first, second, density = catalog(cols["shapes"]), catalog(cols["shapes"]), catalog(columns(5, 60))
    cfg = config()
    layouts = [cat.build_trees(ZEDGES, with_shear=True, with_redshifts=True) for cat in (first, second)]
    dens_layout = density.build_trees(ZEDGES, with_redshifts=True)
    uploads, calls = [], []
    monkeypatch.setattr(engine, "get_context", lambda *a, **k: ctx)
    ctx = object()
    monkeypatch.setattr(_lib, "ProjShapesHandle", lambda c, *args, sort_axis=2, **kw: uploads.append("shapes") or type("H", (), dict(sort_axis=sort_axis, _h=1, free=lambda self: None))())
    monkeypatch.setattr(_lib, "ProjHandle", lambda c, *args, sort_axis=2, **kw: uploads.append("plain") or type("H", (), dict(sort_axis=sort_axis, _h=1, free=lambda self: None))())
    monkeypatch.setattr(_lib, "proj_count_shear", lambda c, dens, shapes, *a: calls.append((dens, shapes)) or ((), None))
    monkeypatch.setattr(_lib, "proj_count_shapes", lambda c, a, b, *rest: calls.append((a, b)) or ((), None))
    kwargs = dict(pi_edges=PI_EDGES, cosmology=cfg.cosmology, unit=cfg.scales.scales.unit)
    cells, r2 = np.zeros((1, 4), dtype=np.int32), np.zeros((2, 13))
    engine.count_projected_shear_fine(dens_layout, layouts[0], cells, r2, **kwargs)  # w_g+ uploads the shapes ...
    assert uploads == ["plain", "shapes"]
    engine.count_projected_shapes_fine(layouts[0], layouts[0], cells, r2, **kwargs)  # ... and w_++ finds them there
    assert uploads == ["plain", "shapes"] and calls[1][0] is calls[1][1] is calls[0][1]
    engine.count_projected_shapes_fine(layouts[0], layouts[1], cells, r2, **kwargs)
    assert uploads == ["plain", "shapes", "shapes"] and calls[2][0] is calls[0][1] and calls[2][1] is not calls[2][0]
    engine.count_projected_shapes_fine(layouts[1], layouts[0], cells, r2, **kwargs)
    assert len(uploads) == 3 and calls[3] == calls[2][::-1]


# --------------------------------------------------------------------------- 4. the result class
def test_shape_shape_corrfunc_round_trip_equality_subsets_and_nan(stand_in):
    cols = scenario(shape_rand=True)
    cf = yaw.autocorrelate_alignment(config(), catalog(cols["shapes"]), catalog(cols["shape_rand"]), pi_max=PI_MAX, pi_bins=PI_EDGES)[0]
    again = yaw.ShapeShapeCorrFunc.from_dict(cf.to_dict())
    assert again == cf and again is not cf and cf.is_compatible(again, require=True)
    assert cf.num_bins == 2 and cf.num_patches == 3 and cf.binning == cf.pi_bins[0]["w"].binning and "num_pi=3" in repr(cf)
    state = cf.to_dict()
    state["pi_bins"][1] = dict(state["pi_bins"][1], xx=state["pi_bins"][1]["pp"])
    assert yaw.ShapeShapeCorrFunc.from_dict(state) != cf
    other_edges = yaw.ShapeShapeCorrFunc([0.0, 10.0, 25.0, 50.0], cf.pi_bins)
    assert other_edges != cf and not cf.is_compatible(other_edges)
    with pytest.raises(ValueError, match="pi edges differ"):
        cf.is_compatible(other_edges, require=True)
    assert cf != 1 and not cf.is_compatible(1)
    without = yaw.ShapeShapeCorrFunc(cf.pi_edges, [{k: v for k, v in planes.items() if k != "rr"} for planes in cf.pi_bins])
    assert without != cf and not np.array_equal(without.sample().data, cf.sample().data)  # the denominator is W there
    # the two estimators differ by 1 + xi_gg: (w/n) / (rr/n) per pi bin
    for j, planes in enumerate(cf.pi_bins):
        clustering = planes["w"].sample_patch_sum().data / planes["rr"].sample_patch_sum().data
        np.testing.assert_allclose(cf.sample_xi("cross")[j].data, without.sample_xi("cross")[j].data * clustering, rtol=1e-12, atol=0)
    for bad_edges, bad_bins in (([0.0, 10.0], cf.pi_bins), ([1.0, 10.0, 25.0, 60.0], cf.pi_bins), (cf.pi_edges, [*cf.pi_bins[:2], without.pi_bins[2]]),
                                (cf.pi_edges, [{k: v for k, v in planes.items() if k != "px"} for planes in cf.pi_bins])):
        with pytest.raises(ValueError):
            yaw.ShapeShapeCorrFunc(bad_edges, bad_bins)
    with pytest.raises(TypeError):
        yaw.ShapeShapeCorrFunc(cf.pi_edges, [dict(planes, pp=planes["pp"].counts) for planes in cf.pi_bins])
    with pytest.raises(ValueError, match="component"):
        cf.sample("minus")
    # the other result class of the pi bins is another type
    assert cf != yaw.AlignmentCorrFunc and not cf.is_compatible(object())
    # subsets go bin by bin
    one_bin, two_patches = cf.bins_subset(1), cf.patches_subset([0, 2])
    assert type(one_bin) is yaw.ShapeShapeCorrFunc and one_bin.num_bins == 1 and two_patches.num_patches == 2 and one_bin.num_pi == two_patches.num_pi == 3
    np.testing.assert_array_equal(one_bin.sample("cross").data, cf.sample("cross").data[1:])
    for j in range(3):
        assert two_patches.pi_bins[j]["pp"] == cf.pi_bins[j]["pp"].patches_subset([0, 2])
    # the sum over the pi bins, by hand
    for component in ("plus", "cross", "plus_cross"):
        xi = cf.sample_xi(component)
        by_hand = 2.0 * sum(dpi * x.data for dpi, x in zip(np.diff(PI_EDGES), xi))
        np.testing.assert_allclose(cf.sample(component).data, by_hand, rtol=1e-14, atol=0)
    # an empty RR: NaN in that pi bin and in the sum, the other redshift bin untouched
    emptied = [dict(planes) for planes in cf.pi_bins]
    counts = emptied[1]["rr"].counts.counts.copy()
    counts[0] = 0.0
    emptied[1]["rr"] = yaw.NormalisedCounts(yaw.PatchedCounts(cf.binning, counts, auto=True), emptied[1]["rr"].sum_weights)
    holed = yaw.ShapeShapeCorrFunc(cf.pi_edges, emptied)
    for component in ("plus", "cross", "plus_cross"):
        xi = holed.sample_xi(component)
        assert np.isnan(xi[1].data[0]) and np.all(np.isnan(xi[1].samples[:, 0])) and np.isfinite(xi[1].data[1])
        assert np.all(np.isfinite(xi[0].data)) and np.all(np.isfinite(xi[2].data))
        total = holed.sample(component)
        assert np.isnan(total.data[0]) and np.all(np.isnan(total.samples[:, 0]))
        assert total.data[1] == cf.sample(component).data[1]
