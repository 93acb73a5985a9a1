"""CPU: the projected position-shape correlation (``crosscorrelate_alignment``, ``AlignmentCorrFunc``)
above the device seam -- the two new names of the C ABI, the driver with ``engine.count_projected_shear_fine`` replaced by
the oracle of tests/proj_shear_oracle.py against a brute force straight from the definitions (trigonometric angles and
position angles, one pair at a time in numpy), the jackknife samples against leave-one-patch-out recomputation, the error
cases, the result class and the LDS formula of include/yawhip.h."""
import ctypes
import os
import re

import numpy as np
import pytest

import proj_oracle
import proj_pi_oracle
import proj_shear_oracle
import yet_another_wizz_amd as yaw
from conftest import ROOT
from helpers import use_oracle_engine
from shear_oracle import position_angle
from test_projected_host import NEIGHBOURS, ZEDGES
from test_shear_host import ring_around
from yet_another_wizz_amd import _lib, engine, parallel
from yet_another_wizz_amd.coordinates import radec_to_xyz

RTOL_SUM = 1e-10  # the project's tolerance of a weighted sum, relative to its cancellation-free magnitude (helpers.RTOL_W)
PI_MAX = 60.0
PI_EDGES = np.array([0.0, 10.0, 25.0, 60.0])
RMIN, RMAX = (0.15, 0.4), (2.8, 1.5)  # Mpc/h: comoving radii


@pytest.fixture
def stand_in(monkeypatch):
    monkeypatch.setattr(engine, "count_projected_shear_fine", proj_shear_oracle.count_projected_shear_fine)
    monkeypatch.setattr(engine, "count_projected_pi_fine", proj_pi_oracle.count_projected_pi_fine)
    monkeypatch.setattr(engine, "count_projected_fine", proj_oracle.count_projected_fine)
    use_oracle_engine(monkeypatch)


def config():
    return yaw.Configuration.create(rmin=list(RMIN), rmax=list(RMAX), unit="Mpc/h", edges=ZEDGES)


def columns(seed, n, *, shear=False, weighted=True, redshifts=True, centres=NEIGHBOURS):
    """``n`` objects around each of the centres: dict(ra, dec[, redshifts, weights, g1, g2])."""
    rng = np.random.default_rng(seed)
    ra, dec = (np.concatenate(c) for c in zip(*(ring_around(rng, ra_c, dec_c, n, 1e-5, 1.8e-3) for ra_c, dec_c in centres)))
    cols = dict(ra=ra, dec=dec)
    if redshifts:
        cols["redshifts"] = rng.uniform(0.22, 0.58, len(ra))
    if weighted:
        cols["weights"] = rng.uniform(0.5, 1.5, len(ra))
    if shear:
        cols["g1"], cols["g2"] = rng.normal(0.01, 0.05, len(ra)), rng.normal(-0.02, 0.05, len(ra))
    return cols


def catalog(cols, centres=NEIGHBOURS):
    cols = dict(cols)
    return yaw.Catalog.from_arrays(cols.pop("ra"), cols.pop("dec"), patch_centers=yaw.AngularCoordinates(np.array(centres)), degrees=False,
                                   **cols)


def scenario(shape_rand=False):
    cols = dict(shapes=columns(3, 70, shear=True), density=columns(5, 60), density_rand=columns(7, 110, weighted=False))
    if shape_rand:
        cols["shape_rand"] = columns(11, 100, weighted=False)
    return cols


# --------------------------------------------------------------------------- 1. ABI
def test_the_new_symbols_are_declared_bound_and_built_at_abi_6():
    text = open(os.path.join(ROOT, "include", "yawhip.h")).read()
    code = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    lib = ctypes.CDLL(_lib.LIB_PATH)
    for name in ("yawhip_proj_upload_shapes", "yawhip_proj_count_shear"):
        assert name in _lib.ABI_SYMBOLS and hasattr(lib, name)
        assert re.search(rf"\bint {name}\s*\((.*?)\);", code, flags=re.S), name
    assert re.search(r"#define YAWHIP_ABI_VERSION 6\b", text)
    bound = _lib.load_library()
    assert bound.yawhip_proj_count_shear.argtypes == bound.yawhip_proj_count_pi.argtypes
    plain = bound.yawhip_proj_upload.argtypes
    assert bound.yawhip_proj_upload_shapes.argtypes == [*plain[:6], plain[6], plain[6], *plain[6:]]  # g1, g2 before d, c
    assert issubclass(_lib.ProjShapesHandle, _lib.ShearSources) and callable(_lib.proj_count_shear)
    assert callable(engine.count_projected_shear_fine)
    for name in ("crosscorrelate_alignment", "AlignmentCorrFunc"):
        assert name in yaw.__all__
    assert yaw.AlignmentCorrFunc is yaw.corrfunc.AlignmentCorrFunc


# --------------------------------------------------------------------------- 2. the driver against the definitions
def brute_force(cfg, shapes, density, pi_edges, centres=NEIGHBOURS):
    """``(T, X, W, A)`` f64[S, n_pi, B, P, P] of shapes about density objects from the definitions: the angle
    ``theta = 2 asin(chord / 2)``, ``r_p = (d_a + d_b) / 2 theta`` with the comoving transverse distance ``d = chi`` of the
    flat cosmology, ``pi = |chi_a - chi_b|``, the position angle ``phi`` of the density object seen from the shape by
    spherical trigonometry, ``e_t = -(g1 cos 2 phi + g2 sin 2 phi)`` and ``e_x = g1 sin 2 phi - g2 cos 2 phi``; redshift
    bins ``(z_k, z_k+1]``, an object in the patch of its nearest centre. Slot ``[p, q]``: density patch p, shape patch q."""
    n_patches, centres = len(centres), np.stack(radec_to_xyz(*np.array(centres).T), axis=1)

    def prepare(cols):
        xyz = np.stack(radec_to_xyz(cols["ra"], cols["dec"]), axis=1)
        patch = np.argmin(((xyz[:, None, :] - centres[None]) ** 2).sum(axis=-1), axis=1)
        zbin = np.digitize(cols["redshifts"], ZEDGES, right=True) - 1
        chi = np.asarray(cfg.cosmology.comoving_distance(cols["redshifts"]), dtype=np.float64)
        return xyz, patch, zbin, chi, cols.get("weights", np.ones(len(xyz)))

    sx, sp, sk, sc, sw = prepare(shapes)
    dx, dp, dk, dc, dw = prepare(density)
    out = np.zeros((4, len(RMIN), len(pi_edges) - 1, len(ZEDGES) - 1, n_patches, n_patches))
    for i in range(len(dx)):
        chord = np.sqrt(((sx - dx[i]) ** 2).sum(axis=1))
        rp = 0.5 * (sc + dc[i]) * 2.0 * np.arcsin(0.5 * chord)
        pi = np.abs(sc - dc[i])
        phi = position_angle(shapes["ra"], shapes["dec"], density["ra"][i], density["dec"][i])
        ww = dw[i] * sw
        et = -(shapes["g1"] * np.cos(2 * phi) + shapes["g2"] * np.sin(2 * phi))
        ex = shapes["g1"] * np.sin(2 * phi) - shapes["g2"] * np.cos(2 * phi)
        terms = (ww * et, ww * ex, ww, ww * (np.abs(shapes["g1"]) + np.abs(shapes["g2"])))
        j = (pi[:, None] > pi_edges[None, 1:]).sum(axis=1)
        for s in range(len(RMIN)):
            keep = np.flatnonzero((sk == dk[i]) & (j < len(pi_edges) - 1) & (rp > RMIN[s]) & (rp <= RMAX[s]))
            for c, term in enumerate(terms):
                np.add.at(out[c, s], (j[keep], dk[i], dp[i], sp[keep]), term[keep])
    return out


def weight_sums(cols, centres=NEIGHBOURS):
    """[B, P] sums of weights."""
    n_patches, centres = len(centres), np.stack(radec_to_xyz(*np.array(centres).T), axis=1)
    xyz = np.stack(radec_to_xyz(cols["ra"], cols["dec"]), axis=1)
    patch = np.argmin(((xyz[:, None, :] - centres[None]) ** 2).sum(axis=-1), axis=1)
    zbin = np.digitize(cols["redshifts"], ZEDGES, right=True) - 1
    sums = np.zeros((len(ZEDGES) - 1, n_patches))
    np.add.at(sums, (zbin, patch), cols.get("weights", np.ones(len(xyz))))
    return sums


def leave_one_out(arr):
    """[..., P, P] -> [1 + P, ...]: the sum over all patch pairs, then without every pair that touches patch m."""
    P = arr.shape[-1]
    keeps = [np.arange(P)] + [np.flatnonzero(np.arange(P) != m) for m in range(P)]
    return np.array([arr[..., keep, :][..., keep].sum(axis=(-2, -1)) for keep in keeps])


def estimate(sd, sr, n_sd, n_sr, norm, n_norm, sign):
    """``sign (sd / n_sd - sr / n_sr) / (norm / n_norm)`` [1 + P, n_pi, B] -> ``2 sum_j dpi_j`` of it [1 + P, B]."""
    xi = sign * (sd / n_sd - sr / n_sr) / (norm / n_norm)
    return xi, 2.0 * np.tensordot(np.diff(PI_EDGES), xi, axes=(0, 1))


def check_driver(cols, centres=NEIGHBOURS, cats=None):
    """``crosscorrelate_alignment`` on the catalogues of ``cols`` against ``brute_force``: every plane per slot under the
    weighted-sum rule, ``sample_xi`` and ``sample`` for the data and every jackknife sample under the bound that rule gives
    them. ``engine.count_projected_shear_fine`` is whatever the caller left in place. Returns the result."""
    with_shape_rand = "shape_rand" in cols
    cats = {name: catalog(c, centres) for name, c in cols.items()} if cats is None else cats
    cfg = config()
    result = yaw.crosscorrelate_alignment(cfg, cats["shapes"], cats["density"], cats["density_rand"], pi_max=PI_MAX, pi_bins=PI_EDGES,
                                          shape_rand=cats.get("shape_rand"))
    assert len(result) == len(RMIN)
    SD, SR = (brute_force(cfg, cols["shapes"], cols[name], PI_EDGES, centres) for name in ("density", "density_rand"))
    w_s, w_d, w_r = (weight_sums(cols[name], centres) for name in ("shapes", "density", "density_rand"))
    n_sd, n_sr = (leave_one_out(w[:, :, None] * w_s[:, None, :])[:, None, :] for w in (w_d, w_r))  # [1 + P, 1, B]
    if with_shape_rand:
        zeros = np.zeros(len(cols["shape_rand"]["ra"]))
        RR = brute_force(cfg, dict(cols["shape_rand"], g1=zeros, g2=zeros), cols["density_rand"], PI_EDGES, centres)[2]
        n_rr = leave_one_out(w_r[:, :, None] * weight_sums(cols["shape_rand"], centres)[:, None, :])[:, None, :]
    for s, cf in enumerate(result):
        assert type(cf) is yaw.AlignmentCorrFunc and cf.num_pi == 3 and np.array_equal(cf.pi_edges, PI_EDGES)
        assert ("rr" in cf.pi_bins[0]) == with_shape_rand
        for j, planes in enumerate(cf.pi_bins):
            for kind, exp in (("sd", SD), ("sr", SR)):
                assert planes[f"t_{kind}"].sum_weights is cf.pi_bins[0]["t_sd" if kind == "sd" else "t_sr"].sum_weights  # ONE normalisation
                assert np.count_nonzero(exp[3, s, j]) > 2 * len(centres)  # pairs across the patch borders
                for c, plane in enumerate("tx"):
                    assert np.all(np.abs(planes[f"{plane}_{kind}"].counts.counts - exp[c, s, j]) <= RTOL_SUM * exp[3, s, j]), (kind, plane, s, j)
                np.testing.assert_allclose(planes[f"w_{kind}"].counts.counts, exp[2, s, j], rtol=RTOL_SUM, atol=0)
            if with_shape_rand:
                np.testing.assert_allclose(planes["rr"].counts.counts, RR[s, j], rtol=RTOL_SUM, atol=0)
        norm, n_norm = (leave_one_out(RR[s]), n_rr) if with_shape_rand else (leave_one_out(SR[2, s]), n_sr)
        for component, c, sign in (("plus", 0, -1.0), ("cross", 1, 1.0)):
            xi, w = estimate(leave_one_out(SD[c, s]), leave_one_out(SR[c, s]), n_sd, n_sr, norm, n_norm, sign)
            # every sum is held to RTOL_SUM of its magnitude A, every pair count to RTOL_SUM of itself
            bound_xi = 4.0 * RTOL_SUM * (leave_one_out(SD[3, s]) / n_sd + leave_one_out(SR[3, s]) / n_sr) / (norm / n_norm)
            bound_w = 2.0 * np.tensordot(np.diff(PI_EDGES), bound_xi, axes=(0, 1))
            got_xi, got = cf.sample_xi(component), cf.sample(component)
            for j in range(3):
                assert np.all(np.abs(got_xi[j].data - xi[0, j]) <= bound_xi[0, j]) and np.all(np.abs(got_xi[j].samples - xi[1:, j]) <= bound_xi[1:, j])
            assert np.all(np.isfinite(w)) and np.all(np.abs(w[0]) > 100.0 * bound_w[0])  # a signal far above the bound
            assert np.all(np.abs(got.data - w[0]) <= bound_w[0]), (component, s)
            assert np.all(np.abs(got.samples - w[1:]) <= bound_w[1:]), (component, s)  # the jackknife: recomputed without a patch
    return result


@pytest.mark.parametrize("with_shape_rand", [False, True])
def test_the_driver_gives_the_alignment_of_the_definitions(stand_in, with_shape_rand):
    check_driver(scenario(with_shape_rand))


def test_one_bin_is_the_default_and_a_rotation_by_45_degrees_swaps_the_components(stand_in):
    cols = scenario()
    cfg = config()

    def run(shapes, **kwargs):
        cats = {name: catalog(c) for name, c in dict(cols, shapes=shapes).items()}
        return yaw.crosscorrelate_alignment(cfg, cats["shapes"], cats["density"], cats["density_rand"], pi_max=PI_MAX, **kwargs)

    base = run(cols["shapes"])
    assert all(cf.num_pi == 1 and np.array_equal(cf.pi_edges, [0.0, PI_MAX]) for cf in base)
    assert base == run(cols["shapes"], pi_bins=1) and base == run(cols["shapes"], pi_bins=[0.0, PI_MAX])
    turned = run(dict(cols["shapes"], g1=-cols["shapes"]["g2"], g2=cols["shapes"]["g1"]))  # (g1, g2) -> (-g2, g1)
    for cf, rot in zip(base, turned):
        plus, cross = cf.sample("plus"), cf.sample("cross")
        scale = np.abs(plus.data) + np.abs(cross.data)
        # T' = -(-g2 c2 + g1 s2p) = -X and X' = -g2 s2p - g1 c2 = T (include/yawhip.h); w_g+ is -T and w_gx is +X, so the
        # turned shapes have plus' = cross and cross' = -plus
        for got, exp in ((rot.sample("plus"), cross), (rot.sample("cross"), plus)):
            sign = -1.0 if exp is plus else 1.0
            np.testing.assert_allclose(got.data, sign * exp.data, rtol=0, atol=1e-12 * scale.max())
            np.testing.assert_allclose(got.samples, sign * exp.samples, rtol=0, atol=1e-12 * scale.max())


# --------------------------------------------------------------------------- 3. refusals
def test_the_driver_refuses_what_it_cannot_measure(stand_in, monkeypatch):
    cols = scenario()
    shapes, density, rand = (catalog(cols[name]) for name in ("shapes", "density", "density_rand"))
    cfg = config()
    call = lambda *cats, **kw: yaw.crosscorrelate_alignment(cfg, *cats, **dict(dict(pi_max=PI_MAX), **kw))  # noqa: E731
    with pytest.raises(ValueError, match="radi|unit"):  # an angular unit has no radius
        yaw.crosscorrelate_alignment(yaw.Configuration.create(rmin=1.0, rmax=10.0, unit="arcmin", edges=ZEDGES), shapes, density, rand, pi_max=PI_MAX)
    with pytest.raises(ValueError, match="redshift"):
        call(shapes, catalog(columns(5, 60, redshifts=False)), rand)
    with pytest.raises(ValueError, match="redshift"):
        call(catalog(columns(3, 70, shear=True, redshifts=False)), density, rand)
    with pytest.raises(ValueError, match="g1"):
        call(catalog(columns(3, 70)), density, rand)
    with pytest.raises(ValueError, match="separate Catalog"):
        call(shapes, density, density)
    with pytest.raises(ValueError, match="separate Catalog"):
        call(shapes, shapes, rand)
    for bad in (dict(pi_max=0.0), dict(pi_max=np.inf), dict(pi_bins=0), dict(pi_bins=[0.0, 30.0]), dict(pi_bins=[1.0, PI_MAX])):
        with pytest.raises(ValueError):
            call(shapes, density, rand, **bad)
    links = yaw.PatchLinkage.from_catalogs(cfg, shapes, density)
    density.build_trees(ZEDGES, with_redshifts=True)
    shapes.build_trees(ZEDGES, with_redshifts=True)  # the layout without shear
    with pytest.raises(ValueError, match="with_shear"):
        links.count_alignment_pairs(shapes, density, pi_max=PI_MAX)
    with pytest.raises(ValueError, match="g1"):  # the seam itself
        proj_shear_oracle.count_projected_shear_fine(density._active_layout, shapes._active_layout, np.zeros((0, 4), dtype=np.int32),
                                                     np.array([[0.0, 1.0]]), pi_edges=PI_EDGES, cosmology=cfg.cosmology, unit=cfg.scales.scales.unit)
    monkeypatch.setattr(parallel, "world", lambda: (0, 2))
    with pytest.raises(NotImplementedError):
        call(shapes, density, rand)
    with pytest.raises(NotImplementedError):
        links.count_alignment_pairs(shapes, density, pi_max=PI_MAX)


def lds_bytes(n_edges, n_pi):
    """The formula of include/yawhip.h for yawhip_proj_count_shear."""
    return 24576 + 8 * (((n_edges + 1) & ~1) + ((n_pi + 2) & ~1)) + 96 * n_pi * (n_edges - 1)


def test_the_lds_formula_of_the_header_gives_the_caps_it_quotes_and_the_engine_states_them(monkeypatch):
    text = open(os.path.join(ROOT, "include", "yawhip.h")).read()
    contract = text[text.index("yawhip_proj_upload_shapes  "):]
    assert "24576 + 8 (((n_edges + 1) & ~1) + ((n_pi + 2) & ~1)) + 96 n_pi (n_edges - 1) <= 65536" in contract
    quoted = re.search(r"n_pi <= (\d+) at 13 edges, <= (\d+) at 51, <= (\d+) at 256, <= (\d+) at 2\b", contract)
    assert quoted and [int(v) for v in quoted.groups()] == [35, 8, 1, 393]
    for n_edges, cap in ((13, 35), (51, 8), (256, 1), (2, 393)):
        assert lds_bytes(n_edges, cap) <= 65536 < lds_bytes(n_edges, cap + 1)

    # pi_bins over the cap: the library's refusal becomes the engine's ValueError with the cap in it
    def refuse(*args, **kwargs):
        raise _lib.YawhipError(-1, "yawhip_proj_count_shear: 36 pi bins of 12 radius bins do not fit the LDS of a workgroup: at most 35 pi bins "
                                   "at n_edges=13")

    cols = scenario()
    density, shapes = catalog(cols["density"]), catalog(cols["shapes"])
    dens_layout = density.build_trees(ZEDGES, with_redshifts=True)
    shape_layout = shapes.build_trees(ZEDGES, with_shear=True, with_redshifts=True)
    made = []
    monkeypatch.setattr(engine, "get_context", lambda *a, **k: object())
    monkeypatch.setattr(engine, "_handle", lambda layout, ctx, axis, role, upload, cosmology=None: made.append(role) or role)
    monkeypatch.setattr(_lib, "proj_count_shear", refuse)
    cfg = config()
    with pytest.raises(ValueError, match="at most 35 pi bins fit"):
        engine.count_projected_shear_fine(dens_layout, shape_layout, np.zeros((1, 4), dtype=np.int32), np.zeros((2, 13)),
                                          pi_edges=np.linspace(0.0, PI_MAX, 37), cosmology=cfg.cosmology, unit=cfg.scales.scales.unit)
    assert made == ["projected comoving", "projected shapes comoving"]  # the density side is the handle of w_p


# --------------------------------------------------------------------------- 4. the result class
def test_alignment_corrfunc_round_trip_equality_subsets_and_nan(stand_in):
    cols = scenario(shape_rand=True)
    cats = {name: catalog(c) for name, c in cols.items()}
    cf = yaw.crosscorrelate_alignment(config(), cats["shapes"], cats["density"], cats["density_rand"], pi_max=PI_MAX, pi_bins=PI_EDGES,
                                      shape_rand=cats["shape_rand"])[0]
    again = yaw.AlignmentCorrFunc.from_dict(cf.to_dict())
    assert again == cf and again is not cf and cf.is_compatible(again, require=True)
    assert cf.num_bins == 2 and cf.num_patches == 3 and cf.binning == cf.pi_bins[0]["w_sd"].binning and "num_pi=3" in repr(cf)
    state = cf.to_dict()
    state["pi_bins"][1] = dict(state["pi_bins"][1], x_sd=state["pi_bins"][1]["t_sd"])
    assert yaw.AlignmentCorrFunc.from_dict(state) != cf
    other_edges = yaw.AlignmentCorrFunc([0.0, 10.0, 25.0, 50.0], cf.pi_bins)
    assert other_edges != cf and not cf.is_compatible(other_edges)
    with pytest.raises(ValueError, match="pi edges differ"):
        cf.is_compatible(other_edges, require=True)
    assert cf != 1 and not cf.is_compatible(1)
    without = yaw.AlignmentCorrFunc(cf.pi_edges, [{k: v for k, v in planes.items() if k != "rr"} for planes in cf.pi_bins])
    assert without != cf and not np.array_equal(without.sample().data, cf.sample().data)  # N is W of SR there
    for bad_edges, bad_bins in (([0.0, 10.0], cf.pi_bins), ([1.0, 10.0, 25.0, 60.0], cf.pi_bins), (cf.pi_edges, [*cf.pi_bins[:2], without.pi_bins[2]]),
                                (cf.pi_edges, [{k: v for k, v in planes.items() if k != "x_sr"} for planes in cf.pi_bins])):
        with pytest.raises(ValueError):
            yaw.AlignmentCorrFunc(bad_edges, bad_bins)
    with pytest.raises(TypeError):
        yaw.AlignmentCorrFunc(cf.pi_edges, [dict(planes, t_sd=planes["t_sd"].counts) for planes in cf.pi_bins])
    with pytest.raises(ValueError, match="component"):
        cf.sample("tangential")
    # subsets go bin by bin
    one_bin, two_patches = cf.bins_subset(1), cf.patches_subset([0, 2])
    assert one_bin.num_bins == 1 and two_patches.num_patches == 2 and one_bin.num_pi == two_patches.num_pi == 3
    np.testing.assert_array_equal(one_bin.sample("cross").data, cf.sample("cross").data[1:])
    for j in range(3):
        assert two_patches.pi_bins[j]["t_sd"] == cf.pi_bins[j]["t_sd"].patches_subset([0, 2])
    # an empty N: NaN in that pi bin and in the sum, the other redshift bin untouched
    emptied = [dict(planes) for planes in cf.pi_bins]
    counts = emptied[1]["rr"].counts.counts.copy()
    counts[0] = 0.0
    emptied[1]["rr"] = yaw.NormalisedCounts(yaw.PatchedCounts(cf.binning, counts, auto=False), emptied[1]["rr"].sum_weights)
    holed = yaw.AlignmentCorrFunc(cf.pi_edges, emptied)
    for component in ("plus", "cross"):
        xi = holed.sample_xi(component)
        assert np.isnan(xi[1].data[0]) and np.all(np.isnan(xi[1].samples[:, 0])) and np.isfinite(xi[1].data[1])
        assert np.all(np.isfinite(xi[0].data)) and np.all(np.isfinite(xi[2].data))
        total = holed.sample(component)
        assert np.isnan(total.data[0]) and np.all(np.isnan(total.samples[:, 0]))
        assert total.data[1] == cf.sample(component).data[1]
