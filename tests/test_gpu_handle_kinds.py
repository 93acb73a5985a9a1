"""GPU: which kind of ``yawhip_shear_sources`` handle each argument of the ten lensing and projected counts takes (DESIGN.md
sections 21 and 26). One handle of each of the six kinds -- shear, excess-surface-density sources, lenses, radial lenses,
projected, projected shapes -- from the same 8 objects in 2 patches goes to every handle argument of every count, with an
empty job or cell list: no kernel runs, and the role checks precede everything that depends on the list.

The first six counts of the table below were written from the checks of the library as it stood before the handle had a
``kind`` (flags and pointer tests per entry point), the four counts over projected cells that came later from the five entry
points as they stood before they shared one path; each part was run against that library, and the code that replaced it must
answer the same. The ten counts have eighteen handle arguments (the lens side of ``yawhip_shear_count`` is a
``yawhip_catalog``, not such a handle): 108 cases, and two more where another check than the role's answers first. One case
uploads the kinds without objects from NULL columns, and the last ones hold the order of the refusals of the five counts over
projected cells: a call that is wrong in two places answers with the earlier check."""
import numpy as np
import pytest

from yet_another_wizz_amd import _lib, engine

pytestmark = pytest.mark.gpu
KINDS = ("shear", "dsigma_sources", "lenses", "radial_lenses", "projected", "projected_shapes")
N_PATCHES, N_BINS = 2, 2

# the refusals, as regular expressions of ``re.search`` (the library's message ends the exception's text)
NOT_SHEAR = "not a shear catalogue"
NOT_LENSES = "lenses are not a handle of yawhip_dsigma_upload_lenses$"
NOT_RADIAL = "not a handle of yawhip_dsigma_upload_lenses_radial$"
NOT_SOURCES = "sources are not a handle of yawhip_dsigma_upload_sources"
NOT_PROJECTED = "a handle is not one of yawhip_proj_upload$"
NOT_DENSITY = "the density handle is not one of yawhip_proj_upload$"
NOT_A_SHAPE = "the shape handle is not one of yawhip_proj_upload_shapes"
NOT_SHAPES = "a handle is not one of yawhip_proj_upload_shapes"
OK = None

# argument -> what it answers to a handle of each kind, in the order of KINDS
TABLE = {
    ("shear_count", "sources"): (OK, OK, NOT_SHEAR, NOT_SHEAR, NOT_SHEAR, NOT_SHEAR),
    ("shear_auto_count", "sources"): (OK, OK, NOT_SHEAR, NOT_SHEAR, NOT_SHEAR, NOT_SHEAR),
    ("shear_pair_count", "a"): (OK, OK, NOT_SHEAR, NOT_SHEAR, NOT_SHEAR, NOT_SHEAR),
    ("shear_pair_count", "b"): (OK, OK, NOT_SHEAR, NOT_SHEAR, NOT_SHEAR, NOT_SHEAR),
    ("dsigma_count", "lenses"): (NOT_LENSES, NOT_LENSES, OK, OK, NOT_LENSES, NOT_LENSES),
    ("dsigma_count", "sources"): (NOT_SOURCES, OK, NOT_SOURCES, NOT_SOURCES, NOT_SOURCES, NOT_SOURCES),
    # (a handle that is no lens handle at all is told so before the radial count asks for the column m)
    ("dsigma_count_radial", "lenses"): (NOT_LENSES, NOT_LENSES, NOT_RADIAL, OK, NOT_LENSES, NOT_LENSES),
    ("dsigma_count_radial", "sources"): (NOT_SOURCES, OK, NOT_SOURCES, NOT_SOURCES, NOT_SOURCES, NOT_SOURCES),
    ("proj_count", "a"): (NOT_PROJECTED, NOT_PROJECTED, NOT_PROJECTED, NOT_PROJECTED, OK, NOT_PROJECTED),
    ("proj_count", "b"): (NOT_PROJECTED, NOT_PROJECTED, NOT_PROJECTED, NOT_PROJECTED, OK, NOT_PROJECTED),
    ("proj_count_pi", "a"): (NOT_PROJECTED, NOT_PROJECTED, NOT_PROJECTED, NOT_PROJECTED, OK, NOT_PROJECTED),
    ("proj_count_pi", "b"): (NOT_PROJECTED, NOT_PROJECTED, NOT_PROJECTED, NOT_PROJECTED, OK, NOT_PROJECTED),
    ("proj_count_smu", "a"): (NOT_PROJECTED, NOT_PROJECTED, NOT_PROJECTED, NOT_PROJECTED, OK, NOT_PROJECTED),
    ("proj_count_smu", "b"): (NOT_PROJECTED, NOT_PROJECTED, NOT_PROJECTED, NOT_PROJECTED, OK, NOT_PROJECTED),
    ("proj_count_shear", "dens"): (NOT_DENSITY, NOT_DENSITY, NOT_DENSITY, NOT_DENSITY, OK, NOT_DENSITY),
    ("proj_count_shear", "shapes"): (NOT_A_SHAPE, NOT_A_SHAPE, NOT_A_SHAPE, NOT_A_SHAPE, NOT_A_SHAPE, OK),
    ("proj_count_shapes", "a"): (NOT_SHAPES, NOT_SHAPES, NOT_SHAPES, NOT_SHAPES, NOT_SHAPES, OK),
    ("proj_count_shapes", "b"): (NOT_SHAPES, NOT_SHAPES, NOT_SHAPES, NOT_SHAPES, NOT_SHAPES, OK),
}
PLANES = {"shear_count": 3, "shear_auto_count": 4, "shear_pair_count": 4, "dsigma_count": 3, "dsigma_count_radial": 3, "proj_count": 1,
          "proj_count_pi": 1, "proj_count_smu": 1, "proj_count_shear": 3, "proj_count_shapes": 4}  # (one pi or mu bin each)
CASES = [(count, arg, kind) for (count, arg) in TABLE for kind in KINDS]


@pytest.fixture(scope="module")
def handles():
    """One handle of each kind, a binned shear handle and the lens catalogue of ``shear_count``, on one context and one sort
    axis; freed after the module's tests."""
    ctx = engine.get_context(0)
    rng = np.random.default_rng(21)
    ra, dec = rng.uniform(0.50, 0.51, 8), rng.uniform(0.30, 0.31, 8)
    x, y, z = np.cos(dec) * np.cos(ra), np.cos(dec) * np.sin(ra), np.sin(dec)
    w, g1, g2 = rng.uniform(0.5, 1.5, 8), rng.normal(0.0, 0.1, 8), rng.normal(0.0, 0.1, 8)
    u, f, c = rng.uniform(0.0, 1e-3, 8), rng.uniform(0.5, 1.0, 8), rng.uniform(500.0, 900.0, 8)
    m, d = rng.uniform(4e5, 8e5, 8), rng.uniform(600.0, 900.0, 8)
    unbinned = np.array([0, 4, 8], dtype=np.int64)                # 2 patches
    binned = np.array([0, 2, 4, 6, 8], dtype=np.int64)            # 2 patches x 2 redshift bins
    made = {
        "ctx": ctx,
        "catalog": _lib.DeviceCatalog(ctx, x, y, z, None, N_PATCHES, N_BINS, binned),
        "shear": _lib.ShearSources(ctx, x, y, z, w, g1, g2, N_PATCHES, unbinned),
        "shear_binned": _lib.ShearSources(ctx, x, y, z, w, g1, g2, N_PATCHES, binned, n_bins=N_BINS),
        "dsigma_sources": _lib.ShearSources(ctx, x, y, z, w, g1, g2, N_PATCHES, unbinned, u=u),
        "lenses": _lib.DsigmaLenses(ctx, x, y, z, w, f, c, N_PATCHES, N_BINS, binned),
        "radial_lenses": _lib.DsigmaLenses(ctx, x, y, z, w, f, c, N_PATCHES, N_BINS, binned, m=m),
        "projected": _lib.ProjHandle(ctx, x, y, z, w, d, c, N_PATCHES, N_BINS, binned),
        "projected_shapes": _lib.ProjShapesHandle(ctx, x, y, z, w, g1, g2, d, c, N_PATCHES, N_BINS, binned),
    }
    yield made
    for name, handle in made.items():
        if name != "ctx":
            handle.free()


def table_of(n_rows):
    """A valid 2-edge table: squared chords for the counts in angle, squared radii within the cap for those in a radius (the
    nearest lens has m >= 4e5, the nearest object d >= 600)."""
    return np.tile(np.array([[0.0, 1e-6]]), (n_rows, 1))


def call(h, count, arg, given):
    """``count`` with ``given`` as its argument ``arg``, a handle it takes everywhere else, and an empty list."""
    ctx, jobs = h["ctx"], np.empty((0, 2), dtype=np.int32)
    if count == "shear_count":
        return _lib.shear_count(ctx, h["catalog"], given, jobs, table_of(N_BINS))
    if count == "shear_auto_count":  # (as many rows as the handle has bins: the check after the role's)
        return _lib.shear_auto_count(ctx, given, jobs, table_of(given.n_bins))
    if count == "shear_pair_count":
        a, b = (given, h["shear_binned"]) if arg == "a" else (h["shear_binned"], given)
        return _lib.shear_pair_count(ctx, a, b, np.empty((0, 5), dtype=np.int32), table_of(N_BINS))
    if count in ("dsigma_count", "dsigma_count_radial"):
        lenses = given if arg == "lenses" else h["radial_lenses"]
        sources = given if arg == "sources" else h["dsigma_sources"]
        return getattr(_lib, count)(ctx, lenses, sources, jobs, table_of(N_BINS))
    return call_projected(h, count, arg, given, np.empty((0, 4), dtype=np.int32))


PI_EDGES, M2_EDGES = np.array([0.0, 40.0]), np.array([0.0, 1.0])  # one bin each


def call_projected(h, count, arg, given, cells, *, pmax=40.0, pi_edges=PI_EDGES, m2=M2_EDGES):
    """One of the five counts over projected cells with ``given`` as its argument ``arg`` and a handle it takes as the other;
    the planes of the counts with a second binning come back one per bin, as the others' do."""
    ctx, r2 = h["ctx"], table_of(N_BINS)
    if count == "proj_count_shear":
        dens, shapes = (given, h["projected_shapes"]) if arg == "dens" else (h["projected"], given)
        planes, stats = _lib.proj_count_shear(ctx, dens, shapes, cells, r2, pi_edges)
        return (*(p for plane in planes for p in plane), stats)
    other = h["projected_shapes" if count == "proj_count_shapes" else "projected"]
    a, b = (given, other) if arg == "a" else (other, given)
    if count == "proj_count":
        return _lib.proj_count(ctx, a, b, cells, r2, pmax)
    if count == "proj_count_shapes":
        planes, stats = _lib.proj_count_shapes(ctx, a, b, cells, r2, pi_edges)
        return (*(p for plane in planes for p in plane), stats)
    fine, stats = _lib.proj_count_pi(ctx, a, b, cells, r2, pi_edges) if count == "proj_count_pi" else _lib.proj_count_smu(ctx, a, b, cells, r2, m2)
    return (*fine, stats)


def check(h, count, arg, given, expected):
    if expected is OK:
        *planes, stats = call(h, count, arg, given)
        assert len(planes) == PLANES[count] and all(p.size == 0 and p.shape[0] == 0 and p.shape[-1] == 1 for p in planes)
        assert stats.n_launches == 0 and stats.n_workgroups == 0
    else:
        with pytest.raises(_lib.YawhipError, match=expected) as refusal:
            call(h, count, arg, given)
        assert "(status -5)" in str(refusal.value)  # YAWHIP_ERR_MISMATCH


@pytest.mark.parametrize("count,arg,kind", CASES, ids=[f"{c}-{a}-{k}" for c, a, k in CASES])
def test_each_argument_takes_the_kinds_of_the_table(handles, count, arg, kind):
    # the shear kind: unbinned where the count wants that, binned for the auto and pair counts
    binned = kind == "shear" and count in ("shear_auto_count", "shear_pair_count")
    check(handles, count, arg, handles["shear_binned" if binned else kind], TABLE[count, arg][KINDS.index(kind)])


def test_a_kind_without_objects_from_null_columns_counts_to_nothing():
    """The C contract takes ``n = 0`` with every column NULL. The handle still is of its kind, with everything the kind has:
    the counts in a radius read its least ``m`` or ``d`` per bin (none: no reach) for cells over its empty segments, and
    return zero planes. Through ctypes: the wrappers hand the library a non-null address even for an empty array."""
    import ctypes
    import types

    lib, ctx = _lib.load_library(), engine.get_context(0)
    made = []

    def upload(symbol, n_columns, bins):
        handle = ctypes.c_void_p()
        offsets = np.zeros(N_PATCHES * (bins[0] if bins else 1) + 1, dtype=np.int64)
        rc = getattr(lib, symbol)(ctx._h, 0, *([None] * n_columns), N_PATCHES, *bins, offsets.ctypes.data_as(ctypes.POINTER(ctypes.c_int64)),
                                  2, ctypes.byref(handle))
        assert rc == 0 and handle, (symbol, lib.yawhip_last_error())
        made.append(handle)
        return types.SimpleNamespace(_h=handle)

    try:
        sources = upload("yawhip_dsigma_upload_sources", 7, ())
        lenses = upload("yawhip_dsigma_upload_lenses_radial", 7, (N_BINS,))
        projected = upload("yawhip_proj_upload", 6, (N_BINS,))
        jobs = np.array([[0, 0], [0, 1]], dtype=np.int32)
        cells = np.array([[0, 0, 0, 1], [0, 2, 0, 0], [3, 1, 1, 0]], dtype=np.int32)
        for *planes, stats in (_lib.dsigma_count_radial(ctx, lenses, sources, jobs, table_of(N_BINS)),
                               _lib.dsigma_count(ctx, lenses, sources, jobs, table_of(N_BINS)),
                               _lib.proj_count(ctx, projected, projected, cells, table_of(N_BINS), 40.0)):
            assert all(p.size and not p.any() for p in planes)
            assert stats.candidate_pairs == 0 and stats.evaluated_pairs == 0 and stats.n_launches == 1
    finally:
        for handle in made:
            lib.yawhip_shear_free(handle)


def test_a_check_after_the_roles_still_answers_an_accepted_kind(handles):
    """The role check comes first and is not the last: a binned shear handle is a shear catalogue, and ``shear_count`` wants
    it unbinned; an unbinned one does not fit the two rows of an auto count."""
    jobs = np.empty((0, 2), dtype=np.int32)
    with pytest.raises(_lib.YawhipError, match="upload them unbinned"):
        _lib.shear_count(handles["ctx"], handles["catalog"], handles["shear_binned"], jobs, table_of(N_BINS))
    with pytest.raises(_lib.YawhipError, match=r"bin count \(1\) does not fit n_bins=2"):
        _lib.shear_auto_count(handles["ctx"], handles["dsigma_sources"], jobs, table_of(N_BINS))


# the five counts over projected cells: (count, its second handle argument, a kind that argument refuses, the refusal, what makes
# its own argument bad, the refusal of that)
BAD_PI = dict(pi_edges=np.array([1.0, 2.0]))
OWN_ARGUMENT = [
    ("proj_count", "b", "projected_shapes", NOT_PROJECTED, dict(pmax=-1.0), "pmax must be a number >= 0"),
    ("proj_count_pi", "b", "projected_shapes", NOT_PROJECTED, BAD_PI, "the first pi edge must be 0"),
    ("proj_count_smu", "b", "projected_shapes", NOT_PROJECTED, dict(m2=np.array([0.0, 0.5])), "squared mu edges must start at 0 and end at 1"),
    ("proj_count_shear", "shapes", "projected", NOT_A_SHAPE, BAD_PI, "the first pi edge must be 0"),
    ("proj_count_shapes", "b", "projected", NOT_SHAPES, BAD_PI, "the first pi edge must be 0"),
]
# (count, a number of bins beyond its cap at the 2 edges of ``table_of``, the cap): the caps that the library's static_asserts quote
BEYOND_CAP = [("proj_count_pi", 1024, 1023), ("proj_count_smu", 1024, 1023), ("proj_count_shear", 394, 393), ("proj_count_shapes", 241, 240)]


def taken(h, count, arg):
    """A handle that ``count`` takes as its argument ``arg``."""
    return h[KINDS[TABLE[count, arg].index(OK)]]


@pytest.mark.parametrize("count,arg,kind,not_kind,bad,not_own", OWN_ARGUMENT, ids=[case[0] for case in OWN_ARGUMENT])
def test_projected_counts_refuse_in_the_order_of_their_checks(handles, count, arg, kind, not_kind, bad, not_own):
    """The kind of ``b`` is asked before the count's own argument, that before the cap, and the cap before the cells."""
    cells = np.empty((0, 4), dtype=np.int32)
    with pytest.raises(_lib.YawhipError, match=not_kind) as refusal:  # the wrong kind of b and a bad pmax / pi edges / mu edges
        call_projected(handles, count, arg, handles[kind], cells, **bad)
    assert "(status -5)" in str(refusal.value)  # YAWHIP_ERR_MISMATCH
    with pytest.raises(_lib.YawhipError, match=not_own):  # (the own argument alone is refused too)
        call_projected(handles, count, arg, taken(handles, count, arg), cells, **bad)
    for name, n_bins, cap in BEYOND_CAP:
        if name != count:
            continue
        what = "mu" if count == "proj_count_smu" else "pi"
        edges = np.linspace(0.0, 1.0, n_bins + 1)
        bad_edges = dict(m2=edges[::-1].copy()) if what == "mu" else dict(pi_edges=edges + 1.0)
        with pytest.raises(_lib.YawhipError, match=not_own):  # a bad edge array and a cap that is exceeded
            call_projected(handles, count, arg, taken(handles, count, arg), cells, **bad_edges)
        good_edges = dict(m2=edges) if what == "mu" else dict(pi_edges=edges)
        no_such_cell = np.array([[99, 0, 0, 0]], dtype=np.int32)
        with pytest.raises(_lib.YawhipError, match=f"do not fit the LDS of a workgroup: at most {cap} {what} bins at n_edges=2$"):
            call_projected(handles, count, arg, taken(handles, count, arg), no_such_cell, **good_edges)  # ... and a bad cell list
        with pytest.raises(_lib.YawhipError, match="cell 0 has a segment outside"):  # (within the cap the cell is refused)
            call_projected(handles, count, arg, taken(handles, count, arg), no_such_cell)
