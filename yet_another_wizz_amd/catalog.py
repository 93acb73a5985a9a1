"""In-memory catalogue split into spatial patches.

Keeps the ``yaw.Catalog`` call shapes (src/yaw/catalog/catalog.py:911-1468): a ``Mapping`` from
patch id (0..P-1) to :class:`Patch`, the ``from_dataframe`` / ``from_file`` keyword names, and the
per-patch accessors ``get_centers`` / ``get_radii`` / ``get_num_records`` / ``get_sum_weights`` the
measurement driver reads.  What is different by design: the reference caches every patch on disk
(``data.bin`` AoS rows, catalog.py:325-331, patch.py:164-178) and re-reads pickled KD-trees per job;
here a catalogue is a set of float64 columns held once, sorted by patch, and ``build_trees``
prepares the (patch, redshift-bin)-sorted SoA layout that is uploaded to HBM once per measurement.
"""
from __future__ import annotations

from collections.abc import Mapping
from pathlib import Path

import numpy as np

from . import _threads
from .binning import Binning
from .coordinates import AngularCoordinates, AngularDistances
from .options import Closed

radec_to_xyz = _threads.radec_to_xyz  # numpy's cos / sin on slices of the columns, side by side (same values)

__all__ = ["Catalog", "Patch", "Metadata", "InconsistentPatchesError", "PatchLayout", "ScalarTwin"]

PATCH_ID_MAX = np.iinfo(np.int16).max  # the reference stores patch ids as 16-bit integers (datachunk.py:40-42)


class InconsistentPatchesError(Exception):
    """Patches of two catalogues do not line up (catalog.py:80-82)."""


def _check_patch_count(num: int) -> None:
    if num < 1 or num > PATCH_ID_MAX:
        raise ValueError(f"number of patches must be in range [1, {PATCH_ID_MAX}]")


def _stable_argsort_small(keys, num_values: int):
    """Stable argsort of non-negative integer keys < ``num_values``. numpy sorts 16-bit integers with a
    radix sort (an order of magnitude faster than the merge sort it uses for int64); the permutation is
    the same, stable sorts being unique."""
    if num_values <= np.iinfo(np.uint16).max:
        return np.argsort(keys.astype(np.uint16), kind="stable")
    return np.argsort(keys, kind="stable")


DEVICE_ASSIGN_MIN = 200_000  # below this the host is as fast as a round trip to the device
HOST_GROUP_MIN = 200_000     # below this numpy's argsort + gathers are as fast as the library's threaded counting sort
RANDOM_CHUNKSIZE = 16_777_216  # values per generator call of from_random (the reference's CHUNKSIZE, readers.py:49)
PATCH_METHODS = ("probe", "full")  # what patch_num= runs: kmeans_centers on a probe sample, or patches.py on all objects


def nearest_center(xyz, centers_xyz, chunk: int = 1 << 18):
    """Index of the nearest centre in Euclidean xyz for every object; ``xyz`` is an [N, 3] array or a tuple of
    three columns.

    Same rule as ``assign_patch_centers`` (catalog.py:229-249, scipy.cluster.vq.vq): squared
    distance accumulated x, y, z in that order, first minimum wins."""
    columns = xyz if isinstance(xyz, tuple) else None
    n = len(columns[0]) if columns is not None else len(xyz)
    if n >= DEVICE_ASSIGN_MIN:  # large inputs: on the GPU if there is one (identical ids, 40x faster)
        from . import engine

        ids = engine.assign_patches(columns if columns is not None else xyz, centers_xyz)
        if ids is not None:
            return ids
    if columns is not None:
        xyz = np.column_stack(columns)
    try:
        from scipy.cluster.vq import vq

        ids, _ = vq(xyz, centers_xyz)
        return ids.astype(np.int64)
    except ImportError:  # pragma: no cover - scipy is present in the supported images
        out = np.empty(len(xyz), dtype=np.int64)
        for lo in range(0, len(xyz), chunk):
            blk = xyz[lo : lo + chunk]
            d = (blk[:, None, 0] - centers_xyz[None, :, 0]) ** 2
            d += (blk[:, None, 1] - centers_xyz[None, :, 1]) ** 2
            d += (blk[:, None, 2] - centers_xyz[None, :, 2]) ** 2
            out[lo : lo + chunk] = d.argmin(axis=1)
        return out


def kmeans_centers(xyz, weights, num: int, *, seed: int = 12345, iterations: int = 25) -> AngularCoordinates:
    """Patch centres from spherical k-means on a probe sample (stands in for the treecorr k-means of
    ``create_patch_centers``, catalog.py:183-226; deterministic for a given input)."""
    rng = np.random.default_rng(seed)
    n = len(xyz)
    first = int(rng.integers(n))
    centers = [xyz[first]]
    d2 = ((xyz - centers[0]) ** 2).sum(axis=1)
    for _ in range(1, num):  # k-means++ seeding
        prob = d2 / d2.sum()
        centers.append(xyz[int(rng.choice(n, p=prob))])
        d2 = np.minimum(d2, ((xyz - centers[-1]) ** 2).sum(axis=1))
    centers = np.array(centers)
    w = np.ones(n) if weights is None else np.asarray(weights, dtype=np.float64)
    for _ in range(iterations):
        ids = nearest_center(xyz, centers)
        sums = np.zeros_like(centers)
        for axis in range(3):
            sums[:, axis] = np.bincount(ids, weights=w * xyz[:, axis], minlength=num)
        norm = np.linalg.norm(sums, axis=1)
        moved = np.where(norm[:, None] > 0, sums / np.maximum(norm, 1e-300)[:, None], centers)
        if np.allclose(moved, centers, atol=1e-12):
            break
        centers = moved
    return AngularCoordinates.from_3d(centers)


# ---------------------------------------------------------------------------------------------
# On-disk cache format of the reference (read and written unchanged so that caches are
# interchangeable):  <dir>/patch_ids.bin  int16 ids (catalog.py:325-331,529-530),
# <dir>/patch_<id>/data.bin  1 header byte + row-major float64 records (patch.py:164-178,
# datachunk.py:47,74-117), <dir>/patch_<id>/meta.yml (patch.py:149-161).
PATCH_INFO_FILE = "patch_ids.bin"
PATCH_NAME_TEMPLATE = "patch_{:d}"
PATCH_DATA_FILE = "data.bin"
PATCH_META_FILE = "meta.yml"
_ATTR_BITS = (("ra", 0), ("dec", 1), ("weights", 2), ("redshifts", 3), ("patch_ids", 4), ("kappa", 5))


def read_patch_file(path):
    """data.bin -> dict of float64 columns (header byte: bit set = column present)."""
    with open(path, "rb") as f:
        flags = int.from_bytes(f.read(1), byteorder="big")
        fields = [name for name, bit in _ATTR_BITS if flags & (1 << bit)]
        raw = np.fromfile(f, dtype=np.float64)
    if "ra" not in fields or "dec" not in fields or len(raw) % len(fields):
        raise ValueError(f"not a patch data file: {path}")
    table = raw.reshape(-1, len(fields))
    return {name: table[:, i].copy() for i, name in enumerate(fields)}


def write_patch_file(path, ra, dec, weights=None, redshifts=None, kappa=None) -> None:
    """Columns in the reference's ATTR_ORDER (ra, dec, weights, redshifts, [patch ids: never stored], kappa; datachunk.py:47)."""
    cols = [ra, dec] + [c for c in (weights, redshifts, kappa) if c is not None]
    flags = 0b11 | (int(weights is not None) << 2) | (int(redshifts is not None) << 3) | (int(kappa is not None) << 5)
    with open(path, "wb") as f:
        f.write(flags.to_bytes(1, byteorder="big"))
        np.column_stack(cols).astype(np.float64).tofile(f)


class Metadata:
    """Patch summary used to link patches (mirror of patch.py:44-161)."""

    __slots__ = ("num_records", "sum_weights", "center", "radius")

    def __init__(self, *, num_records: int, sum_weights: float, center: AngularCoordinates,
                 radius: AngularDistances) -> None:
        self.num_records = num_records
        self.sum_weights = sum_weights
        self.center = center
        self.radius = radius

    def __repr__(self) -> str:
        return (f"Metadata(num_records={self.num_records}, sum_weights={self.sum_weights}, "
                f"center={self.center.data[0]}, radius={self.radius.data[0]})")

    @classmethod
    def compute(cls, coords: AngularCoordinates, *, weights=None, center: AngularCoordinates | None = None, xyz=None):
        """Sum of weights (or N), weighted mean direction, radius = largest separation from the
        centre (patch.py:103-147). ``xyz`` = ``coords.to_3d()`` if the caller has it already (the
        catalogue computes the unit vectors once): the same values go through the same operations as
        ``coords.mean`` / ``coords.distance``."""
        if center is not None and len(center) != 1:
            raise ValueError("'center' must be one single coordinate")
        sum_weights = float(len(coords)) if weights is None else float(np.sum(weights))
        if xyz is None:
            xyz = coords.to_3d()
        if isinstance(xyz, tuple):  # three columns: the same numbers without an [N, 3] copy
            x, y, z = xyz
            if center is not None:
                centre = center.copy()
            else:  # the reference averages the rows of the [N, 3] array: same call, same summation order
                centre = AngularCoordinates.from_3d(np.average(np.column_stack(xyz), weights=weights, axis=0))
            cx, cy, cz = centre.to_3d()[0]
            chord = np.sqrt(((x - cx) ** 2 + (y - cy) ** 2) + (z - cz) ** 2)  # = ((xyz - c) ** 2).sum(axis=1): left to right
        else:
            centre = center.copy() if center is not None else AngularCoordinates.from_3d(np.average(xyz, weights=weights, axis=0))
            chord = np.sqrt(((xyz - centre.to_3d()) ** 2).sum(axis=1))
        radius = AngularDistances.from_3d(chord).max()
        return cls(num_records=len(coords), sum_weights=sum_weights, center=centre, radius=radius)

    def to_dict(self) -> dict:
        return dict(num_records=int(self.num_records), sum_weights=float(self.sum_weights),
                    center=self.center.tolist()[0], radius=self.radius.tolist()[0])


class Patch:
    """One spatial patch: a contiguous row range of its catalogue's columns."""

    __slots__ = ("meta", "_cat", "_lo", "_hi")

    def __init__(self, catalog: "Catalog", lo: int, hi: int, meta: Metadata) -> None:
        self._cat, self._lo, self._hi, self.meta = catalog, lo, hi, meta

    def __repr__(self) -> str:
        return (f"Patch(num_records={self.meta.num_records}, weights={self.has_weights}, "
                f"redshifts={self.has_redshifts})")

    def __len__(self) -> int:
        return self._hi - self._lo

    @property
    def has_weights(self) -> bool:
        return self._cat._w is not None

    @property
    def has_redshifts(self) -> bool:
        return self._cat._z is not None

    @property
    def has_kappa(self) -> bool:
        return self._cat._k is not None

    @property
    def coords(self) -> AngularCoordinates:
        sl = slice(self._lo, self._hi)
        return AngularCoordinates(np.column_stack([self._cat._ra[sl], self._cat._dec[sl]]))

    @property
    def weights(self):
        return None if self._cat._w is None else self._cat._w[self._lo : self._hi]

    @property
    def redshifts(self):
        return None if self._cat._z is None else self._cat._z[self._lo : self._hi]

    @property
    def kappa(self):
        """Scalar-field values of the patch's objects, or ``None`` (patch.py:431-436)."""
        return None if self._cat._k is None else self._cat._k[self._lo : self._hi]

    @property
    def g1(self):
        """First shear component of the patch's objects (east / north frame, see ``Catalog.from_arrays``), or ``None``."""
        return None if self._cat._g1 is None else self._cat._g1[self._lo : self._hi]

    @property
    def g2(self):
        """Second shear component of the patch's objects, or ``None``."""
        return None if self._cat._g2 is None else self._cat._g2[self._lo : self._hi]


class PatchLayout:
    """Device-ready layout of one catalogue for one redshift binning: float64 SoA columns sorted
    by (patch, bin), CSR offsets over the P*B segments, and the per-segment sum of weights.

    This is the counterpart of ``build_trees`` (src/yaw/catalog/trees.py:365-429): objects outside
    the binning are dropped (:414), an unbinned catalogue has one segment per patch (:400-404)."""

    __slots__ = ("x", "y", "z", "w", "offsets", "num_patches", "num_bins", "sum_weights", "device", "z_extent", "kappa", "twin", "g1", "g2",
                 "redshifts", "handles")

    def __init__(self, x, y, z, w, offsets, num_patches: int, num_bins: int, kappa=None, g1=None, g2=None, redshifts=None) -> None:
        self.x, self.y, self.z, self.w = x, y, z, w
        self.redshifts = redshifts  # the objects' redshifts in the layout's order (build_trees(with_redshifts=True)), or None
        self.g1, self.g2 = g1, g2  # shear columns in the layout's order (unbinned layouts, and build_trees(with_shear=True)), or None
        self.handles = {}  # (Context id, role) -> (resident handle of a lensing or projected count, the cosmology of its columns or None)
        self.kappa = kappa  # scalar-field column in the layout's order, or None
        self.twin = None if kappa is None else ScalarTwin(self)  # the "k" side of a scalar count
        self.offsets = offsets
        self.num_patches, self.num_bins = num_patches, num_bins
        if w is None:
            seg = np.diff(offsets).astype(np.float64)  # sum_weights = float(N) without weights (trees.py:225-227)
        else:  # ndarray.sum() per tree (trees.py:233-234); an empty tree has 0.0 (trees.py:249-258)
            seg = np.array([float(w[lo:hi].sum()) for lo, hi in zip(offsets[:-1], offsets[1:])], dtype=np.float64)
        self.sum_weights = seg.reshape(num_patches, num_bins).T.copy()  # [B_or_1, P]
        self.device = {}  # Context id -> DeviceCatalog
        # extent of every patch along the axis the device sorts by (z): feeds the cost model that
        # balances jobs over GPUs (the z-window culling makes flat patches cheaper than tall ones)
        bounds = offsets[:: num_bins]
        self.z_extent = np.array([np.ptp(z[lo:hi]) if hi > lo else 0.0 for lo, hi in zip(bounds[:-1], bounds[1:])])

    @property
    def weighted(self) -> bool:
        return self.w is not None

    @property
    def num_records(self) -> int:
        return len(self.x)

    def segment_sizes(self):
        """int64[P, B_or_1]."""
        return np.diff(self.offsets).reshape(self.num_patches, self.num_bins)

    def sum_weights_for(self, num_bins: int):
        """f64[B, P]; an unbinned catalogue repeats its single tree for every bin (trees.py:600-601)."""
        if self.num_bins == 1 and num_bins != 1:
            return np.repeat(self.sum_weights, num_bins, axis=0)
        return self.sum_weights


class ScalarTwin:
    """The "k" side of a layout that carries a scalar field: the same objects, segments and order with the per-object weight
    ``kappa * w`` (``kappa`` without weights) -- what ``AngularTree.get_pair_weights`` hands to the count for a tree on the
    "k" side of a mode (trees.py:270-301). On the device it is the second catalogue of ``yawhip_catalog_upload_scalar``, made
    together with the plain one (``engine.device_catalog``); the host never needs the product, ``w`` forms it on first use
    for code that reads layouts on the host (the CPU oracle of the tests, the cost model)."""

    __slots__ = ("base", "device", "_w")

    def __init__(self, base: PatchLayout) -> None:
        self.base = base
        self.device = {}  # Context id -> DeviceCatalog (the twin)
        self._w = None

    x = property(lambda self: self.base.x)
    y = property(lambda self: self.base.y)
    z = property(lambda self: self.base.z)
    offsets = property(lambda self: self.base.offsets)
    num_patches = property(lambda self: self.base.num_patches)
    num_bins = property(lambda self: self.base.num_bins)
    z_extent = property(lambda self: self.base.z_extent)
    num_records = property(lambda self: self.base.num_records)
    weighted = True

    @property
    def w(self):
        if self._w is None:
            self._w = self.base.kappa.copy() if self.base.w is None else self.base.kappa * self.base.w
        return self._w

    def segment_sizes(self):
        return self.base.segment_sizes()


class Catalog(Mapping):
    """Catalogue of points on the sphere, split into P spatial patches with ids 0..P-1."""

    def __init__(self, cache_directory, *, max_workers: int | None = None) -> None:
        """Restore a catalogue from a cache directory written by the reference or by :meth:`to_cache`
        (same call as ``yaw.Catalog(cache_directory)``, catalog.py:966-977)."""
        directory = Path(cache_directory)
        if not directory.exists():
            raise OSError(f"cache directory not found: {directory}")
        info = directory / PATCH_INFO_FILE
        if not info.exists():
            raise InconsistentPatchesError("patch info file not found")
        ids = np.fromfile(info, dtype=np.int16).astype(np.int64)
        if not np.array_equal(np.sort(ids), np.arange(len(ids))):
            raise InconsistentPatchesError("patch IDs must be contiguous and start at 0")
        columns, metas = [], {}
        for pid in range(len(ids)):
            patch_dir = directory / PATCH_NAME_TEMPLATE.format(pid)
            columns.append(read_patch_file(patch_dir / PATCH_DATA_FILE))
            meta_file = patch_dir / PATCH_META_FILE
            if meta_file.exists():
                import yaml

                with meta_file.open() as f:
                    metas[pid] = yaml.safe_load(f)
        present = [tuple(sorted(c)) for c in columns]
        if any(p != present[0] for p in present):
            raise InconsistentPatchesError("data columns are not consistent between patches")

        def joined(name):
            return np.concatenate([c[name] for c in columns]) if name in columns[0] else None

        self._setup(joined("ra"), joined("dec"), patch_ids=np.repeat(np.arange(len(ids)), [len(c["ra"]) for c in columns]),
                    num_patches=len(ids), weights=joined("weights"), redshifts=joined("redshifts"),
                    kappa=joined("kappa"), cache_directory=directory, stored_meta=metas)

    @classmethod
    def _from_columns(cls, ra, dec, **kwargs):
        new = cls.__new__(cls)
        new._setup(ra, dec, **kwargs)
        return new

    def _setup(self, ra, dec, *, patch_ids, num_patches: int | None = None, weights=None, redshifts=None, kappa=None,
               g1=None, g2=None, patch_centers: AngularCoordinates | None = None, cache_directory=None, stored_meta=None,
               xyz=None) -> None:
        """Common initialiser; coordinates in radian. ``xyz`` = ``radec_to_xyz(ra, dec)`` if already known."""
        ra = np.asarray_chkfinite(ra, dtype=np.float64)
        dec = np.asarray_chkfinite(dec, dtype=np.float64)
        patch_ids = np.asarray(patch_ids)
        if not (len(ra) == len(dec) == len(patch_ids)):
            raise ValueError("input columns differ in length")
        if len(ra) == 0:
            raise ValueError("catalogue is empty")
        if patch_ids.min() < 0 or patch_ids.max() > PATCH_ID_MAX:
            raise ValueError(f"'patch_ids' must be in range [0, {PATCH_ID_MAX}]")
        patch_ids = patch_ids.astype(np.int64)
        num = int(patch_ids.max()) + 1 if num_patches is None else int(num_patches)
        _check_patch_count(num)
        if patch_ids.max() >= num:
            raise ValueError("patch id exceeds the number of patches")
        sizes = np.bincount(patch_ids, minlength=num)
        if np.any(sizes == 0):  # same restriction as the reference (catalog.py:944-947)
            empty = np.flatnonzero(sizes == 0).tolist()
            raise ValueError(f"empty patches are not supported (patch ids {empty})")
        weights = None if weights is None else np.asarray_chkfinite(weights, dtype=np.float64)
        redshifts = None if redshifts is None else np.asarray_chkfinite(redshifts, dtype=np.float64)
        kappa = None if kappa is None else np.asarray_chkfinite(kappa, dtype=np.float64)
        if (g1 is None) != (g2 is None):
            raise ValueError("shear needs both components: give 'g1' and 'g2', or neither")
        g1 = None if g1 is None else np.asarray_chkfinite(g1, dtype=np.float64)
        g2 = None if g2 is None else np.asarray_chkfinite(g2, dtype=np.float64)
        if any(c is not None and len(c) != len(ra) for c in (weights, redshifts, kappa, g1, g2)):
            raise ValueError("input columns differ in length")
        # unit vectors: computed once per catalogue (assignment, patch metadata and the device layouts all use
        # these values -- the exact host numbers the pair predicate runs on)
        xyz = radec_to_xyz(ra, dec) if xyz is None else tuple(np.asarray(c, dtype=np.float64) for c in xyz)
        columns = [ra, dec, *xyz] + [c for c in (weights, redshifts, kappa, g1, g2) if c is not None]
        grouped = False
        if np.all(patch_ids[1:] >= patch_ids[:-1]):
            # already grouped by patch (a restored cache): the stable order is the identity. The catalogue keeps its own copy
            # of the columns all the same -- a later change of the caller's arrays must not reach into it
            columns = [np.array(c, dtype=np.float64, copy=True) for c in columns]
            grouped = True
        elif len(ra) >= HOST_GROUP_MIN:  # one threaded counting sort over all columns (yawhip_host_group_columns)
            from . import _lib

            try:
                columns, _ = _lib.group_columns(patch_ids, num, columns)
                grouped = True
            except _lib.YawhipError:  # no library on this machine: catalogue preparation is host work, numpy does it too
                pass
        if not grouped:
            order = _stable_argsort_small(patch_ids, num)
            columns = [c[order] for c in columns]
        self._ra, self._dec, self._xyz = columns[0], columns[1], tuple(columns[2:5])
        rest = iter(columns[5:])
        self._w = None if weights is None else next(rest)
        self._z = None if redshifts is None else next(rest)
        self._k = None if kappa is None else next(rest)  # scalar field ("kappa"), carried like any other column
        self._g1 = None if g1 is None else next(rest)    # shear components, carried the same way
        self._g2 = None if g2 is None else next(rest)
        self._patch_off = np.concatenate([[0], np.cumsum(sizes)]).astype(np.int64)
        self._layouts: dict = {}
        self._active_layout = None
        self.cache_directory = None if cache_directory is None else Path(cache_directory)
        if patch_centers is not None and len(patch_centers) != num:
            raise ValueError("number of patch centers does not match the number of patches")

        def patch_meta(pid):
            lo, hi = int(self._patch_off[pid]), int(self._patch_off[pid + 1])
            if stored_meta and pid in stored_meta:  # meta.yml of the cache (patch.py:359-362)
                m = stored_meta[pid]
                return Metadata(num_records=int(m["num_records"]), sum_weights=float(m["sum_weights"]),
                                center=AngularCoordinates(m["center"]), radius=AngularDistances(m["radius"]))
            return Metadata.compute(
                range(hi - lo),  # only its length is used when the unit vectors are given
                weights=None if self._w is None else self._w[lo:hi],
                center=None if patch_centers is None else patch_centers[pid],
                xyz=tuple(c[lo:hi] for c in self._xyz),
            )

        if len(ra) >= _threads.MIN_PARALLEL and _threads.pool_size() > 1:  # patches are independent
            metas = list(_threads._executor().map(patch_meta, range(num)))
        else:
            metas = [patch_meta(pid) for pid in range(num)]
        self._patches = {pid: Patch(self, int(self._patch_off[pid]), int(self._patch_off[pid + 1]), metas[pid])
                         for pid in range(num)}

    # ------------------------------------------------------------------ constructors
    @classmethod
    def from_arrays(cls, ra, dec, *, weights=None, redshifts=None, kappa=None, g1=None, g2=None, flip_g2: bool = False,
                    patch_centers=None, patch_ids=None, patch_num: int | None = None, degrees: bool = True,
                    cache_directory=None, overwrite: bool = False, probe_size: int = -1, patch_method: str = "probe"):
        """Build from plain arrays. One of ``patch_centers`` (nearest-centre assignment),
        ``patch_ids`` (pre-assigned, contiguous from 0) or ``patch_num`` (k-means) is required, with
        that precedence (``PatchMode.determine``, catalog.py:95-167). ``patch_method`` says which k-means ``patch_num``
        runs: ``"probe"``, :func:`kmeans_centers` on a probe sample, or ``"full"``, the deterministic k-means of
        :mod:`~yet_another_wizz_amd.patches` over all objects with the catalogue's weights (on the GPU when there is one);
        it is ignored where centres or ids take precedence.

        ``g1`` / ``g2`` (both or neither) attach a shear for ``crosscorrelate_shear``, given in the local frame whose first
        axis points east (+RA) and whose second axis points north: ``g1 > 0`` is an elongation along east-west, ``g2 > 0``
        one along the diagonal between +east and +north. Catalogues in the opposite handedness pass ``flip_g2=True``,
        which stores ``-g2``."""
        if patch_method not in PATCH_METHODS:
            raise ValueError(f"'patch_method' must be one of {PATCH_METHODS}, got {patch_method!r}")
        if (g1 is None) != (g2 is None):
            raise ValueError("shear needs both components: give 'g1' and 'g2', or neither")
        if g2 is not None and flip_g2:
            g2 = -np.asarray(g2, dtype=np.float64)
        ra = np.asarray_chkfinite(ra, dtype=np.float64)
        dec = np.asarray_chkfinite(dec, dtype=np.float64)
        if degrees:  # datachunk.py:265-267
            ra, dec = np.deg2rad(ra), np.deg2rad(dec)
        centers = None
        xyz = None
        if patch_centers is not None:
            if isinstance(patch_centers, Catalog):
                centers = patch_centers.get_centers()
            elif isinstance(patch_centers, AngularCoordinates):
                centers = patch_centers
            else:
                raise TypeError("'patch_centers' must be a set of coordinates or another catalog")
            _check_patch_count(len(centers))
        elif patch_ids is None:
            if patch_num is None:
                raise ValueError("no patch method specified")
            if not isinstance(patch_num, (int, np.integer)):
                raise TypeError("'patch_num' must be an integer")
            _check_patch_count(int(patch_num))
            if patch_method == "full":
                from . import patches

                xyz = radec_to_xyz(ra, dec)
                centers = patches.centers_from_xyz(xyz, weights, int(patch_num))
            else:
                if probe_size < 10 * patch_num:
                    probe_size = int(100_000 * np.sqrt(patch_num))
                step = max(1, len(ra) // probe_size)
                x, y, z = radec_to_xyz(ra[::step], dec[::step])
                centers = kmeans_centers(np.column_stack([x, y, z]), None if weights is None else np.asarray(weights)[::step],
                                         int(patch_num))
        num = None
        if centers is not None:
            if xyz is None:
                xyz = radec_to_xyz(ra, dec)
            patch_ids = nearest_center(xyz, centers.to_3d())
            num = len(centers)
        new = cls._from_columns(ra, dec, patch_ids=patch_ids, num_patches=num, weights=weights, redshifts=redshifts,
                                kappa=kappa, g1=g1, g2=g2, patch_centers=centers, cache_directory=None, xyz=xyz)
        if cache_directory is not None:
            new.to_cache(cache_directory, overwrite=overwrite)
        return new

    @classmethod
    def from_dataframe(cls, cache_directory, dataframe, *, ra_name: str, dec_name: str, weight_name: str | None = None,
                       redshift_name: str | None = None, patch_centers=None, patch_name: str | None = None,
                       patch_num: int | None = None, kappa_name: str | None = None, degrees: bool = True,
                       overwrite: bool = False, progress: bool = False, max_workers: int | None = None,
                       chunksize: int | None = None, probe_size: int = -1, patch_method: str = "probe",
                       g1_name: str | None = None, g2_name: str | None = None, flip_g2: bool = False, **reader_kwargs):
        """Same signature as ``yaw.Catalog.from_dataframe`` (catalog.py:980-1108). ``dataframe`` may
        be a pandas DataFrame or any mapping from column name to array. ``cache_directory`` may be
        ``None`` (nothing is written: the catalogue lives in memory and in HBM); a path gets a cache in
        the reference's on-disk format, readable by both packages (``overwrite`` as in the reference).
        ``kappa_name`` names a column of scalar-field values (convergence, a shear amplitude, ...) for
        ``autocorrelate_scalar`` / ``crosscorrelate_scalar``; ``g1_name`` / ``g2_name`` name the two shear columns for
        ``crosscorrelate_shear`` (frame and ``flip_g2``: see :meth:`from_arrays`). ``patch_method``: see :meth:`from_arrays`."""
        if patch_name is not None and not isinstance(patch_name, str):
            raise TypeError("'patch_name' must be a string")

        def column(name):
            return None if name is None else np.asarray(dataframe[name])

        use_ids = patch_centers is None and patch_name is not None
        return cls.from_arrays(
            column(ra_name), column(dec_name), weights=column(weight_name), redshifts=column(redshift_name),
            kappa=column(kappa_name), g1=column(g1_name), g2=column(g2_name), flip_g2=flip_g2, patch_centers=patch_centers,
            patch_ids=column(patch_name) if use_ids else None, patch_num=patch_num,
            degrees=degrees, cache_directory=cache_directory, overwrite=overwrite, probe_size=probe_size,
            patch_method=patch_method,
        )

    @classmethod
    def from_file(cls, cache_directory, path, *, ra_name: str, dec_name: str, weight_name: str | None = None,
                  redshift_name: str | None = None, patch_centers=None, patch_name: str | None = None,
                  patch_num: int | None = None, kappa_name: str | None = None, degrees: bool = True,
                  g1_name: str | None = None, g2_name: str | None = None, **kwargs):
        """Parquet (``.pqt/.parquet``) or ``.npz`` input (reference: catalog.py:1111-1243; FITS and
        HDF5 readers need libraries that are outside this build's scope)."""
        path = Path(path)
        names = [n for n in (ra_name, dec_name, weight_name, redshift_name, patch_name, kappa_name, g1_name, g2_name) if n is not None]
        if path.suffix.lower() in (".pqt", ".parquet"):
            import pyarrow.parquet as pq

            table = pq.read_table(str(path), columns=names)
            frame = {n: table[n].to_numpy() for n in names}
        elif path.suffix.lower() == ".npz":
            with np.load(str(path)) as data:
                frame = {n: data[n] for n in names}
        else:
            raise ValueError(f"unsupported file type '{path.suffix}' (supported: .pqt, .parquet, .npz)")
        return cls.from_dataframe(cache_directory, frame, ra_name=ra_name, dec_name=dec_name, weight_name=weight_name,
                                  redshift_name=redshift_name, patch_centers=patch_centers, patch_name=patch_name,
                                  patch_num=patch_num, kappa_name=kappa_name, degrees=degrees, g1_name=g1_name, g2_name=g2_name,
                                  **kwargs)

    @classmethod
    def from_random(cls, cache_directory, generator, num_randoms: int, *, patch_centers=None, patch_num: int | None = None,
                    overwrite: bool = False, progress: bool = False, max_workers: int | None = None,
                    chunksize: int | None = None, probe_size: int = -1, patch_method: str = "probe"):
        """Same signature as ``yaw.Catalog.from_random`` (catalog.py:1245-1340): ``num_randoms`` points of ``generator``
        (a :class:`~yet_another_wizz_amd.randoms.BoxRandoms` or :class:`~yet_another_wizz_amd.randoms.HealPixRandoms`), drawn
        from its reseeded stream in calls of ``chunksize`` (default 16 777 216, readers.py:49) -- for a ``BoxRandoms`` the
        reference's catalogue for the same seed, and the generator is left in the reference's end state. Both generators
        are drawn on the GPU when there is one (``engine.draw_box_randoms`` / ``engine.draw_healpix_randoms``, the same
        values), otherwise chunk by chunk on the host; ``dec = arcsin(y)`` is taken on the host either way.
        The columns then go through ``from_arrays``. ``patch_num`` runs this package's k-means (as ``from_dataframe``
        does), whose centres differ from the treecorr centres of the reference; pass ``patch_centers`` for the
        reference's patches; ``patch_method``: see :meth:`from_arrays`. ``progress`` and ``max_workers`` are accepted for
        compatibility and have no effect."""
        from .randoms import BoxRandoms, HealPixRandoms

        num = int(num_randoms)
        if num < 1:
            raise ValueError("catalogue is empty")
        if patch_centers is None and patch_num is None:
            raise ValueError("no patch method specified")
        chunksize = int(chunksize or RANDOM_CHUNKSIZE)
        generator.reseed()
        drawn = None
        if type(generator) is BoxRandoms:
            from . import engine

            drawn = engine.draw_box_randoms(generator, num, chunksize)
        elif type(generator) is HealPixRandoms:
            from . import engine

            drawn = engine.draw_healpix_randoms(generator, num, chunksize)
        if drawn is not None:
            (ra, y, weights, redshifts), _ = drawn
            dec = np.empty_like(y)
            for lo in range(0, num, chunksize):  # numpy's arcsin on the same slices as the reference's chunks
                np.arcsin(y[lo : lo + chunksize], out=dec[lo : lo + chunksize])
            route = "device"
        else:
            chunks = [generator(min(chunksize, num - lo)) for lo in range(0, num, chunksize)]

            def joined(name):
                return np.concatenate([c[name] for c in chunks]) if name in chunks[0] else None

            ra, dec, weights, redshifts = joined("ra"), joined("dec"), joined("weights"), joined("redshifts")
            route = "host"
        new = cls.from_arrays(ra, dec, weights=weights, redshifts=redshifts, patch_centers=patch_centers, patch_num=patch_num,
                              degrees=False, cache_directory=cache_directory, overwrite=overwrite, probe_size=probe_size,
                              patch_method=patch_method)
        new._random_route = route
        return new

    @classmethod
    def from_healpix_map(cls, cache_directory, values, *, weights=None, nested: bool = False, patch_centers=None,
                         patch_num: int | None = None, overwrite: bool = False, probe_size: int = -1, chunksize: int | None = None,
                         patch_method: str = "probe"):
        """A full-sky HEALPix scalar map (a convergence map, a y-map) as a catalogue: one object per unmasked pixel, at the
        pixel's centre, with the map's value as ``kappa`` and, with a weight / coverage map ``weights``, its weight. The
        maps hold ``12 nside^2`` values, ``nside`` a power of two up to 8192, in RING order unless ``nested``; which pixels are
        masked and the order of the objects are those of :func:`healpix.map_pixels <yet_another_wizz_amd.healpix.map_pixels>`.
        Large maps are compacted on the GPU when there is one (the same values, in passes of ``chunksize`` nested pixels);
        ``dec = arcsin(z)`` is taken on the host either way. The columns then go through ``from_arrays``: one of
        ``patch_centers`` / ``patch_num`` is required, as for ``from_random`` (``patch_method``: see :meth:`from_arrays`; with
        ``"full"`` the centres are jackknife regions of the map's footprint). The catalogue has no redshifts: it is the
        scalar side of ``crosscorrelate_scalar_map``."""
        from . import healpix

        if patch_centers is None and patch_num is None:
            raise ValueError("no patch method specified")
        (_, ra, z, kappa, w), route = healpix._map_pixels(values, weights, nested, int(chunksize or 0))
        new = cls.from_arrays(ra, np.arcsin(z), weights=w, kappa=kappa, patch_centers=patch_centers, patch_num=patch_num,
                              degrees=False, cache_directory=cache_directory, overwrite=overwrite, probe_size=probe_size,
                              patch_method=patch_method)
        new._random_route = route
        return new

    def healpix_map(self, nside: int, *, nested: bool = True, weighted: bool = True):
        """HEALPix map (float64[12 nside^2]) of the catalogue: the sum of weights per pixel if it has weights and
        ``weighted``, else the objects per pixel; NESTED numbers unless ``nested=False`` (RING). ``nside`` is a power of two
        up to 8192 (ValueError otherwise). The pixels are those of ``healpix.ang2pix`` for ``(ra, sin dec)``; large
        catalogues are mapped on the GPU when there is one (``healpix.healpix_map``, the same values)."""
        from . import healpix

        order = healpix.nside2order(nside)
        weights = self._w if weighted else None
        return healpix.healpix_map(order, self._ra, self._unit_vectors()[2], weights, nested=nested)

    # ------------------------------------------------------------------ mapping interface
    def __len__(self) -> int:
        return len(self._patches)

    def __getitem__(self, patch_id: int) -> Patch:
        return self._patches[patch_id]

    def __iter__(self):
        yield from sorted(self._patches)

    def __repr__(self) -> str:
        return (f"Catalog(num_patches={self.num_patches}, num_records={len(self._ra)}, "
                f"weights={self.has_weights}, redshifts={self.has_redshifts})")

    @property
    def num_patches(self) -> int:
        return len(self)

    @property
    def has_weights(self) -> bool:
        return self._w is not None

    @property
    def has_redshifts(self) -> bool:
        return self._z is not None

    @property
    def has_kappa(self) -> bool:
        return self._k is not None

    @property
    def has_shear(self) -> bool:
        return self._g1 is not None

    def get_num_records(self) -> tuple:
        return tuple(p.meta.num_records for p in self.values())

    def get_sum_weights(self) -> tuple:
        return tuple(p.meta.sum_weights for p in self.values())

    def get_centers(self) -> AngularCoordinates:
        return AngularCoordinates.from_coords(p.meta.center for p in self.values())

    def get_radii(self) -> AngularDistances:
        return AngularDistances.from_dists(p.meta.radius for p in self.values())

    # ------------------------------------------------------------------ cache on disk
    def to_cache(self, cache_directory, *, overwrite: bool = False) -> None:
        """Write the catalogue in the reference's cache format (``patch_ids.bin``, ``patch_<id>/data.bin``,
        ``patch_<id>/meta.yml``); restore with ``Catalog(cache_directory)`` here or in the reference. A catalogue with shear
        columns raises ``ValueError``: the format has no place for them."""
        import shutil

        import yaml

        if self.has_shear:  # data.bin has no place for the two columns
            raise ValueError("a catalogue with shear columns cannot be written to a cache")
        directory = Path(cache_directory)
        if directory.exists():
            if not overwrite:
                raise FileExistsError(f"cache directory exists and overwrite=False: {directory}")
            if any(directory.iterdir()) and not (directory / PATCH_INFO_FILE).exists():
                raise FileExistsError(f"not a catalog cache, cannot be overwritten: {directory}")
            shutil.rmtree(directory)
        directory.mkdir(parents=True)
        np.arange(self.num_patches, dtype=np.int16).tofile(directory / PATCH_INFO_FILE)
        for pid, patch in self._patches.items():
            patch_dir = directory / PATCH_NAME_TEMPLATE.format(pid)
            patch_dir.mkdir()
            lo, hi = patch._lo, patch._hi
            write_patch_file(patch_dir / PATCH_DATA_FILE, self._ra[lo:hi], self._dec[lo:hi],
                             None if self._w is None else self._w[lo:hi], None if self._z is None else self._z[lo:hi],
                             None if self._k is None else self._k[lo:hi])
            with (patch_dir / PATCH_META_FILE).open("w") as f:
                yaml.safe_dump(patch.meta.to_dict(), f, indent=4)
        self.cache_directory = directory

    # ------------------------------------------------------------------ device layout
    def _unit_vectors(self):
        if self._xyz is None:
            self._xyz = radec_to_xyz(self._ra, self._dec)  # the exact host values the predicate runs on
        return self._xyz

    def build_trees(self, binning=None, *, closed=Closed.right, leafsize: int = 16, force: bool = False,
                    progress: bool = False, max_workers: int | None = None, with_shear: bool = False,
                    with_redshifts: bool = False) -> PatchLayout:
        """Prepare (and cache) the (patch, bin)-sorted layout for ``binning`` (array of edges or
        ``None``).  Keeps the name and arguments of ``yaw.Catalog.build_trees`` (catalog.py:1406-1461);
        no tree is built -- ``leafsize`` is accepted and ignored. ``with_shear`` (no counterpart in the reference) makes a
        binned layout carry ``g1`` / ``g2``, grouped with the other columns, for ``autocorrelate_shear``: a layout of its own
        in the cache, next to the plain one of the same binning; the unbinned layout always carries them. ``with_redshifts``
        (no counterpart either) makes the layout, binned or not, carry the objects' redshifts in its order
        (``PatchLayout.redshifts``) for ``crosscorrelate_delta_sigma``: again a layout of its own in the cache."""
        bins = None if binning is None else (binning if isinstance(binning, Binning) else Binning(binning, closed=closed))
        if with_shear and not self.has_shear:
            raise ValueError("catalog has no 'g1'/'g2' attached")
        if (bins is not None or with_redshifts) and not self.has_redshifts:
            raise ValueError("patch has no 'redshifts' attached")  # trees.py:396-397
        key = None if bins is None else (bins.edges.tobytes(), str(bins.closed), *(("shear",) if with_shear else ()))
        if with_redshifts:
            key = (*(key or ()), "redshifts")
        if not force and key in self._layouts:
            self._active_layout = self._layouts[key]
            return self._active_layout
        x, y, z = self._unit_vectors()
        num_patches = self.num_patches
        if bins is None:
            layout = PatchLayout(x, y, z, self._w, self._patch_off.copy(), num_patches, 1, kappa=self._k, g1=self._g1, g2=self._g2,
                                 redshifts=self._z if with_redshifts else None)
        else:
            num_bins = len(bins)
            bin_idx = bins.assign(self._z)
            patch_of = np.repeat(np.arange(num_patches), np.diff(self._patch_off))
            offsets = np.zeros(num_patches * num_bins + 1, dtype=np.int64)
            shear = (self._g1, self._g2) if with_shear else ()
            extra = (*shear, *((self._z,) if with_redshifts else ()))
            columns = [x, y, z] + [c for c in (self._w, self._k, *extra) if c is not None]  # kappa is binned (and dropped) as the rest
            grouped = False
            if len(x) >= HOST_GROUP_MIN:  # (patch, bin) grouping in one threaded pass; objects outside the binning dropped
                from . import _lib

                seg_key = np.where(bin_idx >= 0, patch_of * num_bins + bin_idx, -1)
                try:
                    columns, sizes = _lib.group_columns(seg_key, num_patches * num_bins, columns)
                    np.cumsum(sizes, out=offsets[1:])
                    grouped = True
                except _lib.YawhipError:  # no library on this machine: numpy below
                    pass
            if not grouped:
                keep = np.flatnonzero(bin_idx >= 0)
                seg_key = patch_of[keep] * num_bins + bin_idx[keep]
                order = keep[_stable_argsort_small(seg_key, num_patches * num_bins)]
                np.cumsum(np.bincount(seg_key, minlength=num_patches * num_bins), out=offsets[1:])
                columns = [c[order] for c in columns]
            rest = iter(columns[3:])
            layout = PatchLayout(columns[0], columns[1], columns[2], None if self._w is None else next(rest), offsets,
                                 num_patches, num_bins, kappa=None if self._k is None else next(rest),
                                 g1=next(rest) if with_shear else None, g2=next(rest) if with_shear else None,
                                 redshifts=next(rest) if with_redshifts else None)
        self._layouts[key] = layout
        self._active_layout = layout  # what the next count_pairs() uses, like the cached trees.pkl
        return layout

    def drop_layouts(self) -> None:
        """Release cached layouts (and with them the device copies)."""
        for layout in self._layouts.values():
            for held in (layout, layout.twin):  # the plain device catalogue and, with kappa, its twin
                if held is None:
                    continue
                for dev in held.device.values():
                    dev.free()
                held.device.clear()
            for handle, _ in layout.handles.values():
                handle.free()
            layout.handles.clear()
        self._layouts.clear()
        self._active_layout = None
