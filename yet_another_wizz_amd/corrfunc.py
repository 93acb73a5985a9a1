"""DD / DR / RD / RR bundle and the correlation estimators (mirror of
``yaw.correlation.corrfunc``, src/yaw/correlation/corrfunc.py:69-352; file I/O out of scope)."""
from __future__ import annotations

import numpy as np

from .corrdata import CorrData
from .paircounts import NormalisedCounts, NormalisedScalarCounts

__all__ = ["CorrFunc", "ScalarCorrFunc", "ProjectedCorrFunc", "MultipoleCorrFunc", "SignedProjectedCorrFunc", "SignedMultipoleCorrFunc", "AlignmentCorrFunc", "ShapeShapeCorrFunc", "EstimatorError", "davis_peebles", "landy_szalay", "scalar_correlation"]


class EstimatorError(Exception):
    pass


def davis_peebles(*, dd, dr=None, rd=None, rr=None):
    """(DD - DR) / DR, preferring RD when present (corrfunc.py:69-78)."""
    if dr is None and rd is None:
        raise EstimatorError("either 'dr' or 'rd' are required")
    mixed = dr if rd is None else rd
    return (dd - mixed) / mixed


davis_peebles.name = "DP"


def landy_szalay(*, dd, dr, rd=None, rr):
    """((DD - DR) + (RR - RD)) / RR with RD defaulting to DR (corrfunc.py:81-88)."""
    if rd is None:
        rd = dr
    return ((dd - dr) + (rr - rd)) / rr


landy_szalay.name = "LS"


def scalar_correlation(*, dd, dr=None):
    """DD, or DD - DR when DR is given (corrfunc.py:91-97)."""
    return dd if dr is None else dd - dr


scalar_correlation.name = "SC"


class CorrFunc:
    """Normalised pair counts of one correlation scale; ``sample()`` turns them into w(z)."""

    __slots__ = ("_counts_dict",)
    _kinds = ("dd", "dr", "rd", "rr")
    _counts_type = NormalisedCounts

    def __init__(self, dd, dr=None, rd=None, rr=None) -> None:
        self._init(dd, dr=dr, rd=rd, rr=rr)
        if len(self._counts_dict) == 1:
            raise EstimatorError("missing at least one additional pair count")

    def _init(self, dd, **counts) -> None:
        if type(dd) is not self._counts_type:
            raise TypeError(f"pair counts must be of type {self._counts_type}")
        self._counts_dict = dict(dd=dd)
        for kind, count in counts.items():
            if count is None:
                continue
            try:
                dd.is_compatible(count, require=True)
            except ValueError as err:
                raise ValueError(f"pair counts '{kind}' and 'dd' are not compatible") from err
            self._counts_dict[kind] = count

    def __repr__(self) -> str:
        kinds = "|".join(self._counts_dict)
        return (f"{type(self).__name__}(counts={kinds}, auto={self.auto}, binning={self.binning}, "
                f"num_patches={self.num_patches})")

    dd = property(lambda self: self._counts_dict["dd"])
    dr = property(lambda self: self._counts_dict.get("dr"))
    rd = property(lambda self: self._counts_dict.get("rd"))
    rr = property(lambda self: self._counts_dict.get("rr"))

    @property
    def binning(self):
        return self.dd.binning

    @property
    def auto(self) -> bool:
        return self.dd.auto

    @property
    def num_patches(self) -> int:
        return self.dd.num_patches

    @property
    def num_bins(self) -> int:
        return self.dd.num_bins

    def to_dict(self) -> dict:
        return dict(self._counts_dict)

    @classmethod
    def from_dict(cls, counts: dict):
        return cls(**counts)

    def __eq__(self, other) -> bool:
        if type(self) is not type(other):
            return NotImplemented
        mine, theirs = self.to_dict(), other.to_dict()
        return mine.keys() == theirs.keys() and all(mine[k] == theirs[k] for k in mine)

    def is_compatible(self, other, *, require: bool = False) -> bool:
        if type(self) is not type(other):
            if require:
                raise TypeError(f"{type(other)} is not compatible with {type(self)}")
            return False
        return self.dd.is_compatible(other.dd, require=require)

    def get_estimator(self):
        return davis_peebles if self.rr is None else landy_szalay

    def sample(self) -> CorrData:
        """Patch-summed counts -> estimator, for the data and each jackknife sample
        (corrfunc.py:243-272)."""
        estimator = self.get_estimator()
        values, samples = {}, {}
        for kind, counts in self._counts_dict.items():
            resampled = counts.sample_patch_sum()
            values[kind], samples[kind] = resampled.data, resampled.samples
        return CorrData(self.binning, estimator(**values), estimator(**samples))

    def bins_subset(self, item):
        return type(self).from_dict({k: c.bins_subset(item) for k, c in self._counts_dict.items()})

    def patches_subset(self, item):
        return type(self).from_dict({k: c.patches_subset(item) for k, c in self._counts_dict.items()})


class ScalarCorrFunc(CorrFunc):
    """Scalar-field pair counts of one correlation scale (corrfunc.py:355-399): ``dd`` and optionally ``dr``, both
    ``NormalisedScalarCounts``; the estimator is DD, or DD - DR. Everything else -- ``sample()``, ``to_dict`` /
    ``from_dict``, ``==``, ``is_compatible``, the bin and patch subsets -- is ``CorrFunc``'s."""

    __slots__ = ()
    _kinds = ("dd", "dr")
    _counts_type = NormalisedScalarCounts

    def __init__(self, dd, dr=None) -> None:
        self._init(dd, dr=dr)

    def get_estimator(self):
        return scalar_correlation


class ProjectedCorrFunc:
    """The pair counts of one scale of the projected clustering binned in the line-of-sight separation ``pi``
    (``autocorrelate_projected(pi_bins=...)``; no counterpart in the reference): ``pi_edges`` f64[n_pi + 1], from 0 and
    strictly ascending, and ``pi_bins``, a tuple of ``n_pi`` ``CorrFunc(dd, dr, None, rr)`` -- bin 0 holds the pairs with
    ``pi`` in ``[0, pe[1]]``, bin j those in ``(pe[j], pe[j + 1]]``. All bins hold the same kinds of counts on one binning
    and one set of patches.

    ``sample_xi()`` is ``xi(r_p, pi_j)`` per pi bin, ``sample()`` the summed ``w_p(r_p) = 2 sum_j dpi_j xi_j`` and
    ``cylinder()`` the single-cylinder measurement over the pi-summed counts. A pi bin whose RR (DR for Davis-Peebles) is
    empty in some redshift bin gives NaN there, in ``sample_xi()`` and in the sum of ``sample()``, as ``CorrFunc.sample()``
    does: nothing is masked. ``to_dict`` / ``from_dict``, ``==`` and the bin and patch subsets go bin by bin through
    ``CorrFunc``'s."""

    __slots__ = ("pi_edges", "pi_bins")

    def __init__(self, pi_edges, pi_bins) -> None:
        edges = np.array(pi_edges, dtype=np.float64)
        bins = tuple(pi_bins)
        if edges.ndim != 1 or len(edges) != len(bins) + 1 or len(bins) < 1:
            raise ValueError("'pi_edges' must hold one edge more than there are pi bins, and there is at least one bin")
        if edges[0] != 0.0 or not np.all(np.isfinite(edges)) or not np.all(np.diff(edges) > 0.0):
            raise ValueError("'pi_edges' must start at 0, be finite and ascend strictly")
        for cf in bins:
            if type(cf) is not CorrFunc:
                raise TypeError(f"the pi bins must be of type {CorrFunc}")
            bins[0].is_compatible(cf, require=True)
            if cf.to_dict().keys() != bins[0].to_dict().keys():
                raise ValueError("the pi bins must hold the same kinds of pair counts")
        edges.setflags(write=False)
        self.pi_edges = edges
        self.pi_bins = bins

    def __repr__(self) -> str:
        return f"{type(self).__name__}(num_pi={self.num_pi}, pi_max={self.pi_edges[-1]}, pi_bins[0]={self.pi_bins[0]!r})"

    binning = property(lambda self: self.pi_bins[0].binning)
    auto = property(lambda self: self.pi_bins[0].auto)
    num_patches = property(lambda self: self.pi_bins[0].num_patches)
    num_bins = property(lambda self: self.pi_bins[0].num_bins)
    num_pi = property(lambda self: len(self.pi_bins))

    def to_dict(self) -> dict:
        return dict(pi_edges=self.pi_edges.copy(), pi_bins=[cf.to_dict() for cf in self.pi_bins])

    @classmethod
    def from_dict(cls, state: dict):
        return cls(state["pi_edges"], [CorrFunc.from_dict(counts) for counts in state["pi_bins"]])

    def __eq__(self, other) -> bool:
        if type(self) is not type(other):
            return NotImplemented
        return np.array_equal(self.pi_edges, other.pi_edges) and self.pi_bins == other.pi_bins

    def is_compatible(self, other, *, require: bool = False) -> bool:
        if type(self) is not type(other):
            if require:
                raise TypeError(f"{type(other)} is not compatible with {type(self)}")
            return False
        if not np.array_equal(self.pi_edges, other.pi_edges):
            if require:
                raise ValueError("the pi edges differ")
            return False
        return self.pi_bins[0].is_compatible(other.pi_bins[0], require=require)

    def sample_xi(self) -> list:
        """``xi(r_p, pi_j)`` per pi bin: ``CorrFunc.sample()`` of each, Landy-Szalay or (without RR) Davis-Peebles, for the
        data and every jackknife sample."""
        return [cf.sample() for cf in self.pi_bins]

    def sample(self) -> CorrData:
        """``w_p = 2 sum_j dpi_j xi_j``, summed in the order of the pi bins for the data and for each jackknife sample
        separately; errors and covariance are those of the summed samples."""
        data, samples = 0.0, 0.0
        for dpi, xi in zip(np.diff(self.pi_edges), self.sample_xi()):
            data, samples = data + dpi * xi.data, samples + dpi * xi.samples
        return CorrData(self.binning, 2.0 * data, 2.0 * samples)

    def cylinder(self) -> CorrFunc:
        """The single-cylinder measurement ``|pi| <= pi_edges[-1]``: the ``CorrFunc`` over the counts summed over the pi bins
        (in their order), on the bins' one normalisation -- what ``autocorrelate_projected(pi_bins=None)`` counts."""
        summed = {}
        for kind, first in self.pi_bins[0].to_dict().items():
            counts = first.counts
            for cf in self.pi_bins[1:]:
                counts = counts + cf.to_dict()[kind].counts
            summed[kind] = NormalisedCounts(counts, first.sum_weights)
        return CorrFunc.from_dict(summed)

    def bins_subset(self, item):
        return type(self)(self.pi_edges, [cf.bins_subset(item) for cf in self.pi_bins])

    def patches_subset(self, item):
        return type(self)(self.pi_edges, [cf.patches_subset(item) for cf in self.pi_bins])


class MultipoleCorrFunc:
    """The pair counts of one scale of the redshift-space clustering binned in ``mu = pi / s``
    (``autocorrelate_multipoles``; no counterpart in the reference): ``mu_edges`` f64[n_mu + 1], from 0 to 1 and strictly
    ascending, and ``mu_bins``, a tuple of ``n_mu`` ``CorrFunc(dd, dr, None, rr)`` -- bin 0 holds the pairs with ``mu`` in
    ``[0, mu_1]``, bin j those in ``(mu_j, mu_{j+1}]``; ``mu`` is unsigned. All bins hold the same kinds of counts on one
    binning and one set of patches.

    ``sample_xi()`` is ``xi(s, mu_j)`` per mu bin, ``sample(ell)`` the multipole ``xi_ell(s)`` and ``sample_multipoles()``
    several of them. A mu bin whose RR (DR for Davis-Peebles) is empty in some redshift bin gives NaN there, in
    ``sample_xi()`` and in EVERY multipole, as ``CorrFunc.sample()`` does: nothing is masked. ``to_dict`` / ``from_dict``,
    ``==`` and the bin and patch subsets go bin by bin through ``CorrFunc``'s, as ``ProjectedCorrFunc``'s do."""

    __slots__ = ("mu_edges", "mu_bins")

    def __init__(self, mu_edges, mu_bins) -> None:
        edges = np.array(mu_edges, dtype=np.float64)
        bins = tuple(mu_bins)
        if edges.ndim != 1 or len(edges) != len(bins) + 1 or len(bins) < 1:
            raise ValueError("'mu_edges' must hold one edge more than there are mu bins, and there is at least one bin")
        if edges[0] != 0.0 or edges[-1] != 1.0 or not np.all(np.isfinite(edges)) or not np.all(np.diff(edges) > 0.0):
            raise ValueError("'mu_edges' must start at 0, end at 1, be finite and ascend strictly")
        for cf in bins:
            if type(cf) is not CorrFunc:
                raise TypeError(f"the mu bins must be of type {CorrFunc}")
            bins[0].is_compatible(cf, require=True)
            if cf.to_dict().keys() != bins[0].to_dict().keys():
                raise ValueError("the mu bins must hold the same kinds of pair counts")
        edges.setflags(write=False)
        self.mu_edges = edges
        self.mu_bins = bins

    def __repr__(self) -> str:
        return f"{type(self).__name__}(num_mu={self.num_mu}, mu_bins[0]={self.mu_bins[0]!r})"

    binning = property(lambda self: self.mu_bins[0].binning)
    auto = property(lambda self: self.mu_bins[0].auto)
    num_patches = property(lambda self: self.mu_bins[0].num_patches)
    num_bins = property(lambda self: self.mu_bins[0].num_bins)
    num_mu = property(lambda self: len(self.mu_bins))

    def to_dict(self) -> dict:
        return dict(mu_edges=self.mu_edges.copy(), mu_bins=[cf.to_dict() for cf in self.mu_bins])

    @classmethod
    def from_dict(cls, state: dict):
        return cls(state["mu_edges"], [CorrFunc.from_dict(counts) for counts in state["mu_bins"]])

    def __eq__(self, other) -> bool:
        if type(self) is not type(other):
            return NotImplemented
        return np.array_equal(self.mu_edges, other.mu_edges) and self.mu_bins == other.mu_bins

    def is_compatible(self, other, *, require: bool = False) -> bool:
        if type(self) is not type(other):
            if require:
                raise TypeError(f"{type(other)} is not compatible with {type(self)}")
            return False
        if not np.array_equal(self.mu_edges, other.mu_edges):
            if require:
                raise ValueError("the mu edges differ")
            return False
        return self.mu_bins[0].is_compatible(other.mu_bins[0], require=require)

    def sample_xi(self) -> list:
        """``xi(s, mu_j)`` per mu bin: ``CorrFunc.sample()`` of each, Landy-Szalay or (without RR) Davis-Peebles, for the data
        and every jackknife sample."""
        return [cf.sample() for cf in self.mu_bins]

    def legendre_weights(self, ell: int) -> np.ndarray:
        """``I_ell,j = int_{mu_j}^{mu_{j+1}} P_ell(mu) dmu`` per mu bin, f64[n_mu], from the antiderivative of the Legendre
        polynomial. ``ell`` is even and in 0 ... 8: ``mu`` is unsigned, so the odd multipoles are not measured."""
        if isinstance(ell, (bool, np.bool_)) or not isinstance(ell, (int, np.integer)) or ell < 0 or ell > 8 or ell % 2:
            raise ValueError(f"ell must be an even integer in 0 ... 8 (mu is unsigned), not {ell!r}")
        primitive = np.polynomial.legendre.Legendre.basis(int(ell)).integ()
        return np.diff(primitive(self.mu_edges))

    def sample(self, ell: int = 0) -> CorrData:
        """``xi_ell(s) = (2 ell + 1) sum_j xi_j I_ell,j`` (``legendre_weights``), summed in the order of the mu bins for the
        data and for each jackknife sample separately; errors and covariance are those of the summed samples. With equal
        weights over [0, 1] this is the usual ``(2 ell + 1) int_0^1 xi(s, mu) P_ell(mu) dmu`` with ``xi`` constant per bin."""
        data, samples = 0.0, 0.0
        for weight, xi in zip(self.legendre_weights(ell), self.sample_xi()):
            data, samples = data + weight * xi.data, samples + weight * xi.samples
        return CorrData(self.binning, (2 * int(ell) + 1) * data, (2 * int(ell) + 1) * samples)

    def sample_multipoles(self, ells=(0, 2, 4)) -> tuple:
        """``sample(ell)`` for every ``ell`` of ``ells``."""
        return tuple(self.sample(ell) for ell in ells)

    def bins_subset(self, item):
        return type(self)(self.mu_edges, [cf.bins_subset(item) for cf in self.mu_bins])

    def patches_subset(self, item):
        return type(self)(self.mu_edges, [cf.patches_subset(item) for cf in self.mu_bins])


class _SignedBinnedCorrFunc:
    """What the two results with a signed line of sight share: ``edges`` f64[n + 1], finite and strictly ascending with
    ``edges[0] == -edges[-1]``, and ``n`` ``CorrFunc`` of the same kinds on one binning and one set of patches -- bin 0 holds
    ``[e[0], e[1]]``, bin j ``(e[j], e[j + 1]]``. The sign is that of the count: second sample minus first. A subclass names
    the second binning (``_name``: its edges and bins are the attributes ``<name>_edges``, ``<name>_bins`` and the keys of
    ``to_dict``), checks the ends of the edges and says what ``folded()`` builds."""

    __slots__ = ("_edges", "_bins")
    _name = ""
    _folded_type = None

    def __init__(self, edges, bins) -> None:
        name = self._name
        edges = np.array(edges, dtype=np.float64)
        bins = tuple(bins)
        if edges.ndim != 1 or len(edges) != len(bins) + 1 or len(bins) < 1:
            raise ValueError(f"'{name}_edges' must hold one edge more than there are {name} bins, and there is at least one bin")
        if not np.all(np.isfinite(edges)) or not np.all(np.diff(edges) > 0.0) or edges[0] != -edges[-1]:
            raise ValueError(f"'{name}_edges' must be finite, ascend strictly and span zero symmetrically at the ends")
        self._check_ends(edges)
        for cf in bins:
            if type(cf) is not CorrFunc:
                raise TypeError(f"the {name} bins must be of type {CorrFunc}")
            bins[0].is_compatible(cf, require=True)
            if cf.to_dict().keys() != bins[0].to_dict().keys():
                raise ValueError(f"the {name} bins must hold the same kinds of pair counts")
        edges.setflags(write=False)
        self._edges = edges
        self._bins = bins

    def _check_ends(self, edges) -> None:
        pass

    binning = property(lambda self: self._bins[0].binning)
    auto = property(lambda self: self._bins[0].auto)
    num_patches = property(lambda self: self._bins[0].num_patches)
    num_bins = property(lambda self: self._bins[0].num_bins)

    def to_dict(self) -> dict:
        return {f"{self._name}_edges": self._edges.copy(), f"{self._name}_bins": [cf.to_dict() for cf in self._bins]}

    @classmethod
    def from_dict(cls, state: dict):
        return cls(state[f"{cls._name}_edges"], [CorrFunc.from_dict(counts) for counts in state[f"{cls._name}_bins"]])

    def __eq__(self, other) -> bool:
        if type(self) is not type(other):
            return NotImplemented
        return np.array_equal(self._edges, other._edges) and self._bins == other._bins

    def is_compatible(self, other, *, require: bool = False) -> bool:
        if type(self) is not type(other):
            if require:
                raise TypeError(f"{type(other)} is not compatible with {type(self)}")
            return False
        if not np.array_equal(self._edges, other._edges):
            if require:
                raise ValueError(f"the {self._name} edges differ")
            return False
        return self._bins[0].is_compatible(other._bins[0], require=require)

    def sample_xi(self) -> list:
        """The correlation function per signed bin: ``CorrFunc.sample()`` of each -- Landy-Szalay with RR, else
        Davis-Peebles -- for the data and every jackknife sample."""
        return [cf.sample() for cf in self._bins]

    def _weighted_sum(self, weights, factor: float) -> CorrData:
        """``factor * sum_j weights[j] xi_j``, summed in the order of the bins, data and jackknife samples separately."""
        data, samples = 0.0, 0.0
        for weight, xi in zip(weights, self.sample_xi()):
            data, samples = data + weight * xi.data, samples + weight * xi.samples
        return CorrData(self.binning, factor * data, factor * samples)

    def folded(self):
        """The unsigned result over the counts of mirrored bins summed: with ``2 m`` bins whose edges are symmetric about 0,
        folded bin j holds bin ``m + j`` plus bin ``m - 1 - j`` on the bins' one normalisation, over the edges ``e[m:]``.
        Possible only where the edges are symmetric about 0 and 0 is an edge (``ValueError`` otherwise)."""
        edges, m = self._edges, len(self._bins) // 2
        if len(self._bins) % 2 or edges[m] != 0.0 or not np.array_equal(edges, -edges[::-1]):
            raise ValueError(f"folding needs {self._name} edges that are symmetric about 0 with 0 among them")
        bins = []
        for upper, lower in zip(self._bins[m:], self._bins[:m][::-1]):
            mirrored = lower.to_dict()
            bins.append(CorrFunc.from_dict({kind: NormalisedCounts(counts.counts + mirrored[kind].counts, counts.sum_weights)
                                            for kind, counts in upper.to_dict().items()}))
        return self._folded_type(edges[m:], bins)

    def bins_subset(self, item):
        return type(self)(self._edges, [cf.bins_subset(item) for cf in self._bins])

    def patches_subset(self, item):
        return type(self)(self._edges, [cf.patches_subset(item) for cf in self._bins])


class SignedProjectedCorrFunc(_SignedBinnedCorrFunc):
    """The pair counts of one scale of the projected cross-correlation of two samples binned in the SIGNED line-of-sight
    separation ``pi = chi_2 - chi_1`` (``crosscorrelate_projected(signed=True)``; no counterpart in the reference):
    ``pi_edges`` f64[n + 1], strictly ascending from ``-pi_max`` to ``pi_max`` and symmetric inside or not, and ``pi_bins``, a
    tuple of ``n`` ``CorrFunc(dd, dr, rd, rr)`` -- bin 0 holds ``[pe[0], pe[1]]``, bin j ``(pe[j], pe[j + 1]]``; positive where
    the object of the second sample lies behind.

    ``sample_xi()`` is ``xi(r_p, pi_j)`` per bin, ``sample()`` the summed ``w_p(r_p) = sum_j dpi_j xi_j`` -- the bins cover
    both signs, so there is no factor 2 -- and ``folded()`` the ``ProjectedCorrFunc`` of ``signed=False``. An empty RR (DR)
    gives NaN as in ``ProjectedCorrFunc``. ``to_dict`` / ``from_dict``, ``==``, ``is_compatible`` and the bin and patch
    subsets go bin by bin through ``CorrFunc``'s."""

    __slots__ = ()
    _name = "pi"
    _folded_type = ProjectedCorrFunc

    pi_edges = property(lambda self: self._edges)
    pi_bins = property(lambda self: self._bins)
    num_pi = property(lambda self: len(self._bins))

    def __repr__(self) -> str:
        return f"{type(self).__name__}(num_pi={self.num_pi}, pi_max={self.pi_edges[-1]}, pi_bins[0]={self.pi_bins[0]!r})"

    def sample(self) -> CorrData:
        """``w_p = sum_j dpi_j xi_j`` over the signed bins; errors and covariance are those of the summed samples."""
        return self._weighted_sum(np.diff(self.pi_edges), 1.0)


class SignedMultipoleCorrFunc(_SignedBinnedCorrFunc):
    """The pair counts of one scale of the redshift-space cross-correlation of two samples binned in the SIGNED
    ``mu = pi / s``, ``pi = chi_2 - chi_1`` (``crosscorrelate_multipoles(signed=True)``; no counterpart in the reference):
    ``mu_edges`` f64[n + 1], strictly ascending from -1 to 1, and ``mu_bins``, a tuple of ``n`` ``CorrFunc(dd, dr, rd, rr)`` --
    bin 0 holds ``[-1, mu_1]``, bin j ``(mu_j, mu_{j+1}]``.

    ``sample_xi()`` is ``xi(s, mu_j)`` per bin, ``sample(ell)`` the multipole ``xi_ell(s)`` of EVERY integer ``ell`` in
    0 ... 8 -- the odd ones are what the sign is kept for -- ``sample_multipoles()`` several of them and ``folded()`` the
    ``MultipoleCorrFunc`` of ``signed=False``. The rest is ``SignedProjectedCorrFunc``'s."""

    __slots__ = ()
    _name = "mu"
    _folded_type = MultipoleCorrFunc

    mu_edges = property(lambda self: self._edges)
    mu_bins = property(lambda self: self._bins)
    num_mu = property(lambda self: len(self._bins))

    def _check_ends(self, edges) -> None:
        if edges[0] != -1.0 or edges[-1] != 1.0:
            raise ValueError("'mu_edges' must start at -1 and end at 1")

    def __repr__(self) -> str:
        return f"{type(self).__name__}(num_mu={self.num_mu}, mu_bins[0]={self.mu_bins[0]!r})"

    def legendre_weights(self, ell: int) -> np.ndarray:
        """``I_ell,j = int_{mu_j}^{mu_{j+1}} P_ell(mu) dmu`` per mu bin, f64[n_mu], from the antiderivative of the Legendre
        polynomial, for every integer ``ell`` in 0 ... 8."""
        if isinstance(ell, (bool, np.bool_)) or not isinstance(ell, (int, np.integer)) or ell < 0 or ell > 8:
            raise ValueError(f"ell must be an integer in 0 ... 8, not {ell!r}")
        primitive = np.polynomial.legendre.Legendre.basis(int(ell)).integ()
        return np.diff(primitive(self.mu_edges))

    def sample(self, ell: int = 0) -> CorrData:
        """``xi_ell(s) = (2 ell + 1) / 2 sum_j xi_j I_ell,j`` (``legendre_weights``): the usual
        ``(2 ell + 1) / 2 int_{-1}^{1} xi(s, mu) P_ell(mu) dmu`` with ``xi`` constant per bin."""
        return self._weighted_sum(self.legendre_weights(ell), (2 * int(ell) + 1) / 2.0)

    def sample_multipoles(self, ells=(0, 1, 2, 3, 4)) -> tuple:
        """``sample(ell)`` for every ``ell`` of ``ells``."""
        return tuple(self.sample(ell) for ell in ells)


class AlignmentCorrFunc:
    """The sums of one scale of the projected position-shape correlation (``crosscorrelate_alignment``; no counterpart in the
    reference): ``pi_edges`` f64[n_pi + 1], from 0 and strictly ascending, and ``pi_bins``, a tuple of ``n_pi`` dicts of
    ``NormalisedCounts`` -- bin 0 holds the pairs with ``pi`` in ``[0, pe[1]]``, bin j those in ``(pe[j], pe[j + 1]]``. Each
    dict holds the planes of shapes x density, ``t_sd``, ``x_sd``, ``w_sd``, those of shapes x density randoms, ``t_sr``,
    ``x_sr``, ``w_sr`` (T and X are signed sums), and optionally ``rr``, the pair count of shape randoms x density randoms.
    The slot ``[bin, p, q]`` of every tensor pairs patch ``p`` of the density side with patch ``q`` of the shape side.

    Sign convention: the device sums the TANGENTIAL ellipticity ``e_t`` of a shape about the density object, which is
    negative for a shape that points at it. ``w_g+`` is positive for radial alignment, so the sign is flipped here, once:
    with ``/n`` the division by the product of the two weight sums of the redshift bin and ``N`` the normalising pair count
    -- ``rr`` where given, else ``w_sr`` -- per pi bin j, for the data and every jackknife sample separately,

        xi_plus_j  = -(t_sd/n - t_sr/n) / (N/n)
        xi_cross_j =  (x_sd/n - x_sr/n) / (N/n)
        sample("plus" | "cross") = 2 sum_j dpi_j xi_j     -> w_g+(r_p), w_gx(r_p)

    ``sample_xi(component)`` gives the pi bins. An empty ``N`` gives NaN there and in the sum: nothing is masked.
    ``to_dict`` / ``from_dict``, ``==``, ``is_compatible`` and the bin and patch subsets go bin by bin."""

    __slots__ = ("pi_edges", "pi_bins")
    _required = ("t_sd", "x_sd", "w_sd", "t_sr", "x_sr", "w_sr")  # (the first of them stands for the binning and the patches)

    def __init__(self, pi_edges, pi_bins) -> None:
        edges = np.array(pi_edges, dtype=np.float64)
        bins = tuple(dict(planes) for planes in pi_bins)
        if edges.ndim != 1 or len(edges) != len(bins) + 1 or len(bins) < 1:
            raise ValueError("'pi_edges' must hold one edge more than there are pi bins, and there is at least one bin")
        if edges[0] != 0.0 or not np.all(np.isfinite(edges)) or not np.all(np.diff(edges) > 0.0):
            raise ValueError("'pi_edges' must start at 0, be finite and ascend strictly")
        first = bins[0].get(self._required[0])
        for planes in bins:
            if planes.keys() != bins[0].keys() or not set(self._required) <= planes.keys() <= {*self._required, "rr"}:
                raise ValueError(f"every pi bin holds the planes {self._required}, and all or none of them 'rr'")
            for kind, counts in planes.items():
                if type(counts) is not NormalisedCounts:
                    raise TypeError(f"the planes must be of type {NormalisedCounts}")
                try:
                    first.is_compatible(counts, require=True)
                except ValueError as err:
                    raise ValueError(f"plane '{kind}' and '{self._required[0]}' of the first pi bin are not compatible") from err
        edges.setflags(write=False)
        self.pi_edges = edges
        self.pi_bins = bins

    def __repr__(self) -> str:
        return (f"{type(self).__name__}(num_pi={self.num_pi}, pi_max={self.pi_edges[-1]}, planes={'|'.join(self.pi_bins[0])}, "
                f"binning={self.binning}, num_patches={self.num_patches})")

    binning = property(lambda self: self.pi_bins[0][self._required[0]].binning)
    num_patches = property(lambda self: self.pi_bins[0][self._required[0]].num_patches)
    num_bins = property(lambda self: len(self.binning))
    num_pi = property(lambda self: len(self.pi_bins))

    def to_dict(self) -> dict:
        return dict(pi_edges=self.pi_edges.copy(), pi_bins=[dict(planes) for planes in self.pi_bins])

    @classmethod
    def from_dict(cls, state: dict):
        return cls(state["pi_edges"], state["pi_bins"])

    def __eq__(self, other) -> bool:
        if type(self) is not type(other):
            return NotImplemented
        return (np.array_equal(self.pi_edges, other.pi_edges) and len(self.pi_bins) == len(other.pi_bins)
                and all(mine.keys() == theirs.keys() and all(mine[k] == theirs[k] for k in mine)
                        for mine, theirs in zip(self.pi_bins, other.pi_bins)))

    def is_compatible(self, other, *, require: bool = False) -> bool:
        if type(self) is not type(other):
            if require:
                raise TypeError(f"{type(other)} is not compatible with {type(self)}")
            return False
        if not np.array_equal(self.pi_edges, other.pi_edges):
            if require:
                raise ValueError("the pi edges differ")
            return False
        return self.pi_bins[0][self._required[0]].is_compatible(other.pi_bins[0][self._required[0]], require=require)

    @staticmethod
    def _component(component: str):
        if component not in ("plus", "cross"):
            raise ValueError(f"component must be 'plus' or 'cross', not {component!r}")
        return ("t", -1.0) if component == "plus" else ("x", 1.0)

    def sample_xi(self, component: str = "plus") -> list:
        """``xi_plus_j`` or ``xi_cross_j`` per pi bin as ``CorrData``, for the data and every jackknife sample."""
        plane, sign = self._component(component)
        out = []
        for planes in self.pi_bins:
            sd, sr = planes[f"{plane}_sd"].sample_patch_sum(), planes[f"{plane}_sr"].sample_patch_sum()
            norm = planes.get("rr", planes["w_sr"]).sample_patch_sum()
            with np.errstate(divide="ignore", invalid="ignore"):  # an empty N: NaN, whatever the numerator holds
                data = np.where(norm.data == 0.0, np.nan, sign * (sd.data - sr.data) / norm.data)
                samples = np.where(norm.samples == 0.0, np.nan, sign * (sd.samples - sr.samples) / norm.samples)
            out.append(CorrData(self.binning, data, samples))
        return out

    def sample(self, component: str = "plus") -> CorrData:
        """``w_g+(r_p)`` ("plus") or ``w_gx(r_p)`` ("cross"): ``2 sum_j dpi_j xi_j``, summed in the order of the pi bins for
        the data and for each jackknife sample separately; errors and covariance are those of the summed samples."""
        data, samples = 0.0, 0.0
        for dpi, xi in zip(np.diff(self.pi_edges), self.sample_xi(component)):
            data, samples = data + dpi * xi.data, samples + dpi * xi.samples
        return CorrData(self.binning, 2.0 * data, 2.0 * samples)

    def bins_subset(self, item):
        return type(self)(self.pi_edges, [{k: c.bins_subset(item) for k, c in planes.items()} for planes in self.pi_bins])

    def patches_subset(self, item):
        return type(self)(self.pi_edges, [{k: c.patches_subset(item) for k, c in planes.items()} for planes in self.pi_bins])


class ShapeShapeCorrFunc(AlignmentCorrFunc):
    """The sums of one scale of the projected shape-shape correlation (``autocorrelate_alignment``; no counterpart in the
    reference): ``pi_edges`` and ``pi_bins`` as ``AlignmentCorrFunc`` has them, each pi bin a dict of ``NormalisedCounts``
    with the planes of shapes x shapes -- ``pp``, ``xx``, ``px`` (signed sums of ``w_a w_b et_a et_b``, ``w_a w_b ex_a ex_b``
    and ``w_a w_b (et_a ex_b + ex_a et_b)``, both ellipticities rotated to the great circle through the pair) and ``w`` (the
    sum of ``w_a w_b``) -- and optionally ``rr``, the pair count of the shape randoms with themselves.

    Sign convention: the device sums the TANGENTIAL ellipticity ``et``, as for ``AlignmentCorrFunc``, and ``e+ = -et``. In
    ``pp`` the two signs cancel; ``px`` holds one of them, so the ``+x`` component flips it here, once. With ``/n`` the
    division by a count's own normalisation, per pi bin j, for the data and every jackknife sample separately,

        with randoms:     xi_j = (pp/n) / (rr/n)          S+S+ over R_S R_S
        without randoms:  xi_j = pp / w                   the pair-weighted mean product, as autocorrelate_shear reports xi_+
        sample("plus" | "cross" | "plus_cross") = 2 sum_j dpi_j xi_j     -> w_++(r_p), w_xx(r_p), w_+x(r_p)

    from ``pp``, ``xx`` and ``-px``. The two estimators differ by the factor ``1 + xi_gg`` of the shape sample's own
    clustering (``w/n`` over ``rr/n``). ``plus_cross`` is parity-odd and vanishes without systematics: the null test.
    ``sample_xi(component)`` gives the pi bins. An empty denominator gives NaN there and in the sum: nothing is masked.
    ``to_dict`` / ``from_dict``, ``==``, ``is_compatible`` and the bin and patch subsets go bin by bin."""

    __slots__ = ()
    _required = ("pp", "xx", "px", "w")
    _planes = dict(plus=("pp", 1.0), cross=("xx", 1.0), plus_cross=("px", -1.0))

    def sample_xi(self, component: str = "plus") -> list:
        """``xi_j`` of the component per pi bin as ``CorrData``, for the data and every jackknife sample."""
        if component not in self._planes:
            raise ValueError(f"component must be 'plus', 'cross' or 'plus_cross', not {component!r}")
        plane, sign = self._planes[component]
        out = []
        for planes in self.pi_bins:
            num = planes[plane].sample_patch_sum()
            norm = planes.get("rr", planes["w"]).sample_patch_sum()
            with np.errstate(divide="ignore", invalid="ignore"):  # an empty denominator: NaN, whatever the numerator holds
                data = np.where(norm.data == 0.0, np.nan, sign * num.data / norm.data)
                samples = np.where(norm.samples == 0.0, np.nan, sign * num.samples / norm.samples)
            out.append(CorrData(self.binning, data, samples))
        return out
