"""Binned values with jackknife samples and their ASCII result files (mirror of ``yaw.correlation.corrdata``,
src/yaw/correlation/corrdata.py:48-260,383-603: ``.dat`` / ``.smp`` / ``.cov`` written and read byte for byte as the
reference does; plotting is out of scope)."""
from __future__ import annotations

import warnings
from pathlib import Path

import numpy as np

from .binning import Binning

__all__ = ["SampledData", "CorrData", "cov_from_samples", "PRECISION", "format_float_fixed_width", "write_data", "write_samples",
           "write_covariance", "load_data", "load_samples"]

# Result files (the reference's ASCII format, corrdata.py:420-605): every number takes PRECISION characters, columns are
# separated by one blank, and a file opens with '# <description>' and a line of right-aligned column names whose first
# two name the bin edges and show the closed side: '(z_low z_high]' or '[z_low z_high)'.
PRECISION = 10
_EDGE_NAMES = {"left": ("[z_low", "z_high)"), "right": ("(z_low", "z_high]")}


def format_float_fixed_width(value: float, width: int) -> str:
    """``value`` in ``width`` characters: a sign column, then as many decimals as fit; digits before the point are never
    cut. Non-finite values are right-aligned words (``nan``, ``inf``, ``-inf``)."""
    if not np.isfinite(value):
        return format(float(value), "").rjust(width)
    text = format(float(value), f" .{width}f")  # the point is always there: 'width' decimals
    return text[: max(width, text.index("."))]


def _header(description: str, names, closed: str) -> str:
    cells = " ".join(name.rjust(PRECISION) for name in (*_EDGE_NAMES[closed], *names))
    return f"# {description}\n#{cells[1:]}\n"  # the '#' takes the place of the first cell's leading blank


def _table(path, description: str, names, closed: str, left, right, columns) -> None:
    """One row per bin: its edges, then the bin's value of every column."""
    lines = [_header(description, names, closed)]
    for row in zip(left, right, *columns):
        lines.append(" ".join(format_float_fixed_width(v, PRECISION) for v in row) + "\n")
    Path(path).write_text("".join(lines))


def write_data(path, description: str, *, zleft, zright, data, error, closed: str) -> None:
    """``.dat``: bin edges, values and their errors."""
    _table(path, description, ("nz", "nz_err"), closed, zleft, zright, (data, error))


def write_samples(path, description: str, *, zleft, zright, samples, closed: str) -> None:
    """``.smp``: bin edges and one column per jackknife sample."""
    _table(path, description, [f"jack_{i}" for i in range(len(samples))], closed, zleft, zright, list(samples))


def write_covariance(path, description: str, *, covariance) -> None:
    """``.cov``: one line per matrix row, each entry in exponent notation followed by a blank; it is not read back."""
    rows = ("".join(format(float(v), f" .{PRECISION - 3}e") + " " for v in row) + "\n" for row in covariance)
    Path(path).write_text(f"# {description}\n" + "".join(rows))


def _closed_side(path) -> str:
    with Path(path).open() as f:
        f.readline()  # the description
        first_name = f.readline().lstrip("#").split()[0]
    return "left" if first_name.startswith("[") else "right"


def load_data(path) -> tuple:
    """``(edges, closed, data, error)`` of a ``.dat`` file."""
    table = np.loadtxt(path, ndmin=2)
    edges = np.concatenate([table[:, 0], table[-1:, 1]])
    return edges, _closed_side(path), table[:, 2], table[:, 3]


def load_samples(path):
    """The jackknife samples of a ``.smp`` file, shape (M, B): its columns after the two edge columns."""
    return np.loadtxt(path, ndmin=2)[:, 2:].T


def cov_from_samples(samples, rowvar: bool = False, kind: str = "full"):
    """Jackknife covariance: np.cov(ddof=0) * (M - 1) (corrdata.py:48-106)."""
    if kind not in ("full", "diag", "var"):
        raise ValueError(f"invalid covariance kind '{kind}'")
    ax_samples, ax_observ = (1, 0) if rowvar else (0, 1)
    blocks = None
    if isinstance(samples, np.ndarray) and samples.ndim == 2:
        joint = samples
    else:
        blocks = [np.asarray(s) for s in samples]
        joint = np.concatenate(blocks, axis=ax_observ)
    n_samples, n_observ = joint.shape[ax_samples], joint.shape[ax_observ]
    if n_samples == 1:
        return np.full((n_observ, n_observ), np.nan)
    cov = np.cov(joint, rowvar=rowvar, ddof=0) * (n_samples - 1)
    cov = np.atleast_2d(cov)
    if kind == "var":
        cov = np.diag(np.diag(cov))
    elif kind == "diag":
        keep = np.diag(np.diag(cov))
        shift = 0
        for block in blocks or []:
            shift += block.shape[ax_observ]
            if shift >= n_observ:
                break
            keep += np.diag(np.diag(cov, k=-shift), k=-shift) + np.diag(np.diag(cov, k=shift), k=shift)
        cov = keep
    return cov


class SampledData:
    """Values in B redshift bins plus M jackknife realisations (corrdata.py:109-260)."""

    __slots__ = ("binning", "data", "samples")

    def __init__(self, binning, data, samples) -> None:
        self.binning = binning
        self.data = np.asarray(data)
        if self.data.shape != (len(binning),):
            raise ValueError("unexpected shape of 'data' array")
        self.samples = np.asarray(samples)
        if self.samples.ndim != 2:
            raise ValueError("'samples' must be two-dimensional")
        if self.samples.shape[1] != len(binning):
            raise ValueError("number of bins for 'data' and 'samples' do not match")

    @property
    def num_bins(self) -> int:
        return len(self.binning)

    @property
    def num_samples(self) -> int:
        return len(self.samples)

    @property
    def covariance(self):
        return cov_from_samples(self.samples)

    @property
    def error(self):
        return np.sqrt(np.diag(self.covariance))

    @property
    def correlation(self):
        cov = self.covariance
        with warnings.catch_warnings():
            warnings.simplefilter("ignore")
            std = np.sqrt(np.diag(cov))
            corr = cov / np.outer(std, std)
        corr[cov == 0] = 0
        return corr

    def __repr__(self) -> str:
        return f"{type(self).__name__}(binning={self.binning}, num_samples={self.num_samples})"

    def __eq__(self, other) -> bool:
        if not isinstance(other, type(self)):
            return NotImplemented
        return (
            self.binning == other.binning
            and np.array_equal(self.data, other.data, equal_nan=True)
            and np.array_equal(self.samples, other.samples, equal_nan=True)
        )

    def _combine(self, other, op):
        if not isinstance(other, type(self)):
            return NotImplemented
        if self.binning != other.binning or self.num_samples != other.num_samples:
            raise ValueError("binning or number of samples do not match")
        return type(self)(self.binning.copy(), op(self.data, other.data), op(self.samples, other.samples))

    def __add__(self, other):
        return self._combine(other, np.add)

    def __sub__(self, other):
        return self._combine(other, np.subtract)

    # descriptions of the result files' headers: every concrete class has its own
    @property
    def _description_data(self) -> str:
        raise NotImplementedError(f"{type(self).__name__} has no result-file description")

    @property
    def _description_samples(self) -> str:
        raise NotImplementedError(f"{type(self).__name__} has no result-file description")

    @property
    def _description_covariance(self) -> str:
        raise NotImplementedError(f"{type(self).__name__} has no result-file description")

    @classmethod
    def from_files(cls, path_prefix):
        """Restore from ``[path_prefix].dat`` (edges, closed side, data) and ``[path_prefix].smp`` (samples), as
        :meth:`to_files` or the reference write them."""
        dat, smp = (Path(path_prefix).with_suffix(ext) for ext in (".dat", ".smp"))
        edges, closed, data, _ = load_data(dat)
        return cls(Binning(edges, closed=closed), data, load_samples(smp))

    def to_files(self, path_prefix) -> None:
        """Write ``[path_prefix].dat`` (bin edges, data, error), ``.smp`` (bin edges, one column per jackknife sample) and
        ``.cov`` (covariance, not read back) in the reference's format. As there, ``with_suffix`` replaces an extension
        the prefix may have."""
        dat, smp, cov = (Path(path_prefix).with_suffix(ext) for ext in (".dat", ".smp", ".cov"))
        left, right, closed = self.binning.left, self.binning.right, str(self.binning.closed)
        write_data(dat, self._description_data, zleft=left, zright=right, data=self.data, error=self.error, closed=closed)
        write_samples(smp, self._description_samples, zleft=left, zright=right, samples=self.samples, closed=closed)
        write_covariance(cov, self._description_covariance, covariance=self.covariance)


class CorrData(SampledData):
    """Correlation function amplitude w(z) with jackknife samples (corrdata.py:383-)."""

    __slots__ = ()

    @property
    def _description_data(self) -> str:
        return "correlation function with symmetric 68% percentile confidence"

    @property
    def _description_samples(self) -> str:
        return f"{self.num_samples} correlation function jackknife samples"

    @property
    def _description_covariance(self) -> str:
        n = self.num_bins
        return f"correlation function covariance matrix ({n}x{n})"
