"""Descriptor tools — the drop-in for ``mdapy.potential_tool``, limited to ``fps_sample``, ``PCA`` and ``rmse``: what consumes the
descriptors of ``NEP.get_descriptor`` / ``get_latentspace`` in an active-learning loop.

    picks = fps_sample(100, descriptors)                       # farthest-point sampling from row 0
    picks, distance = fps_sample(100, descriptors, return_distance=True)
    xy = PCA(2).fit_transform(descriptors)

``fps_sample`` keeps every row's minimum distance to the rows selected so far and picks the arg-max, ``n_sample - 1`` times; nothing
is excluded, a row already selected simply has minimum 0 (a table of identical rows gives ``[start_idx, 0, 0, ...]``).  Each pick
is one pass over the table on the GPU (csrc/sample.hip; tests/_fps_ref.py restates it in numpy), queued without the host looking
in between.  ``PCA`` takes the column means, the covariance (divisor N - 1) and the projection on the GPU; the eigenvectors of the
(D, D) matrix come from ``numpy.linalg.eigh`` on the host, largest eigenvalue first, each with its entry of largest magnitude
positive.

What differs from the reference:

* **squared distances**: the rows are compared by their squared distances; the reference compares the roots.  The root is
  monotone, so a pick differs only where two candidates' squared minima differ and their roots round to the same double.
* **the pinned sum**: the squared distance of a row a to the current point b is ``acc = acc + (a_k - b_k) * (a_k - b_k)`` for
  k = 0 .. D-1: one accumulator, ascending k, binary64, no fused multiply-add.  This sum is the contract — it does not depend on
  the launch shape, and the two kernels (one launch per pick; one workgroup looping over the picks of a small table) give the
  same bits.  ``np.linalg.norm`` sums in numpy's own pairwise order.
* **ties**: of equal values the lowest row index is picked, as ``np.argmax`` does.
* **errors**: wrong arguments raise ``ValueError`` with the reference's messages (the reference ``assert``s).  A table that holds a
  value that is not finite raises ``ValueError`` as well — checked on the device in the first pass; the reference goes on and
  picks the first NaN row for ever.  (With ``n_sample=1`` there is no pass and nothing is checked.)
* **return_distance** (an extension): also the (N,) distances of every row to the selected set — the root, taken here on the
  host, of the minima the kernel keeps after its last pass, i.e. to all picks but the last one; users cut ``n_sample`` with it.
* **small inputs**: ``PCA.fit_transform`` needs at least two rows; ``n_components`` above the number of columns keeps all the
  columns, as slicing does in the reference.  The kernels take up to 128 columns for the PCA and 1024 for the sampling.
* the sums of the PCA run in a fixed order on the device: two runs give the same bits; they differ from numpy's in the last bits.

Not here: the rest of the reference's module (the GPUMD and VASP file helpers, ``get_eos``, the stacking-fault helpers, the plots)."""
import numpy as np

from . import kernels
from .devarray import HArray, have_gpu

__all__ = ["fps_sample", "PCA", "rmse"]


def rmse(predictions, targets):
    """root-mean-square error of two arrays, on the host"""
    error = np.asarray(predictions) - np.asarray(targets)
    return np.sqrt(np.mean(np.square(error)))


def _table(what):
    """a 2-D table as the kernels take it: arrays, ``HArray``s and device tensors stay what they are, anything else becomes an array"""
    table = what if hasattr(what, "ndim") and hasattr(what, "shape") else np.asarray(what)
    if table.ndim != 2:
        raise ValueError("Only support 2-D ndarray.")
    return table, int(table.shape[0]), int(table.shape[1])


def fps_sample(n_sample, descriptors, start_idx=0, return_distance=False):
    """(n_sample,) int32 rows of ``descriptors`` by farthest-point sampling, the first one ``start_idx``; with ``return_distance``
    also the (N,) float64 distances of every row to the selected set"""
    table, n_points, _ = _table(descriptors)
    if n_sample > n_points:
        raise ValueError(f"n_sample must <= {n_points}.")
    if n_sample <= 0:
        raise ValueError("n_sample must be a positive number.")
    if start_idx < 0 or start_idx >= n_points:
        raise ValueError(f"start_idx must belong [0, {n_points - 1}].")
    picks = np.empty(int(n_sample), np.int32)
    squared = np.empty(n_points, np.float64) if return_distance else None
    kernels.sample.fps(table, int(n_sample), int(start_idx), picks, squared)
    return (picks, np.sqrt(squared)) if return_distance else picks


class PCA:
    """Principal components of a table: ``fit_transform`` projects the rows on the ``n_components`` directions of largest variance
    and leaves their variances in ``explained_variance`` and their shares of the total in ``explained_variance_ratio``."""

    def __init__(self, n_components):
        self.n_components = n_components
        self.explained_variance = None
        self.explained_variance_ratio = None

    def fit_transform(self, X):
        """(N, D) -> (N, min(n_components, D)) numpy"""
        table, n_rows, n_columns = _table(X)
        if n_rows < 2:
            raise ValueError(f"PCA needs at least two rows, got {n_rows}.")
        keep = min(int(self.n_components), n_columns)
        if keep < 1:
            raise ValueError("n_components must be a positive number.")
        if isinstance(table, np.ndarray) and have_gpu():  # two kernels read it: it goes up once
            table = HArray.from_numpy(np.ascontiguousarray(table, dtype=np.float64))
        mean, cov = np.empty(n_columns), np.empty((n_columns, n_columns))
        kernels.sample.moments(table, mean, cov)

        # eigh returns the eigenvalues in ascending order: read backwards they are sorted descending
        variance, vectors = np.linalg.eigh(cov)
        variance, vectors = variance[::-1], vectors[:, ::-1]
        self.explained_variance = variance[:keep].copy()
        self.explained_variance_ratio = variance[:keep] / variance.sum()
        # an eigenvector is defined up to its sign: the entry of largest magnitude is made positive
        components = np.array(vectors[:, :keep], order="C")
        largest = components[np.abs(components).argmax(axis=0), np.arange(keep)]
        components[:, largest < 0.0] *= -1.0

        out = np.empty((n_rows, keep))
        kernels.sample.project(table, mean, components, out)
        return out
