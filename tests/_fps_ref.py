"""Plain-numpy restatements of farthest-point sampling and of the PCA, written from their definitions (mdapy_amd/potential_tool.py's
docstring): the yardsticks of test_potential_tool_host.py and test_gpu_potential_tool.py."""
import math

import numpy as np


def squared_distances(X, row):
    """the pinned sum: acc = acc + (a_k - b_k) * (a_k - b_k), k ascending, one accumulator per row, binary64 — numpy evaluates
    the difference, the product and the sum as three separately rounded operations"""
    acc = np.zeros(X.shape[0])
    for k in range(X.shape[1]):
        d = X[:, k] - X[row, k]
        acc = acc + d * d
    return acc


def fps_squared(n, X, start):
    """-> (picks int32 (n,), the squared minima after the n - 1 passes): the library's rule"""
    X = np.ascontiguousarray(X, dtype=np.float64)
    picks = np.empty(n, np.int32)
    picks[0] = start
    minima = np.full(X.shape[0], np.inf)
    for s in range(n - 1):
        minima = np.minimum(minima, squared_distances(X, picks[s]))
        picks[s + 1] = np.argmax(minima)  # the first of equal values
    return picks, minima


def fps_norm(n, X, start):
    """-> picks int32 (n,): the reference's rule — the minima are Euclidean norms, taken by np.linalg.norm"""
    X = np.ascontiguousarray(X, dtype=np.float64)
    chosen = [int(start)]
    nearest = np.full(X.shape[0], np.inf)
    while len(chosen) < n:
        nearest = np.minimum(nearest, np.linalg.norm(X - X[chosen[-1]], axis=1))
        chosen.append(int(np.argmax(nearest)))
    return np.array(chosen, np.int32)


def pca(X, k):
    """-> (projection (N, k'), explained variance, its ratio), k' = min(k, D): covariance with divisor N - 1, eigh, largest
    eigenvalue first, every component's entry of largest magnitude positive, projection of the centred rows"""
    X = np.asarray(X, dtype=np.float64)
    centred = X - X.mean(axis=0)
    cov = centred.T @ centred / (X.shape[0] - 1)
    w, v = np.linalg.eigh(cov)
    w, v = w[::-1], v[:, ::-1]
    k = min(k, X.shape[1])
    comp = v[:, :k].copy()
    for c in range(k):
        if comp[np.argmax(np.abs(comp[:, c])), c] < 0:
            comp[:, c] = -comp[:, c]
    return centred @ comp, w[:k], w[:k] / w.sum()


def exact_moments(X, mean):
    """The sums the device takes, added exactly (math.fsum) -> (means, sum |x| per column, covariance, sum |term| per entry).
    The covariance terms (x_a - mean_a) * (x_b - mean_b) are formed in binary64 from the ``mean`` given — the device's own — so
    that its centring error is not counted a second time."""
    X = np.asarray(X, dtype=np.float64)
    N, D = X.shape
    means = np.array([math.fsum(X[:, c]) / N for c in range(D)])
    mass = np.array([math.fsum(np.abs(X[:, c])) for c in range(D)])
    centred = X - np.asarray(mean)[None, :]
    cov, cov_mass = np.empty((D, D)), np.empty((D, D))
    for a in range(D):
        for b in range(D):
            terms = centred[:, a] * centred[:, b]
            cov[a, b] = math.fsum(terms) / (N - 1)
            cov_mass[a, b] = math.fsum(np.abs(terms))
    return means, mass, cov, cov_mass


def exact_projection(X, mean, components):
    """-> ((X - mean) @ components with every entry's D terms added exactly, sum |term| per entry)"""
    X = np.asarray(X, dtype=np.float64)
    centred = X - np.asarray(mean)[None, :]
    N, C = X.shape[0], components.shape[1]
    out, mass = np.empty((N, C)), np.empty((N, C))
    for c in range(C):
        terms = centred * components[None, :, c]
        for i in range(N):
            out[i, c] = math.fsum(terms[i])
        mass[:, c] = np.abs(terms).sum(axis=1)
    return out, mass


class Shim:
    """the restatement with the signatures of mdapy_amd/_sample.py: what the CPU tests install as ``kernels.sample``"""

    @staticmethod
    def fps(descriptors, n_sample, start_idx, picks, min_d2=None, _path=None):
        got, minima = fps_squared(n_sample, np.asarray(descriptors), start_idx)
        picks[...] = got
        if min_d2 is not None:
            min_d2[...] = minima
        return "grid"

    @staticmethod
    def moments(X, mean, cov):
        X = np.asarray(X, dtype=np.float64)
        mean[...] = X.mean(axis=0)
        centred = X - mean
        cov[...] = centred.T @ centred / (X.shape[0] - 1)

    @staticmethod
    def project(X, mean, components, out):
        out[...] = (np.asarray(X, dtype=np.float64) - mean) @ components
