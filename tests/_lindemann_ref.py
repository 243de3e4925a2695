"""The Lindemann index in numpy, restated from reading the reference (src/lindemann.cpp:20-146): the yardstick of
test_gpu_lindemann.py and the stand-in for ``kernels.lindemann`` in test_lindemann_host.py.

Every per-pair quantity — the distance, the running sums of the global mode, the Welford mean and variance of the full mode, the
pair's term — is computed by the reference's elementwise operations in its order, vectorised over the pairs and looped over the
frames, so it carries the reference's bits (numpy's ``+ - * /`` and ``sqrt`` on float64 are IEEE, and nothing is fused).  The SUMS
of terms are taken with ``math.fsum``, which rounds the exact sum once: the yardstick favours no order of summation.  The divisor
is applied to the sum (the reference divides every term of an atom's sum by N - 1)."""
import math
from types import SimpleNamespace

import numpy as np


def _distances(frame):
    """r[i, j] of one frame: dx = pos[i] - pos[j], sqrt(dx*dx + dy*dy + dz*dz) left to right (:42-45, :107-110).  (j, i) holds the
    bits of (i, j): a difference changes sign exactly and is squared."""
    d = frame[:, None, :] - frame[None, :, :]
    dx, dy, dz = d[..., 0], d[..., 1], d[..., 2]
    return np.sqrt(dx * dx + dy * dy + dz * dz)


def restate(pos_list):
    """everything about a trajectory (F, N, 3): ``frame`` (F), ``atom`` (F, N), ``trj`` (the global mode's value), the four
    N x N tables ``mean`` / ``var`` (full mode, symmetric, after the last frame) and ``sum`` / ``sumsq`` (global mode; only the
    strict upper triangle means anything), and the pair masks ``var_positive`` (F, N, N: which ordered pairs have a term in each
    frame) and ``delta_positive`` (N, N, upper triangle: which pairs have a term in the global mode), with ``delta`` itself"""
    pos = np.ascontiguousarray(pos_list, dtype=np.float64)
    F, N = pos.shape[:2]
    off = ~np.eye(N, dtype=bool)
    upper = np.triu(np.ones((N, N), dtype=bool), 1)
    mean, var = np.zeros((N, N)), np.zeros((N, N))
    s1, s2 = np.zeros((N, N)), np.zeros((N, N))
    frame, atom = np.zeros(F), np.zeros((F, N))
    var_positive = np.zeros((F, N, N), dtype=bool)
    with np.errstate(invalid="ignore", divide="ignore"):
        for f in range(F):
            r = _distances(pos[f])
            n = float(f + 1)
            delta = r - mean  # :113-118
            mean = mean + delta / n
            var = var + delta * (r - mean)
            s1 = s1 + r  # :47-48
            s2 = s2 + r * r
            on = off & (var > 0)  # :133
            var_positive[f] = on
            term = np.where(on, np.sqrt(var / n) / mean, 0.0)
            rows = [math.fsum(row) for row in term]
            atom[f] = np.array(rows) / float(N - 1)
            frame[f] = math.fsum(term.ravel()) / float(N * (N - 1))
        sq_mean, r_mean = s2 / float(F), s1 / float(F)  # :63-69
        delta = sq_mean - r_mean * r_mean
        delta_positive = upper & (delta > 0)
        term = np.where(delta_positive, np.sqrt(delta) / r_mean, 0.0)
    trj = math.fsum(term.ravel()) / (float(N * (N - 1)) / 2.0)
    return SimpleNamespace(frame=frame, atom=atom, trj=trj, mean=mean, var=var, sum=np.where(upper, s1, 0.0),
                           sumsq=np.where(upper, s2, 0.0), var_positive=var_positive, delta_positive=delta_positive,
                           delta=np.where(upper, delta, 0.0), upper=upper)


# ---- the two functions of mdapy._lindemann, with the shim's extensions (a table may be None; segments is ignored)
def compute_global(pos_list, pos_mean, pos_variance, num_t=1):
    got = restate(np.asarray(pos_list))
    if pos_mean is not None:
        pos_mean[got.upper] = got.sum[got.upper]
    if pos_variance is not None:
        pos_variance[got.upper] = got.sumsq[got.upper]
    return float(got.trj)


def compute_all(pos_list, pos_mean, pos_variance, lindemann_frame, lindemann_atom, segments=None):
    got = restate(np.asarray(pos_list))
    if pos_mean is not None:
        pos_mean[...] = got.mean
    if pos_variance is not None:
        pos_variance[...] = got.var
    lindemann_frame[...] = got.frame
    lindemann_atom[...] = got.atom
