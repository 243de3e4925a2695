"""The mean squared displacement in numpy, restated from its definition: the yardstick of test_gpu_msd.py and the stand-in for
``kernels.msd`` in test_msd_host.py.

A term is ``(dx*dx + dy*dy) + dz*dz`` with ``dx = a.x - b.x`` ... in that order (numpy's ``- * +`` on float64 are IEEE and nothing
is fused), so it carries the device's bits.  Every SUM — over the time origins of a window entry, over the atoms of an ``msd``
entry — is taken with ``math.fsum``, which rounds the exact sum once, and is then divided once: the yardstick favours no order of
summation."""
import math
from types import SimpleNamespace

import numpy as np


def _terms(a, b):
    """term(a, b) for arrays of positions (..., 3)"""
    d = a - b
    dx, dy, dz = d[..., 0], d[..., 1], d[..., 2]
    return (dx * dx + dy * dy) + dz * dz


def _rows_mean(table):
    """msd[m] = fsum(table[m]) / N"""
    return np.array([math.fsum(row) / float(table.shape[1]) for row in table])


def window_table(pos, lags):
    """particle_msd of the window mode for the lags 0 .. lags - 1"""
    F, N = pos.shape[:2]
    out = np.zeros((lags, N))
    for m in range(lags):
        terms = _terms(pos[m:], pos[:F - m])  # (F - m, N)
        out[m] = np.array([math.fsum(terms[:, i]) for i in range(N)]) / float(F - m)
    return out


def direct_table(pos):
    return _terms(pos, pos[:1])


def restate(pos_list):
    """``window`` / ``direct``: particle_msd (F, N) of the two modes; ``window_msd`` / ``direct_msd``: msd (F)"""
    pos = np.ascontiguousarray(pos_list, dtype=np.float64)
    w, d = window_table(pos, pos.shape[0]), direct_table(pos)
    return SimpleNamespace(window=w, direct=d, window_msd=_rows_mean(w), direct_msd=_rows_mean(d))


def fft_window(pos_list):
    """the windowed particle_msd by the formula of the reference's docstring, MSD(m) = S1(m) - 2 S2(m) with
    S1(m) = 1/(F-m) sum_{t<F-m} [r^2(t) + r^2(t+m)] and S2(m) = 1/(F-m) sum_{t<F-m} r(t) . r(t+m), in numpy doubles: S1 from a
    running total of r^2 (the first F-m squares plus the last F-m), S2 as the autocorrelation of each coordinate — the inverse real
    transform of its power spectrum, the series padded with zeros to 2 F so that the circular sum does not wrap.  Not a result to
    use (it cancels): the host test bounds its distance from the restatement, tools/msd_bench.py times it."""
    pos = np.asarray(pos_list, dtype=np.float64)
    F = pos.shape[0]
    count = (F - np.arange(F))[:, None].astype(np.float64)  # time origins of lag m
    upto = np.concatenate([np.zeros((1,) + pos.shape[1:2]), np.cumsum(np.einsum("tic,tic->ti", pos, pos), axis=0)])  # upto[k] = sum_{t<k} r^2(t)
    heads, tails = upto[F - np.arange(F)], upto[F] - upto[np.arange(F)]
    power = np.abs(np.fft.rfft(pos, n=2 * F, axis=0)) ** 2
    dots = np.fft.irfft(power, n=2 * F, axis=0)[:F].sum(axis=2)  # sum_t r(t) . r(t+m)
    return (heads + tails) / count - 2.0 * (dots / count)


# ---- the two functions of mdapy_amd._msd
def _fill(table, particle_msd, msd):
    if particle_msd is None and msd is None:
        raise ValueError("particle_msd and msd are both None")
    if particle_msd is not None:
        particle_msd[...] = table
    if msd is not None:
        msd[...] = _rows_mean(table)


def window(pos_list, particle_msd, msd):
    pos = np.ascontiguousarray(np.asarray(pos_list), dtype=np.float64)
    given = particle_msd if particle_msd is not None else msd
    _fill(window_table(pos, pos.shape[0] if given is None else int(given.shape[0])), particle_msd, msd)


def direct(pos_list, particle_msd, msd):
    _fill(direct_table(np.ascontiguousarray(np.asarray(pos_list), dtype=np.float64)), particle_msd, msd)
