"""The shim of csrc/sample.hip: farthest-point sampling and the device halves of a PCA (``potential_tool.py`` is the public side).

The reference has no compiled module for these (src/mdapy/potential_tool.py:354-445 is numpy), so the names are the library's
own.  Tables may be numpy arrays, ``HArray``s or device tensors of any float type and stride — they are taken as C-contiguous
float64; the outputs are numpy arrays (or ``HArray``s) of exactly the shapes given below, checked before any device work."""
import ctypes

import numpy as np

from . import _lib
from .devarray import Call

f64 = np.float64

PATHS = {None: 0, "grid": 1, "block": 2}
# what the one-workgroup path accepts (csrc/sample.hip FPS_BLOCK_MAX_D, FPS_BLOCK_MAX_ELEMS)
BLOCK_MAX_COLUMNS = 512
BLOCK_MAX_ENTRIES = 1 << 20


def _table(what, name, x):
    shape = tuple(int(n) for n in x.shape)
    if len(shape) != 2:
        raise ValueError(f"{what}: {name} has shape {shape}, expected two dimensions")
    return shape


def _fits(what, name, a, shape):
    if tuple(int(n) for n in a.shape) != tuple(shape):
        raise ValueError(f"{what}: {name} has shape {tuple(a.shape)}, expected {tuple(shape)}")


def block_path_takes(n_rows, n_columns):
    return n_columns <= BLOCK_MAX_COLUMNS and n_rows * n_columns <= BLOCK_MAX_ENTRIES


def fps(descriptors, n_sample, start_idx, picks, min_d2=None, _path=None):
    """``picks`` (n_sample,) int32 numpy <- the rows chosen by farthest-point sampling from ``start_idx``; ``min_d2`` (N,) float64
    (optional) <- every row's minimum SQUARED distance to the picks but the last.  ``_path``: "grid" or "block" forces one of the
    two kernels (they give the same bits), None lets the library choose.  Returns the path taken.  ValueError for a table with a
    value that is not finite."""
    N, D = _table("fps", "descriptors", descriptors)
    n_sample, start_idx = int(n_sample), int(start_idx)
    if not isinstance(picks, np.ndarray) or picks.dtype != np.int32 or not picks.flags.c_contiguous:
        raise TypeError("fps: picks must be a C-contiguous numpy array of int32")
    _fits("fps", "picks", picks, (n_sample,))
    if min_d2 is not None:
        _fits("fps", "min_d2", min_d2, (N,))
    if not 1 <= n_sample <= N:
        raise ValueError(f"fps: n_sample {n_sample} is outside 1 .. {N}")
    if not 0 <= start_idx < N:
        raise ValueError(f"fps: start_idx {start_idx} is outside 0 .. {N - 1}")
    if _path not in PATHS:
        raise ValueError(f"fps: _path must be one of 'grid', 'block', None, got {_path!r}")
    taken = ctypes.c_int(0)
    c = Call(descriptors, min_d2)
    rc_ = _lib.lib().mdh_fps_sample(c.inp(descriptors, f64), N, D, n_sample, start_idx, PATHS[_path], picks.ctypes.data,
                                    None if min_d2 is None else c.out(min_d2, f64, upload=False), ctypes.addressof(taken), c.space,
                                    c.stream)
    c.done(rc_)
    return {1: "grid", 2: "block"}[int(taken.value)]


def moments(X, mean, cov):
    """``mean`` (D,) <- the column means of ``X`` (N, D); ``cov`` (D, D) <- the covariance of the centred table, divisor N - 1"""
    N, D = _table("moments", "X", X)
    _fits("moments", "mean", mean, (D,))
    _fits("moments", "cov", cov, (D, D))
    if N < 2:
        raise ValueError(f"moments: needs at least two rows, got {N}")
    c = Call(X, mean, cov)
    rc_ = _lib.lib().mdh_pca_moments(c.inp(X, f64), N, D, c.out(mean, f64, upload=False), c.out(cov, f64, upload=False), c.space, c.stream)
    c.done(rc_)


def project(X, mean, components, out):
    """``out`` (N, C) <- (``X`` - ``mean``) @ ``components`` (D, C), each entry summed over the columns in order"""
    N, D = _table("project", "X", X)
    C = _table("project", "components", components)[1]
    _fits("project", "mean", mean, (D,))
    _fits("project", "components", components, (D, C))
    _fits("project", "out", out, (N, C))
    c = Call(X, mean, components, out)
    rc_ = _lib.lib().mdh_pca_project(c.inp(X, f64), N, D, c.inp(mean, f64), c.inp(components, f64), C, c.out(out, f64, upload=False),
                                     c.space, c.stream)
    c.done(rc_)
