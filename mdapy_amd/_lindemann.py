"""Drop-in for ``mdapy._lindemann`` (src/lindemann.cpp:149-153).

``compute_global`` and ``compute_all`` have the reference's names and argument order.  Extensions: either pair table may be
``None`` — the kernels keep the pair state in registers and store nothing N x N then — and ``compute_all`` takes ``segments``
(how many workgroups share the j atoms of one block of i atoms; ``None``: the library chooses).  ``pos_list`` and the outputs
may be numpy arrays, ``HArray``s or device tensors."""
import ctypes

import numpy as np

from . import _lib
from .devarray import Call

f64 = np.float64


def _dims(what, pos_list):
    shape = tuple(int(n) for n in pos_list.shape)
    if len(shape) != 3 or shape[2] != 3:
        raise ValueError(f"{what}: pos_list has shape {shape}, expected (frames, atoms, 3)")
    return shape[0], shape[1]


def _table(what, name, table, n_atoms):
    if table is not None and tuple(table.shape) != (n_atoms, n_atoms):
        raise ValueError(f"{what}: {name} has shape {tuple(table.shape)}, expected {(n_atoms, n_atoms)}")


def compute_global(pos_list, pos_mean, pos_variance, num_t=1):
    """src/lindemann.cpp:20 -> the global index (float).  The strict upper triangle of ``pos_mean`` / ``pos_variance`` receives
    the pairs' sums of r and of r * r, as the reference leaves them; the rest is not touched."""
    F, N = _dims("compute_global", pos_list)
    _table("compute_global", "pos_mean", pos_mean, N)
    _table("compute_global", "pos_variance", pos_variance, N)
    result = ctypes.c_double(0.0)
    c = Call(pos_list, pos_mean, pos_variance)
    rc_ = _lib.lib().mdh_lindemann_global(c.inp(pos_list, f64), F, N, None if pos_mean is None else c.out(pos_mean, f64),
                                          None if pos_variance is None else c.out(pos_variance, f64), ctypes.addressof(result),
                                          c.space, c.stream)
    c.done(rc_)
    return float(result.value)


def compute_all(pos_list, pos_mean, pos_variance, lindemann_frame, lindemann_atom, segments=None):
    """src/lindemann.cpp:85 — ``lindemann_frame`` (F) and ``lindemann_atom`` (F, N) are written whole; ``pos_mean`` /
    ``pos_variance`` (both or neither) receive the pairs' Welford state after the last frame"""
    F, N = _dims("compute_all", pos_list)
    _table("compute_all", "pos_mean", pos_mean, N)
    _table("compute_all", "pos_variance", pos_variance, N)
    if tuple(lindemann_frame.shape) != (F,) or tuple(lindemann_atom.shape) != (F, N):
        raise ValueError(f"compute_all: lindemann_frame {tuple(lindemann_frame.shape)} and lindemann_atom "
                         f"{tuple(lindemann_atom.shape)} do not fit {F} frames of {N} atoms")
    c = Call(pos_list, pos_mean, pos_variance, lindemann_frame, lindemann_atom)
    rc_ = _lib.lib().mdh_lindemann_all(c.inp(pos_list, f64), F, N,
                                       None if pos_mean is None else c.out(pos_mean, f64, upload=False),
                                       None if pos_variance is None else c.out(pos_variance, f64, upload=False),
                                       c.out(lindemann_frame, f64, upload=False), c.out(lindemann_atom, f64, upload=False),
                                       0 if segments is None else int(segments), c.space, c.stream)
    c.done(rc_)
