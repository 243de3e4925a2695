"""The void analysis' door to the library, behind ``_neighbor._fill_cell_for_void``: the two steps the reference takes in numpy and
polars (src/mdapy/void_analysis.py:75-106), so this module's name and signatures are this project's own, not a drop-in.

``void_points`` turns the occupancy grid into the ordered list of void points; ``prune`` drops the points whose cluster has no
second point and renumbers the clusters that stay.  Arrays may be numpy arrays, ``HArray``s or device tensors; results are numpy
arrays for numpy input and HBM resident otherwise.  Both wait for the device: the lengths of their results are read back."""
import ctypes

import numpy as np

from . import _lib
from .devarray import Call, HArray

f64, i32 = np.float64, np.int32


def _new(c, n, dtype):
    return HArray.empty((n,), dtype) if c.space == _lib.DEVICE else np.empty(n, dtype)


def void_points(cell_id_list, box, origin, with_index=False):
    """(x, y, z) — with ``with_index`` (x, y, z, flat cell index, int32) — of the empty cells (== 0) of ``cell_id_list``
    (ncell0, ncell1, ncell2) int32 in ``np.argwhere`` order: ``((index + 0.5) / ncell) @ box + origin``, evaluated as
    ((f0 * box[0, e] + f1 * box[1, e]) + f2 * box[2, e]) + origin[e]."""
    shape = tuple(int(n) for n in cell_id_list.shape)
    if len(shape) != 3 or min(shape) < 1:
        raise ValueError(f"void_points: cell_id_list has shape {shape}, expected (ncell0, ncell1, ncell2)")
    keep, (pb, po, pp) = _lib.host_box(box, origin, np.zeros(3, i32))
    c = Call(cell_id_list)
    grid = c.inp(cell_id_list, i32)
    found = ctypes.c_int64(0)
    rc_ = _lib.lib().mdh_void_points(grid, *shape, pb, po, None, None, None, None, 0, ctypes.addressof(found), c.space, c.stream)
    _lib.check(rc_)
    n = int(found.value)
    out = [_new(c, n, f64) for _ in range(3)] + ([_new(c, n, i32)] if with_index else [])
    if n:
        rc_ = _lib.lib().mdh_void_points(grid, *shape, pb, po, *(c.out(a, f64, upload=False) for a in out[:3]),
                                         c.out(out[3], i32, upload=False) if with_index else None, n, ctypes.addressof(found),
                                         c.space, c.stream)
    c.done(rc_)
    return tuple(out)


def prune(x, y, z, cluster_id, cluster_number):
    """(x, y, z, cluster_id, void_number): the points of the clusters of more than one point, in the order they had, the clusters
    that stay renumbered 1 .. void_number in ascending old id (int32)"""
    m = int(len(x))
    _lib.same_rows("prune", m, y=y, z=z, cluster_id=cluster_id)
    c = Call(x, y, z, cluster_id)
    out = [_new(c, m, f64) for _ in range(3)] + [_new(c, m, i32)]
    kept, voids = ctypes.c_int64(0), ctypes.c_int(0)
    rc_ = _lib.lib().mdh_void_prune(c.inp(x, f64), c.inp(y, f64), c.inp(z, f64), c.inp(cluster_id, i32), m, int(cluster_number),
                                    *(c.out(a, f64, upload=False) for a in out[:3]), c.out(out[3], i32, upload=False),
                                    ctypes.addressof(kept), ctypes.addressof(voids), c.space, c.stream)
    c.done(rc_)
    k = int(kept.value)
    return (*(a.head(k) if isinstance(a, HArray) else a[:k].copy() for a in out), int(voids.value))
