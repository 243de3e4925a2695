"""Drop-in for ``mdapy._chill_plus`` (src/chill_plus.cpp:181-184)."""
import numpy as np

from . import _lib
from .devarray import Call

f64, i32 = np.float64, np.int32


def compute_chill_plus(x, y, z, box, origin, boundary, verlet_list, distance_list, neighbor_number, rc, pattern, num_t=1):
    """src/chill_plus.cpp:76"""
    _lib.same_rows("compute_chill_plus", len(x), y=y, z=z, verlet_list=verlet_list, distance_list=distance_list,
                   neighbor_number=neighbor_number, pattern=pattern)
    if tuple(distance_list.shape) != tuple(verlet_list.shape):
        raise ValueError(f"compute_chill_plus: distance_list has shape {tuple(distance_list.shape)}, verlet_list {tuple(verlet_list.shape)}")
    keep, (pb, po, pp) = _lib.host_box(box, origin, boundary)
    c = Call(x, y, z, verlet_list, distance_list, neighbor_number, pattern)
    N, M = int(verlet_list.shape[0]), int(verlet_list.shape[1])
    rc_ = _lib.lib().mdh_chill_plus(c.inp(x, f64), c.inp(y, f64), c.inp(z, f64), N, pb, po, pp, c.inp(verlet_list, i32),
                                    c.inp(distance_list, f64), c.inp(neighbor_number, i32), M, float(rc),
                                    c.out(pattern, i32, upload=False), c.space, c.stream)
    c.done(rc_)
