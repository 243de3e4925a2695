"""Drop-in for ``mdapy._bond_analysis`` (src/bond_analysis.cpp:281-285).

Both functions ADD into the caller's histograms, int32 or int64, like the reference.  The library counts in u64; an int32
histogram that a count would carry past 2**31 - 1 raises ``OverflowError`` instead of wrapping as the reference's does."""
import numpy as np

from . import _lib
from .devarray import Call

f64, i32, i64 = np.float64, np.int32, np.int64


def _add_into(hist, counts, what):
    if not isinstance(hist, np.ndarray) or hist.dtype not in (np.dtype(i32), np.dtype(i64)) or not hist.flags.writeable:
        raise TypeError(f"{what}: the histogram must be a writable int32 or int64 numpy array")
    total = hist.astype(i64) + counts.reshape(hist.shape)
    if hist.dtype == np.dtype(i32) and (total > np.iinfo(i32).max).any():
        raise OverflowError(f"{what}: a count exceeds the int32 range of the histogram; pass an int64 array")
    hist[...] = total


def compute_bond(x, y, z, box, origin, boundary, verlet_list, distance_list, neighbor_number, bond_length_distribution,
                 bond_angle_distribution, delta_r, delta_theta, rc, nbins, num_t=1):
    """src/bond_analysis.cpp:8"""
    N, M = int(verlet_list.shape[0]), int(verlet_list.shape[1])
    _lib.same_rows("compute_bond", N, x=x, y=y, z=z, neighbor_number=neighbor_number)
    nbins = int(nbins)
    for name, h in (("bond_length_distribution", bond_length_distribution), ("bond_angle_distribution", bond_angle_distribution)):
        if np.asarray(h).size != nbins:
            raise ValueError(f"compute_bond: {name} has {np.asarray(h).size} bins, nbins is {nbins}")
    keep, (pb, po, pp) = _lib.host_box(box, origin, boundary)
    lengths, angles = np.zeros(nbins, i64), np.zeros(nbins, i64)
    c = Call(x, y, z, verlet_list, distance_list, neighbor_number, lengths, angles)
    rc_ = _lib.lib().mdh_bond_analysis(c.inp(x, f64), c.inp(y, f64), c.inp(z, f64), N, pb, po, pp, c.inp(verlet_list, i32),
                                       c.inp(distance_list, f64), c.inp(neighbor_number, i32), M, float(delta_r),
                                       float(delta_theta), float(rc), nbins, c.out(lengths, i64), c.out(angles, i64),
                                       c.space, c.stream)
    c.done(rc_)
    _add_into(bond_length_distribution, lengths, "compute_bond")
    _add_into(bond_angle_distribution, angles, "compute_bond")


def compute_adf(x, y, z, box, origin, boundary, verlet_list, distance_list, neighbor_number, delta_theta, rc_list, pair_list,
                type_list, nbins, bond_angle_distribution, num_t=1):
    """src/bond_analysis.cpp:139 — pair_list (Npair, 3) element codes (centre, j, k), rc_list (Npair, 4), type_list 0-based"""
    N, M = int(verlet_list.shape[0]), int(verlet_list.shape[1])
    _lib.same_rows("compute_adf", N, x=x, y=y, z=z, neighbor_number=neighbor_number, type_list=type_list)
    pairs = np.ascontiguousarray(np.asarray(pair_list, dtype=i32).reshape(-1, 3))
    ranges = np.ascontiguousarray(np.asarray(rc_list, dtype=f64).reshape(-1, 4))
    npair, nbins = int(pairs.shape[0]), int(nbins)
    if ranges.shape[0] != npair:
        raise ValueError(f"compute_adf: {ranges.shape[0]} ranges for {npair} patterns")
    if np.asarray(bond_angle_distribution).size != npair * nbins:
        raise ValueError(f"compute_adf: bond_angle_distribution must hold {npair} x {nbins} bins")
    keep, (pb, po, pp) = _lib.host_box(box, origin, boundary)
    counts = np.zeros(npair * nbins, i64)
    c = Call(x, y, z, verlet_list, distance_list, neighbor_number, type_list, counts)
    rc_ = _lib.lib().mdh_angular_distribution(c.inp(x, f64), c.inp(y, f64), c.inp(z, f64), N, pb, po, pp, c.inp(verlet_list, i32),
                                              c.inp(distance_list, f64), c.inp(neighbor_number, i32), c.inp(type_list, i32), M,
                                              float(delta_theta), pairs.ctypes.data, ranges.ctypes.data, npair, nbins,
                                              c.out(counts, i64), c.space, c.stream)
    c.done(rc_)
    _add_into(bond_angle_distribution, counts, "compute_adf")
