"""Drop-in for ``mdapy._strain`` (src/atomic_strain.cpp:219-221).

``cal_atomic_strain`` has the reference's name and argument order.  ``pack_records`` and ``cal_atomic_strain_records`` are
extensions: a frame's positions as one 32-byte record per atom, made once and handed to every later call — an ``AtomicStrain``
packs its reference frame when it is constructed and only the current frame with every ``compute``."""
import numpy as np

from . import _lib
from .devarray import Call, HArray

f64, i32 = np.float64, np.int32


def _map9(matrix):
    if matrix is None:
        return None, None
    m = np.ascontiguousarray(np.asarray(matrix, dtype=f64).reshape(3, 3))
    return m, m.ctypes.data


def _boxes(ref_box, cur_box, ref_origin, cur_origin, boundary):
    keep_r, (rb, ro, pp) = _lib.host_box(ref_box, ref_origin, boundary)
    keep_c, (cb, co, _) = _lib.host_box(cur_box, cur_origin, boundary)
    return (keep_r, keep_c), (rb, ro, cb, co, pp)


def cal_atomic_strain(verlet_list, neighbor_number, ref_box, cur_box, ref_origin, cur_origin, boundary, ref_x, ref_y, ref_z,
                      cur_x, cur_y, cur_z, shear_strain, volumetric_strain, num_t=1, affine_map=None):
    """src/atomic_strain.cpp:110 — ``affine_map`` (extension, 3 x 3): the current positions through it first, in the kernel"""
    N, M = int(verlet_list.shape[0]), int(verlet_list.shape[1])
    _lib.same_rows("cal_atomic_strain", N, neighbor_number=neighbor_number, ref_x=ref_x, ref_y=ref_y, ref_z=ref_z, cur_x=cur_x,
                   cur_y=cur_y, cur_z=cur_z, shear_strain=shear_strain, volumetric_strain=volumetric_strain)
    keep, (rb, ro, cb, co, pp) = _boxes(ref_box, cur_box, ref_origin, cur_origin, boundary)
    held, pm = _map9(affine_map)
    c = Call(verlet_list, neighbor_number, ref_x, ref_y, ref_z, cur_x, cur_y, cur_z, shear_strain, volumetric_strain)
    rc_ = _lib.lib().mdh_atomic_strain(c.inp(verlet_list, i32), c.inp(neighbor_number, i32), N, M, rb, ro, cb, co, pp,
                                       c.inp(ref_x, f64), c.inp(ref_y, f64), c.inp(ref_z, f64), c.inp(cur_x, f64), c.inp(cur_y, f64),
                                       c.inp(cur_z, f64), pm, c.out(shear_strain, f64, upload=False),
                                       c.out(volumetric_strain, f64, upload=False), c.space, c.stream)
    c.done(rc_)


def pack_records(x, y, z, affine_map=None):
    """-> (N, 4) f64 records (x, y, z, unused) of a frame, where the columns live: numpy for numpy columns, HBM otherwise"""
    N = int(len(x))
    _lib.same_rows("pack_records", N, y=y, z=z)
    on_dev = not all(isinstance(a, np.ndarray) for a in (x, y, z))
    records = HArray.empty((N, 4), f64) if on_dev else np.empty((N, 4), f64)
    held, pm = _map9(affine_map)
    c = Call(x, y, z, records)
    c.done(_lib.lib().mdh_strain_pack(c.inp(x, f64), c.inp(y, f64), c.inp(z, f64), N, pm, c.out(records, f64, upload=False),
                                      c.space, c.stream))
    return records


def cal_atomic_strain_records(verlet_list, neighbor_number, ref_box, cur_box, ref_origin, cur_origin, boundary, ref_records,
                              cur_records, shear_strain, volumetric_strain):
    """``cal_atomic_strain`` on two record buffers of ``pack_records``"""
    N, M = int(verlet_list.shape[0]), int(verlet_list.shape[1])
    _lib.same_rows("cal_atomic_strain_records", N, neighbor_number=neighbor_number, ref_records=ref_records, cur_records=cur_records,
                   shear_strain=shear_strain, volumetric_strain=volumetric_strain)
    for name, r in (("ref_records", ref_records), ("cur_records", cur_records)):
        if tuple(r.shape) != (N, 4):
            raise ValueError(f"cal_atomic_strain_records: {name} has shape {tuple(r.shape)}, expected {(N, 4)}")
    keep, (rb, ro, cb, co, pp) = _boxes(ref_box, cur_box, ref_origin, cur_origin, boundary)
    c = Call(verlet_list, neighbor_number, ref_records, cur_records, shear_strain, volumetric_strain)
    rc_ = _lib.lib().mdh_atomic_strain_records(c.inp(verlet_list, i32), c.inp(neighbor_number, i32), N, M, rb, ro, cb, co, pp,
                                               c.inp(ref_records, f64), c.inp(cur_records, f64),
                                               c.out(shear_strain, f64, upload=False), c.out(volumetric_strain, f64, upload=False),
                                               c.space, c.stream)
    c.done(rc_)
