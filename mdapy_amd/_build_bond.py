"""Drop-in for ``mdapy._build_bond`` (src/build_bond.cpp:10-94), and the two steps behind ``System.cal_chemical_species`` that the
reference takes in polars (src/mdapy/system.py:2680-2739).

``build_bond`` is the reference's function with one more trailing argument, ``n_real``, and with the ``np.unique`` of
``System.create_bonds`` already applied: the pairs come back in lexicographic order, each once.  Arrays may be numpy arrays,
``HArray``s or device tensors; results are numpy arrays for numpy input and HBM resident otherwise.  Every function waits for
the device: a count or a flag is read back."""
import ctypes

import numpy as np

from . import _lib
from .devarray import Call, HArray

f64, i32, i64 = np.float64, np.int32, np.int64


def _new(c, shape, dtype):
    return HArray.empty(shape, dtype) if c.space == _lib.DEVICE else np.empty(shape, dtype)


def build_bond(verlet_list, distance_list, neighbor_number, type_list, cutoff_matrix, num_t=1, n_real=0):
    """(Nbond, 2) int32: the pairs i < j of the list whose distance is at most ``cutoff_matrix[type_i, type_j]``, i ascending,
    j ascending inside a row.  ``type_list`` compact (0 .. ntype - 1) or None.  ``n_real`` > 0: the list was built on a replica of
    ``n_real`` atoms; the rows of the real atoms are read and a neighbour is named by the atom it copies (mdh_build_bond)."""
    if len(verlet_list.shape) != 2:
        raise ValueError(f"build_bond: verlet_list has shape {tuple(verlet_list.shape)}, expected (N, max_neigh)")
    N, M = int(verlet_list.shape[0]), int(verlet_list.shape[1])
    _lib.same_rows("build_bond", N, distance_list=distance_list, neighbor_number=neighbor_number, type_list=type_list)
    if tuple(distance_list.shape) != (N, M):
        raise ValueError(f"build_bond: distance_list has shape {tuple(distance_list.shape)}, verlet_list {(N, M)}")
    cut = np.ascontiguousarray(cutoff_matrix, dtype=f64)
    if cut.ndim != 2 or cut.shape[0] != cut.shape[1] or cut.shape[0] < 1:
        raise ValueError(f"build_bond: cutoff_matrix has shape {cut.shape}, expected (ntype, ntype)")
    ntype = int(cut.shape[0])
    c = Call(verlet_list, distance_list, neighbor_number, type_list)
    args = (c.inp(verlet_list, i32), c.inp(distance_list, f64), c.inp(neighbor_number, i32), N, M, c.inp(type_list, i32),
            cut.ctypes.data, ntype, int(n_real))
    found = ctypes.c_int64(0)
    rc_ = _lib.lib().mdh_build_bond(*args, None, 0, ctypes.addressof(found), c.space, c.stream)
    _lib.check(rc_)
    n = int(found.value)
    bond = _new(c, (n, 2), i32)
    if n:
        rc_ = _lib.lib().mdh_build_bond(*args, c.out(bond, i32, upload=False), n, ctypes.addressof(found), c.space, c.stream)
    c.done(rc_)
    return bond


def cluster_composition(cluster_id, type_list, cluster_number, ntype):
    """(cluster_number, ntype) int32: how many atoms of every compact type (0 .. ntype - 1) each cluster (ids 1 .. cluster_number)
    holds"""
    N = int(cluster_id.shape[0])
    _lib.same_rows("cluster_composition", N, type_list=type_list)
    c = Call(cluster_id, type_list)
    comp = _new(c, (int(cluster_number), int(ntype)), i32)
    rc_ = _lib.lib().mdh_cluster_composition(c.inp(cluster_id, i32), c.inp(type_list, i32), N, int(cluster_number), int(ntype),
                                             c.out(comp, i32, upload=False), c.space, c.stream)
    c.done(rc_)
    return comp


def species_match(composition, want, cluster_id=None):
    """(counts, mol_id): counts (nspecies) int64 = the rows of ``composition`` that equal each row of ``want`` (nspecies, ntype);
    with ``cluster_id`` (N), mol_id (N) int32 = the index of the species an atom's cluster equals (the last one where several
    do), -1 for none; None without"""
    want = np.ascontiguousarray(want, dtype=i32)
    n_cluster, ntype = int(composition.shape[0]), int(composition.shape[1])
    if want.ndim != 2 or want.shape[1] != ntype:
        raise ValueError(f"species_match: want has shape {want.shape}, expected (nspecies, {ntype})")
    c = Call(composition, cluster_id)
    N = 0 if cluster_id is None else int(cluster_id.shape[0])
    mol_id = None if cluster_id is None else _new(c, (N,), i32)
    counts = np.zeros(want.shape[0], i64)
    rc_ = _lib.lib().mdh_species_match(c.inp(composition, i32), n_cluster, ntype, want.ctypes.data, int(want.shape[0]),
                                       c.inp(cluster_id, i32), N, None if mol_id is None else c.out(mol_id, i32, upload=False),
                                       counts.ctypes.data, c.space, c.stream)
    c.done(rc_)
    return counts, mol_id
