"""Drop-in for ``mdapy._fast_knn`` (src/fast_knn.cpp:1024-1031): ``knn`` and ``Tree``; ``cal_site_occupancy`` is an extension."""
import numpy as np

from . import _lib
from .devarray import Call, HArray, have_gpu

f64, i32 = np.float64, np.int32
keeps_candidates = True  # knn(..., candidates=dict) (knn.py asks before passing it: the test backends have no such argument)


def knn(x, y, z, box, origin, boundary, k, indices, distances, num_t=1, key=None, candidates=None):
    """src/fast_knn.cpp:846.  Extensions: ``key`` (i64, N; a permutation of 0 .. N-1) orders exact ties in distance by key instead
    of by index (mdh_knn_keyed) — the rows of the system in the key's numbering, neighbour for neighbour.  ``candidates``: a dict the
    caller keeps with THESE positions in THIS box (frame.py: a Frame's columns never change) — the candidate rows of the search's
    cutoff build are left in it and the next search of the same positions, for whatever k, skips that build
    (mdh_knn_keyed_rows).  Same results with or without."""
    keep, (pb, po, pp) = _lib.host_box(box, origin, boundary)
    c = Call(x, y, z, indices, distances, key)
    L = _lib.lib()
    n = int(len(x))
    if candidates is None or c.space != _lib.DEVICE:
        rc_ = L.mdh_knn_keyed(c.inp(x, f64), c.inp(y, f64), c.inp(z, f64), n, pb, po, pp, int(k),
                              c.out(indices, i32, upload=False), c.out(distances, f64, upload=False), c.inp(key, np.int64),
                              c.space, c.stream)
        c.done(rc_)
        return
    import ctypes

    from .devarray import HArray

    sig = (pb, po, pp, n)  # (host_box memoises equal boxes: equal pointers mean equal bytes)
    have = candidates.get("rows")
    radius = ctypes.c_double(0.0)
    if have is not None and candidates.get("sig") == sig:
        rows, counts, radius.value = have
    else:
        width = int(L.mdh_knn_rows_width(int(k)))
        if width <= 0:
            rows = counts = None
        else:
            rows, counts = HArray.empty((n, width), i32), HArray.empty((n,), i32)
    if rows is None:
        rc_ = L.mdh_knn_keyed(c.inp(x, f64), c.inp(y, f64), c.inp(z, f64), n, pb, po, pp, int(k),
                              c.out(indices, i32, upload=False), c.out(distances, f64, upload=False), c.inp(key, np.int64),
                              c.space, c.stream)
        c.done(rc_)
        return
    rc_ = L.mdh_knn_keyed_rows(c.inp(x, f64), c.inp(y, f64), c.inp(z, f64), n, pb, po, pp, int(k),
                               c.out(indices, i32, upload=False), c.out(distances, f64, upload=False), c.inp(key, np.int64),
                               rows.dev().data_ptr(), counts.dev().data_ptr(), int(rows.shape[1]), ctypes.addressof(radius),
                               c.space, c.stream)
    c.done(rc_)
    candidates.clear()
    if radius.value > 0.0:
        candidates.update(sig=sig, rows=(rows, counts, float(radius.value)), keep=keep)


class Tree:
    """src/fast_knn.cpp:924-972 — the nearest of a set of reference sites for batches of query points (k = 1, periodic images as
    in ``knn``, the query never excluded: the Wigner-Seitz analysis).  ``build_with_coords`` bins the sites into a cell grid once;
    the object owns the grid's two buffers (``records``: the cell-sorted sites, 32 bytes each; ``cell_start``) and keeps them in HBM
    when there is a device, however the sites arrived; every ``query_nearest_batch`` hands them back to the library, which keeps
    no state of its own.  Exact ties in distance go to the lowest site index (the reference's answer there depends on its tree's
    traversal order); a query with a non-finite coordinate, or a tree of no sites, gives index -1.

    ``query_knn_batch`` — a per-stage benchmarking aid in the reference — is not provided."""

    def __init__(self):
        self.n_sites = None
        self.records = self.cell_start = None
        self._box = None

    def build_with_coords(self, x, y, z, box, origin, boundary, num_t=1):
        import ctypes

        n = int(len(x))
        _lib.same_rows("Tree.build_with_coords", n, y=y, z=z)
        keep, (pb, po, pp) = _lib.host_box(box, origin, boundary)
        L = _lib.lib()
        ncell = ctypes.c_int64(0)
        _lib.check(L.mdh_ws_grid_cells(n, pb, po, pp, ctypes.addressof(ncell)))
        if have_gpu():
            records, cell_start = HArray.empty((n, 4), f64), HArray.empty((ncell.value + 1,), i32)
        else:
            records, cell_start = np.empty((n, 4), f64), np.empty((ncell.value + 1,), i32)
        c = Call(x, y, z, records, cell_start)
        c.done(L.mdh_ws_build(c.inp(x, f64), c.inp(y, f64), c.inp(z, f64), n, pb, po, pp, c.out(records, f64, upload=False),
                              c.out(cell_start, i32, upload=False), c.space, c.stream))
        self.n_sites, self.records, self.cell_start, self._box = n, records, cell_start, (keep, pb, po, pp)

    def query_nearest_batch(self, qx, qy, qz, indices, num_t=1, affine_map=None):
        """``indices[i]`` = the site nearest to query i.  Extension: ``affine_map`` (3 x 3) maps every query first, in the kernel:
        x' = (x m[0, 0] + y m[1, 0]) + z m[2, 0], ..."""
        if self.n_sites is None:
            raise RuntimeError("Tree.query_nearest_batch: build_with_coords has not been called")
        nq = int(len(qx))
        _lib.same_rows("Tree.query_nearest_batch", nq, qy=qy, qz=qz, indices=indices)
        keep, pb, po, pp = self._box
        held = pm = None
        if affine_map is not None:
            held = np.ascontiguousarray(np.asarray(affine_map, dtype=f64).reshape(3, 3))
            pm = held.ctypes.data
        c = Call(qx, qy, qz, indices, self.records, self.cell_start)
        c.done(_lib.lib().mdh_ws_query(c.inp(self.records, f64), c.inp(self.cell_start, i32), self.n_sites, pb, po, pp,
                                       c.inp(qx, f64), c.inp(qy, f64), c.inp(qz, f64), nq, pm, c.out(indices, i32, upload=False),
                                       c.space, c.stream))


def cal_site_occupancy(indices, site_type, site_occupancy, atom_occupancy, atom_site_type):
    """Extension: what src/mdapy/wigner_seitz_defect.py:117-128 computes from the indices of ``query_nearest_batch``, on host or
    device arrays.  ``site_occupancy`` (one entry per site, i32) = atoms per site; ``atom_occupancy`` (per atom, i32) =
    ``site_occupancy[indices]``; ``atom_site_type`` = ``site_type[indices]`` (i32; both None: not wanted).  An index -1 is counted
    nowhere: occupancy 0, type -1.  Returns ``(vacancy_count, interstitial_count)`` = the number of sites with occupancy 0 and the
    sum of ``max(occupancy - 1, 0)``."""
    import ctypes

    nq, ns = int(len(indices)), int(len(site_occupancy))
    _lib.same_rows("cal_site_occupancy", nq, atom_occupancy=atom_occupancy, atom_site_type=atom_site_type)
    _lib.same_rows("cal_site_occupancy", ns, site_type=site_type)
    if (site_type is None) != (atom_site_type is None):
        raise ValueError("cal_site_occupancy: site_type and atom_site_type go together")
    counts = (ctypes.c_int * 2)()
    c = Call(indices, site_type, site_occupancy, atom_occupancy, atom_site_type)
    typed = site_type is not None
    c.done(_lib.lib().mdh_ws_occupancy(c.inp(indices, i32), nq, ns, c.inp(site_type, i32), c.out(site_occupancy, i32, upload=False),
                                       c.out(atom_occupancy, i32, upload=False),
                                       c.out(atom_site_type, i32, upload=False) if typed else None, ctypes.addressof(counts),
                                       c.space, c.stream))
    return int(counts[0]), int(counts[1])
