"""Per-atom shear and volumetric strain of a current frame against a reference frame — the drop-in for
``mdapy.atomic_strain.AtomicStrain`` (src/mdapy/atomic_strain.py:129-242): the deformation gradient of every atom's
neighbourhood from the bonds of the REFERENCE frame's cutoff list, measured in both frames (Shimizu, Ogata, Li 2007).

One object is one reference against many frames.  The reference positions are packed into 32-byte records once (the first
``compute``, and again only if the reference's list or positions have been replaced since); a ``compute`` packs the current
frame — through the affine map when asked, in the same kernel — and runs one gather over the rows.  The results stay in HBM
until somebody reads them.

Two things the reference leaves open:

* **a reference box thinner than two cutoffs.**  The reference replicates ``current`` and then looks for its own replica of
  ``ref`` under a name that never exists, so its shape assertion fails.  Here the strain is computed on the replica the
  reference frame's list indexes (``ref._get_compute_view()``), with ``current`` replicated by the same counts
  (``self.repeat``); the first ``N`` rows are stored.
* **an atom without neighbours** gets what the formulas give: shear 0, volumetric -0.5.

When ``ref`` is large and was handed in in no spatial order its list was built on the cell-sorted twin (_twin.py).  The
kernel then runs on the twin's rows and positions, ``current`` is read through the twin's permutation, and the two result
columns are scattered back: the N x M rows are never translated, and no gather goes through a shuffled numbering.  A row lists
the same atoms in the same order either way, so the sums are the same bit for bit."""
import numpy as np

from . import kernels, policy
from . import tool_function as tool
from .box import Box
from .devarray import as_numpy, empty
from .parallel import get_num_threads


def _through(perm, cols):
    """the three columns read through a permutation"""
    order = kernels.order
    if hasattr(order, "gather_positions") and not isinstance(perm, np.ndarray):
        return order.gather_positions(*(c.device_array() for c in cols), perm)
    return tuple(order.permute(c.device_array() if not isinstance(perm, np.ndarray) else c.to_numpy(), perm) for c in cols)


class AtomicStrain:
    def __init__(self, rc, ref, affine=False, max_neigh=None):
        self.ref = ref
        self.rc = rc
        self.max_neigh = max_neigh
        self.ref.build_neighbor(self.rc, self.max_neigh)
        self.affine = affine
        self.repeat = self.ref.box.check_small_box(self.rc)
        self._packed = None  # (the objects the records were made from, the records)

    def _reference(self):
        """(rows, counts, box, position columns, permutation or None) the strain is computed over"""
        ref = self.ref
        twin = ref._listed_on_twin()
        if twin is not None:  # the list lives on the cell-sorted twin; ref.verlet_list is its untranslated mirror
            return twin.verlet_list, twin.neighbor_number, ref.box, policy.positions(twin.data), twin._perm
        cell, frame = ref._get_compute_view()
        return ref.verlet_list, ref.neighbor_number, cell, policy.positions(frame), None

    def _reference_records(self, rows, cols):
        key = (rows, *cols)
        held = self._packed
        if held is None or len(held[0]) != len(key) or any(a is not b for a, b in zip(held[0], key)):
            held = self._packed = (key, kernels.strain.pack_records(*cols))
        return held[1]

    def compute(self, current):
        """columns ``shear_strain`` and ``volumetric_strain`` of ``current`` (which must have as many atoms as the reference)"""
        assert current.N == self.ref.N
        rows, counts, ref_box, ref_cols, perm = self._reference()
        cur_data, cur_box = current.data, current.box
        if hasattr(self.ref, "_enlarge_data") and perm is None and not policy.is_single(self.repeat):
            cur_data, cur_box = tool._replicate_pos(current.data, current.box, *self.repeat)
        cur_cols = policy.positions(cur_data)
        atoms = int(rows.shape[0])
        assert len(cur_cols[0]) == len(ref_cols[0]) == atoms
        if perm is not None:
            cur_cols = _through(perm, cur_cols)
        affine_map = None
        if self.affine:
            affine_map = np.linalg.solve(cur_box.box, ref_box.box)
            cur_box = Box(ref_box)
        shear, volumetric = empty(atoms, np.float64), empty(atoms, np.float64)
        boxes = (ref_box.box, cur_box.box, ref_box.origin, cur_box.origin, ref_box.boundary)
        if hasattr(kernels.strain, "pack_records"):
            ref_records = self._reference_records(rows, ref_cols)
            cur_records = kernels.strain.pack_records(*cur_cols, affine_map)
            kernels.strain.cal_atomic_strain_records(rows, counts, *boxes, ref_records, cur_records, shear, volumetric)
        else:  # (a backend with the reference's one function only: the map on the host, in the reference's expression)
            if affine_map is not None:
                x, y, z = (as_numpy(c) for c in cur_cols)
                m = affine_map
                cur_cols = tuple(x * m[0, k] + y * m[1, k] + z * m[2, k] for k in range(3))
            kernels.strain.cal_atomic_strain(rows, counts, *boxes, *ref_cols, *cur_cols, shear, volumetric, get_num_threads())
        if perm is not None:
            shear, volumetric = (kernels.order.permute(a, perm, scatter=True) for a in (shear, volumetric))
        current._store(shear_strain=shear, volumetric_strain=volumetric)
