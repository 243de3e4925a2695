"""Wigner-Seitz defect analysis — the drop-in for ``mdapy.wigner_seitz_defect.WignerSeitzAnalysis``
(src/mdapy/wigner_seitz_defect.py:11-131): every atom of a current frame is assigned to the nearest site of a reference frame;
a site nobody was assigned to is a vacancy, every atom beyond the first on a site an interstitial.

One object is one reference against many frames.  The reference sites are binned into a cell grid once (``_fast_knn.Tree``, at
construction; again only if the reference's position columns have been replaced since); a ``compute`` runs one nearest-site
query over the current frame — through the affine map when asked, in the kernel — and one occupancy pass, and reads two counts
back.  ``current`` need not have as many atoms as the reference.

Where the reference leaves the answer open: sites at exactly equal distance go to the lowest site index, and an atom without a
position (a non-finite coordinate) is assigned to no site — index -1, occupancy 0, site type ``""`` (element names) or 0."""
import numpy as np

from . import kernels, policy
from .devarray import HArray, as_numpy, empty, have_gpu
from .parallel import get_num_threads


def _site_types(frame, n_sites):
    """what a site is called: its element name, else its type, else 1"""
    for name in ("element", "type"):
        if name in frame.columns:
            return frame[name].to_numpy()
    return np.ones(n_sites, dtype=np.int64)


class WignerSeitzAnalysis:
    def __init__(self, ref, affine=False):
        self.ref, self.affine = ref, affine
        self.type_list = type_list = _site_types(ref.data, ref.N)
        # the site types as i32 codes for the gather: integer types are their own code, names are numbered in sorted order
        if type_list.dtype.kind in "iu" and (type_list.size == 0 or np.abs(type_list).max() < 2 ** 31):
            self._type_names, self._type_codes = None, np.ascontiguousarray(type_list, dtype=np.int32)
        else:
            self._type_names, codes = np.unique(type_list, return_inverse=True)
            self._type_codes = np.ascontiguousarray(codes.reshape(-1), dtype=np.int32)
        if have_gpu():
            self._type_codes = HArray.from_numpy(self._type_codes)  # (uploaded once: every compute gathers from them)
        self._built = None  # (the position columns the grid was made from, the tree)
        self._build_tree_from_ref()

    def _build_tree_from_ref(self):
        """the site grid of the reference's positions; rebuilt only when those columns are other objects than last time
        (``AtomicStrain``'s rule).  Only the columns are watched: a reference whose ``box`` is replaced while its position columns
        stay keeps the grid of the old box — make a new object for a new box."""
        cols = policy.positions(self.ref.data)
        held = self._built
        if held is None or any(a is not b for a, b in zip(held[0], cols)):
            tree = kernels.fast_knn.Tree()
            tree.build_with_coords(*cols, *policy.box_args(self.ref.box), get_num_threads())
            held = self._built = (cols, tree)
        self._tree = held[1]
        return self._tree

    def compute(self, current):
        """dict of ``site_occupancy`` (ref.N) i32, ``atom_site_index`` / ``atom_occupancy`` (current.N) i32, ``atom_site_type``
        (current.N; what ``type_list[atom_site_index]`` holds), ``vacancy_count`` and ``interstitial_count`` (ints).  The arrays
        are numpy arrays; those that were computed in HBM are read-only."""
        tree = self._build_tree_from_ref()
        affine_map = np.linalg.solve(current.box.box, self.ref.box.box) if self.affine else None
        n_atoms, n_sites = int(current.N), int(self.ref.N)
        index = empty(n_atoms, np.int32)
        tree.query_nearest_batch(*policy.positions(current.data), index, get_num_threads(), affine_map=affine_map)
        site_occ, atom_occ, atom_code = empty(n_sites, np.int32), empty(n_atoms, np.int32), empty(n_atoms, np.int32)
        vacancies, interstitials = kernels.fast_knn.cal_site_occupancy(index, self._type_codes, site_occ, atom_occ, atom_code)
        index, atom_code = as_numpy(index), as_numpy(atom_code)
        if self._type_names is None:
            site_type = np.where(index < 0, 0, atom_code).astype(self.type_list.dtype)
        else:
            site_type = np.where(index < 0, "", self._type_names[np.maximum(atom_code, 0)]) if n_sites else np.full(n_atoms, "")
        return {
            "site_occupancy": as_numpy(site_occ),
            "atom_site_index": index,
            "atom_site_type": site_type,
            "atom_occupancy": as_numpy(atom_occ),
            "vacancy_count": int(vacancies),
            "interstitial_count": int(interstitials),
        }
