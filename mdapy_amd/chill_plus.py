"""CHILL+ water-phase identification — the drop-in for ``mdapy.chill_plus.ChillPlus`` (src/mdapy/chill_plus.py:14-103;
Nguyen & Molinero, J. Phys. Chem. B 119 (2015) 9369).  ``pattern`` (atoms) int32 over a cutoff list of the molecule centres
(oxygens or coarse-grained beads, no hydrogens):

    0 other (liquid)   1 hexagonal ice   2 cubic ice   3 interfacial ice   4 gas hydrate   5 interfacial gas hydrate

Two entries of a row are bonded when the listed distance is within ``cutoff``; a list built for a larger cutoff serves as it is.
Without the three list arguments ``compute`` builds a ``Neighbor`` at ``cutoff`` itself — on a replica where the box is thinner
than two cutoffs, and ``pattern`` then holds the atoms of ``data`` only.  The labels stay in HBM until somebody reads them."""
import numpy as np

from . import kernels, policy
from .devarray import HArray, as_numpy, empty
from .neighbor import Neighbor
from .parallel import get_num_threads


class ChillPlus:
    def __init__(self, data, box, cutoff=3.5, verlet_list=None, distance_list=None, neighbor_number=None):
        self.data, self.box = data, box
        self.cutoff = float(cutoff)
        self.verlet_list, self.distance_list, self.neighbor_number = verlet_list, distance_list, neighbor_number
        self.pattern = np.array([], dtype=np.int32)

    def compute(self):
        frame, cell = self.data, self.box
        if self.verlet_list is None or self.distance_list is None or self.neighbor_number is None:
            search = Neighbor(self.cutoff, self.box, self.data)
            search.compute()
            self.verlet_list, self.distance_list, self.neighbor_number = search.verlet_list, search.distance_list, search.neighbor_number
            if hasattr(search, "_enlarge_data"):  # (the rows index the replica)
                frame, cell = search._enlarge_data, search._enlarge_box
        atoms = frame.shape[0]
        pattern = empty(atoms, np.int32)
        lists = (self.verlet_list, self.distance_list, self.neighbor_number)
        kernels.chill_plus.compute_chill_plus(*policy.positions(frame), *policy.box_args(cell), *lists, self.cutoff, pattern,
                                              get_num_threads())
        n = self.data.shape[0]
        if atoms != n:
            pattern = pattern.head(n) if isinstance(pattern, HArray) else as_numpy(pattern)[:n]
        self.pattern = pattern
