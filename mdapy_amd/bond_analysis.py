"""Bond-length and bond-angle histograms — the drop-in for ``mdapy.bond_analysis.BondAnalysis``
(src/mdapy/bond_analysis.py:105-160) over a cutoff list.  Counts are int64 (the reference's int32 wraps past 2**31)."""
import numpy as np

from . import kernels, policy
from .parallel import get_num_threads


def bin_centres(span, nbin):
    """mid-points of nbin equal bins over [0, span] (linspace edges, as the reference's)"""
    edges = np.linspace(0.0, span, nbin + 1)
    return 0.5 * (edges[:-1] + edges[1:])


def checked_bins(nbin):
    count = int(nbin)
    if count < 1:
        raise ValueError(f"nbin must be at least 1, got {nbin}.")
    return count


class BondAnalysis:
    def __init__(self, data, box, rc, nbin, verlet_list, distance_list, neighbor_number):
        self.data, self.box = data, box
        self.rc, self.nbin = rc, nbin
        self.verlet_list = verlet_list
        self.distance_list = distance_list
        self.neighbor_number = neighbor_number

    def compute(self):
        """``bond_length_distribution`` (bonds j > i with r <= rc) and ``bond_angle_distribution`` (pairs of bonds of one centre,
        both r <= rc), ``r_length`` / ``r_angle`` their bin centres"""
        shells, reach = checked_bins(self.nbin), float(self.rc)
        if not reach > 0:
            raise ValueError(f"rc must be positive, got {self.rc}.")
        lengths, angles = (np.zeros(shells, np.int64) for _ in range(2))
        lists = (self.verlet_list, self.distance_list, self.neighbor_number)
        kernels.bond_analysis.compute_bond(*policy.positions(self.data), *policy.box_args(self.box), *lists, lengths, angles,
                                           reach / shells, 180.0 / shells, reach, shells, get_num_threads())
        self.bond_length_distribution, self.bond_angle_distribution = lengths, angles
        self.r_length, self.r_angle = bin_centres(reach, shells), bin_centres(180.0, shells)
