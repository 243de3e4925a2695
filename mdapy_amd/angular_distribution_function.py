"""Angular distribution function per element triplet — the drop-in for
``mdapy.angular_distribution_function.AngularDistributionFunction`` (src/mdapy/angular_distribution_function.py:92-168).

``rc_dict`` maps ``"A-B-C"`` (A the centre) to ``[rij_min, rij_max, rik_min, rik_max]``; each key is one row of
``bond_angle_distribution`` (npattern x nbin, int64), in dict order.  Element codes are the sorted distinct names."""
import numpy as np

from . import kernels, policy
from .bond_analysis import bin_centres, checked_bins
from .parallel import get_num_threads


def _pattern_table(rc_dict, names):
    """(npattern x 3 element codes, npattern x 4 ranges) of ``rc_dict``; rejects what the reference rejects"""
    code = {name: k for k, name in enumerate(names)}
    triples, ranges = [], []
    for key, bounds in rc_dict.items():
        parts = key.split("-")
        assert len(parts) == 3, f"pattern {key!r} must read 'A-B-C'."
        missing = [p for p in parts if p not in code]
        assert not missing, f"element(s) {missing} of {key!r} are not in the system."
        bounds = np.asarray(bounds, dtype=float).ravel()
        assert bounds.shape == (4,), "rc should be a list of 4 floats."
        triples.append([code[p] for p in parts])
        ranges.append(bounds)
    return np.array(triples, np.int32).reshape(-1, 3), np.array(ranges, float).reshape(-1, 4)


class AngularDistributionFunction:
    def __init__(self, data, box, rc_dict, nbin, verlet_list, distance_list, neighbor_number):
        assert "element" in data.columns, "Data must contain element column."
        self.data, self.box, self.nbin = data, box, nbin
        names, self._codes = policy.label_codes(data["element"].to_numpy())
        self.ele_unique = list(names)
        self.pair_list, self.rc_list = _pattern_table(rc_dict, self.ele_unique)
        self.verlet_list = verlet_list
        self.distance_list = distance_list
        self.neighbor_number = neighbor_number

    def compute(self):
        shells = checked_bins(self.nbin)
        counts = np.zeros((self.pair_list.shape[0], shells), np.int64)
        lists = (self.verlet_list, self.distance_list, self.neighbor_number)
        kernels.bond_analysis.compute_adf(*policy.positions(self.data), *policy.box_args(self.box), *lists, 180.0 / shells,
                                          self.rc_list, self.pair_list, np.ascontiguousarray(self._codes, dtype=np.int32), shells,
                                          counts, get_num_threads())
        self.bond_angle_distribution = counts
        self.r_angle = bin_centres(180.0, shells)
