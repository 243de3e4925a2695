"""Void analysis — the drop-in for ``mdapy.void_analysis.VoidAnalysis`` (src/mdapy/void_analysis.py:12-112): the empty cells of
a grid of ``rc``-wide cells, clustered into voids.

``compute()`` sets ``void_number``, ``void_volume`` and ``void_system``, as the reference does, quirks included:

* the grid is the cutoff neighbour build's — ``max(floor(thickness / rc), 3)`` cells of width ``rc`` from the origin, the last one
  taking the remainder — but a void point is the centre of one of that many EQUAL cells, ``((index + 0.5) / ncell) @ box +
  origin``; on an axis thinner than ``3 rc`` the grid still has three cells — the third takes what is left behind ``2 rc``, and
  on an axis thinner than ``2 rc`` no atom inside the box reaches it: its whole layer comes out empty;
* the points are clustered with ``cal_cluster_analysis(rc * 1.1)`` in the system's own box, clusters of a single point are
  dropped, the rest renumbered 1 .. k in ascending old id, the points keep their order and get ``element = "X"``;
* ``void_volume`` is (points kept) x ``rc**3`` — not the volume of the cells;
* with no empty cell, or only single ones, ``void_number = 0``, ``void_volume = 0.0`` and ``void_system`` stays ``None``.

Everything runs in HBM: the occupancy grid, the ordered list of points and the pruning are kernels of csrc/voids.hip, the
clustering the neighbour build and ``_cluster`` as for any system; only the lengths of the lists come back to the host.  The input
system is not touched: its positions are wrapped on the fly, it gains no neighbour list and no column."""
import numpy as np

from . import kernels, policy
from .parallel import get_num_threads


class VoidAnalysis:
    def __init__(self, system, rc):
        self.system = system
        self.rc = rc
        self.void_system = None

    def compute(self):
        from .system import System

        rc = float(self.rc)
        if not rc > 0:
            raise ValueError(f"rc must be positive, got {self.rc}.")
        cell = self.system.box
        self.void_number, self.void_volume = 0, 0.0
        occupied = kernels.neighbor._fill_cell_for_void(*policy.positions(self.system.data), *policy.box_args(cell), rc, get_num_threads())
        x, y, z = kernels.void.void_points(occupied, cell.box, cell.origin)
        if len(x) == 0:
            return
        points = System(data={"x": x, "y": y, "z": z}, box=cell)
        points.cal_cluster_analysis(rc=rc * 1.1)
        x, y, z, ids, voids = kernels.void.prune(*policy.positions(points.data), points.data["cluster_id"], points.cluster_number)
        if voids == 0:
            return
        points.update_data({"x": x, "y": y, "z": z, "cluster_id": ids, "element": np.full(len(x), "X")}, reset_neighbor=True)
        self.void_system = points
        self.void_number = int(voids)
        self.void_volume = points.N * self.rc ** 3
