"""Lindemann index — the drop-in for ``mdapy.lindemann_parameter.LindemannParameter`` (src/mdapy/lindemann_parameter.py:15-151):
the root-mean-square fluctuation of every pair distance over a trajectory, relative to its mean, averaged over the pairs.  It
tells a solid nanoparticle from a molten one.

``pos_list`` is (frames, atoms, 3) and holds UNWRAPPED positions: a pair distance is taken as it stands, with no minimum image.
``only_global=True`` gives ``lindemann_trj`` alone, from the pairs' sums of r and r * r; the full mode runs Welford's update per
pair and frame and also gives ``lindemann_frame`` (the index of the trajectory up to each frame) and ``lindemann_atom`` (every
atom's share of it), with ``lindemann_trj`` the last frame's value.  The two modes agree to rounding.

The reference allocates two atoms x atoms tables for either mode; nothing of that size is allocated here.  There is no ``plot``."""
import numpy as np

from . import kernels
from .parallel import get_num_threads


class LindemannParameter:
    def __init__(self, pos_list, only_global=False):
        if isinstance(pos_list, (list, tuple)):
            pos_list = np.asarray(pos_list, dtype=np.float64)
        shape = tuple(int(n) for n in getattr(pos_list, "shape", ()))
        if len(shape) != 3 or shape[2] != 3 or shape[0] < 1 or shape[1] < 2:
            raise ValueError(f"pos_list has shape {shape}: expected (frames >= 1, atoms >= 2, 3)")
        if isinstance(pos_list, np.ndarray):
            pos_list = np.ascontiguousarray(pos_list, dtype=np.float64)
        self.pos_list = pos_list
        self.only_global = only_global
        self.lindemann_trj = None
        self.lindemann_frame = None
        self.lindemann_atom = None

    def compute(self):
        n_frames, n_atoms = int(self.pos_list.shape[0]), int(self.pos_list.shape[1])
        if self.only_global:
            self.lindemann_trj = float(kernels.lindemann.compute_global(self.pos_list, None, None, get_num_threads()))
            return
        frame, atom = np.empty(n_frames, np.float64), np.empty((n_frames, n_atoms), np.float64)
        kernels.lindemann.compute_all(self.pos_list, None, None, frame, atom)
        self.lindemann_frame, self.lindemann_atom = frame, atom
        self.lindemann_trj = float(frame[-1])
