"""Mean squared displacement of an unwrapped trajectory — what a diffusion coefficient is read from.  The class has the
attributes of ``mdapy.mean_squared_displacement.MeanSquaredDisplacement`` (src/mdapy/mean_squared_displacement.py:15-172)
without its ``plot``.

``pos_list`` is (frames, atoms, 3) and holds UNWRAPPED positions.  ``mode="window"`` averages |r[t+m] - r[t]|^2 over every
time origin t for each lag m = 0 .. frames-1; ``mode="direct"`` takes |r[t] - r[0]|^2.  ``compute()`` sets ``particle_msd``
(frames, atoms) and ``msd`` (frames,), its mean over the atoms.

The reference takes the windowed form through S1 - 2 S2 with an FFT autocorrelation (in complex64 where pyfftw is installed),
which cancels for positions far from the origin.  Here the definition is summed term by term in binary64 on the device: every
term is non-negative, a lattice walk comes out exact, and adding a constant to every position changes nothing."""
import numpy as np

from . import kernels


class MeanSquaredDisplacement:
    def __init__(self, pos_list, mode="window"):
        if mode not in ("window", "direct"):
            raise ValueError(f"mode is {mode!r}: expected 'window' or 'direct'")
        if isinstance(pos_list, (list, tuple)):
            pos_list = np.asarray(pos_list, dtype=np.float64)
        shape = tuple(int(n) for n in getattr(pos_list, "shape", ()))
        if len(shape) != 3 or shape[2] != 3 or shape[0] < 1 or shape[1] < 1:
            raise ValueError(f"pos_list has shape {shape}: expected (frames >= 1, atoms >= 1, 3)")
        if isinstance(pos_list, np.ndarray):
            pos_list = np.ascontiguousarray(pos_list, dtype=np.float64)
        self.pos_list = pos_list
        self.mode = mode
        self.particle_msd = None
        self.msd = None

    def compute(self):
        n_frames, n_atoms = int(self.pos_list.shape[0]), int(self.pos_list.shape[1])
        table, mean = np.empty((n_frames, n_atoms), np.float64), np.empty(n_frames, np.float64)
        run = kernels.msd.window if self.mode == "window" else kernels.msd.direct
        run(self.pos_list, table, mean)
        self.particle_msd, self.msd = table, mean
