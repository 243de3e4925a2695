"""The mean squared displacement's door to the library.  The reference has NO compiled module for it
(src/mdapy/mean_squared_displacement.py does the work in numpy / pyfftw), so this module's name and the signatures of ``window``
and ``direct`` are this project's own, not a drop-in.

Both take ``pos_list`` (frames, atoms, 3), UNWRAPPED float64 positions, and the outputs ``particle_msd`` (rows, atoms) and
``msd`` (rows); either output may be ``None`` (not wanted), not both, and ``msd`` carries the same bits either way.  ``window``
fills the lags 0 .. rows - 1 (rows, from the first dimension of whichever output is given, is 1 .. frames); ``direct`` wants
rows == frames and raises ``ValueError`` otherwise.  The arrays may be numpy arrays, ``HArray``s or device tensors."""
import numpy as np

from . import _lib
from .devarray import Call

f64 = np.float64


def _dims(what, pos_list):
    shape = tuple(int(n) for n in pos_list.shape)
    if len(shape) != 3 or shape[2] != 3 or shape[0] < 1 or shape[1] < 1:
        raise ValueError(f"{what}: pos_list has shape {shape}, expected (frames >= 1, atoms >= 1, 3)")
    return shape[0], shape[1]


def _rows(what, particle_msd, msd, n_frames, n_atoms):
    """the number of rows both outputs agree on"""
    if particle_msd is None and msd is None:
        raise ValueError(f"{what}: particle_msd and msd are both None")
    given = particle_msd if particle_msd is not None else msd
    rows = int(given.shape[0]) if len(given.shape) else -1
    if particle_msd is not None and tuple(particle_msd.shape) != (rows, n_atoms):
        raise ValueError(f"{what}: particle_msd has shape {tuple(particle_msd.shape)}, expected (rows, {n_atoms})")
    if msd is not None and tuple(msd.shape) != (rows,):
        raise ValueError(f"{what}: msd has shape {tuple(msd.shape)}, expected ({rows},)")
    if not 1 <= rows <= n_frames:
        raise ValueError(f"{what}: {rows} rows for {n_frames} frames, expected 1 .. {n_frames}")
    return rows


def window(pos_list, particle_msd, msd):
    """[m, i] = the mean over the time origins t = 0 .. F-m-1 of |r[t+m, i] - r[t, i]|^2; msd[m] = its mean over the atoms"""
    F, N = _dims("window", pos_list)
    L = _rows("window", particle_msd, msd, F, N)
    c = Call(pos_list, particle_msd, msd)
    rc_ = _lib.lib().mdh_msd_window(c.inp(pos_list, f64), F, N, L,
                                    None if particle_msd is None else c.out(particle_msd, f64, upload=False),
                                    None if msd is None else c.out(msd, f64, upload=False), c.space, c.stream)
    c.done(rc_)


def direct(pos_list, particle_msd, msd):
    """[t, i] = |r[t, i] - r[0, i]|^2; msd[t] = its mean over the atoms"""
    F, N = _dims("direct", pos_list)
    if _rows("direct", particle_msd, msd, F, N) != F:
        raise ValueError(f"direct: the outputs have fewer rows than the {F} frames")
    c = Call(pos_list, particle_msd, msd)
    rc_ = _lib.lib().mdh_msd_direct(c.inp(pos_list, f64), F, N,
                                    None if particle_msd is None else c.out(particle_msd, f64, upload=False),
                                    None if msd is None else c.out(msd, f64, upload=False), c.space, c.stream)
    c.done(rc_)
