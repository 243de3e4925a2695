"""The trajectory unwrap's door to the library.  The reference has NO compiled module for it (src/mdapy/unwrap_trajectory.py
walks the frames in numpy), so this module's name and the signature of ``unwrap`` are this project's own, not a drop-in.

``unwrap`` takes ``pos`` (frames, atoms, 3), WRAPPED float64 positions, ``cells`` (frames, 3, 3) on the host (rows a, b, c of
every frame's own cell) and ``pbc`` (3 flags), and fills ``unwrapped`` (frames, atoms, 3) float64.  ``row_of`` (frames, atoms)
int64 makes output row i of frame f the input row ``row_of[f, i]``; ``image`` (frames, atoms, 3) int32, indexed like ``pos``,
switches from the minimum-image scan to the image flags; ``shifts`` (frames, atoms, 3) int64 receives the integer shift of every
atom and frame.  ``chunks`` is how many runs the frame axis is cut into (0: the library chooses); it changes no bit of the result.
The arrays may be numpy arrays, ``HArray``s or device tensors.  The arithmetic: include/mdapy_amd.h, the ``_unwrap`` section."""
import numpy as np

from . import _lib
from .devarray import Call

f64, i64, i32 = np.float64, np.int64, np.int32

AB = 64  # atoms per workgroup (csrc/unwrap.hip UW_AB)
T = 16   # chunks = 0 cuts the frames into at most ceil(frames / T) runs (UW_T)


def _shape(a):
    return tuple(int(n) for n in getattr(a, "shape", ()))


def unwrap(pos, cells, pbc, unwrapped, row_of=None, image=None, shifts=None, chunks=0):
    shape = _shape(pos)
    if len(shape) != 3 or shape[2] != 3 or shape[0] < 1 or shape[1] < 1:
        raise ValueError(f"unwrap: pos has shape {shape}, expected (frames >= 1, atoms >= 1, 3)")
    F, N = shape[:2]
    cells = np.ascontiguousarray(cells, dtype=f64)
    if cells.shape != (F, 3, 3):
        raise ValueError(f"unwrap: cells has shape {cells.shape}, expected ({F}, 3, 3)")
    flags = np.asarray(pbc)
    if flags.shape != (3,):
        raise ValueError(f"unwrap: pbc has shape {flags.shape}, expected (3,)")
    flags = np.ascontiguousarray(flags != 0, dtype=i32)
    if unwrapped is None or _shape(unwrapped) != shape:
        raise ValueError(f"unwrap: unwrapped has shape {None if unwrapped is None else _shape(unwrapped)}, expected {shape}")
    if row_of is not None and _shape(row_of) != (F, N):
        raise ValueError(f"unwrap: row_of has shape {_shape(row_of)}, expected ({F}, {N})")
    if image is not None and _shape(image) != shape:
        raise ValueError(f"unwrap: image has shape {_shape(image)}, expected {shape}")
    if shifts is not None and _shape(shifts) != shape:
        raise ValueError(f"unwrap: shifts has shape {_shape(shifts)}, expected {shape}")
    if int(chunks) != chunks or chunks < 0:
        raise ValueError(f"unwrap: chunks is {chunks!r}, expected an integer >= 0")
    inv = None
    if image is None:
        if not np.isfinite(cells).all():
            raise ValueError(f"unwrap: the cell of frame {int(np.argmax(~np.isfinite(cells).all(axis=(1, 2))))} is not finite")
        try:  # (LAPACK, one matrix at a time: 2.7 ms for 16 384 frames, several times the kernels; a cell that never changes is inverted once)
            inv = np.repeat(np.linalg.inv(cells[:1]), F, axis=0) if F > 1 and (cells == cells[0]).all() else np.linalg.inv(cells)
            inv = np.ascontiguousarray(inv)
        except np.linalg.LinAlgError:
            inv = None
        if inv is None or not np.isfinite(inv).all():
            for f in range(F):
                try:
                    if np.isfinite(np.linalg.inv(cells[f])).all():
                        continue
                except np.linalg.LinAlgError:
                    pass
                raise ValueError(f"unwrap: the cell of frame {f} is singular")
    c = Call(pos, unwrapped, row_of, image, shifts)
    rc_ = _lib.lib().mdh_unwrap_trajectory(c.inp(pos, f64), c.inp(row_of, i64), c.inp(image, i32), cells.ctypes.data,
                                           None if inv is None else inv.ctypes.data, flags.ctypes.data, F, N, int(chunks),
                                           c.out(unwrapped, f64, upload=False),
                                           None if shifts is None else c.out(shifts, i64, upload=False), c.space, c.stream)
    c.done(rc_)
