"""The arithmetic of the FIRE minimizer (csrc/fire.hip; include/mdapy_amd.h "_fire") on (n, 3) f64 arrays that stay where they
are: no reference counterpart in C++ (src/mdapy/minimizer.py:270-375 does it in numpy).  Every function works in place on the
arrays it is handed — numpy or ``HArray`` — and the scalars one step hands to the next live in ``record``, ``RECORD`` f64 words
beside the arrays: a call writes the words it computes (``VF`` ... below) and leaves the others alone."""
import numpy as np

from . import _lib
from .devarray import Call

f64, i32 = np.float64, np.int32
VF, FF, FMAX2, VV, DRDR, ZEROS, ENERGY, VIRIAL, RECORD = 0, 1, 2, 3, 4, 5, 6, 8, 24
MOVE_NORM, MOVE_CAP, MOVE_PLAIN = 0, 1, 2


def _rows(what, record, **arrays):
    """the common row count of (n, 3) arrays"""
    n = None
    for name, a in arrays.items():
        if a is None:
            continue
        if len(a.shape) != 2 or int(a.shape[1]) != 3 or (n is not None and int(a.shape[0]) != n):
            raise ValueError(f"fire.{what}: {name} has shape {tuple(a.shape)}" + ("" if n is None else f" beside {n} rows"))
        n = int(a.shape[0])
    if record is not None and tuple(record.shape) != (RECORD,):
        raise ValueError(f"fire.{what}: the record holds {RECORD} numbers")
    return n


def dots(v, f, record):
    """record[VF] = v . f (0 when v is None), record[FF] = f . f, record[FMAX2] = max |f_i|^2"""
    n = _rows("dots", record, v=v, f=f)
    c = Call(v, f, record)
    c.done(_lib.lib().mdh_fire_dots(c.inp(v, f64), c.inp(f, f64), n, c.out(record, f64), c.space, c.stream))


def kick(v, f, dt, zero_first, record):
    """v += dt * f (after v *= 0.0 when ``zero_first``); record[FF] = f . f, record[VV] = v . v"""
    n = _rows("kick", record, v=v, f=f)
    c = Call(v, f, record)
    c.done(_lib.lib().mdh_fire_kick(c.out(v, f64), c.inp(f, f64), n, float(dt), int(bool(zero_first)), c.out(record, f64), c.space, c.stream))


def mix(v, f, a, abc_multiplier, use_abc, dt, record):
    """v = (1 - a) v + ((a f) / sqrt(f . f)) sqrt(v . v), times ``abc_multiplier`` with ``use_abc``; record[DRDR] and record[ZEROS]"""
    n = _rows("mix", record, v=v, f=f)
    c = Call(v, f, record)
    c.done(_lib.lib().mdh_fire_mix(c.out(v, f64), c.inp(f, f64), n, float(a), float(abc_multiplier), int(bool(use_abc)), float(dt),
                                   c.out(record, f64), c.space, c.stream))


def move(v, dr, n_atoms, scale, dt, maxstep, mode, record, x=None, y=None, z=None, x_out=None, y_out=None, z_out=None, unstrained=None):
    """dr = scale * v, limited as ``mode`` says; the first ``n_atoms`` rows move ``unstrained`` in place or x, y, z into the new columns"""
    n = _rows("move", record, v=v, dr=dr)
    n_atoms = int(n_atoms)
    if unstrained is not None:
        if tuple(unstrained.shape) != (n_atoms, 3):
            raise ValueError(f"fire.move: unstrained has shape {tuple(unstrained.shape)} for {n_atoms} atoms")
    else:
        _lib.same_rows("fire.move", n_atoms, x=x, y=y, z=z, x_out=x_out, y_out=y_out, z_out=z_out)
    c = Call(v, dr, record, x, y, z, x_out, y_out, z_out, unstrained)
    out = (lambda a: None if a is None else c.out(a, f64, upload=False))
    c.done(_lib.lib().mdh_fire_move(c.out(v, f64), c.out(dr, f64, upload=False), n, n_atoms, float(scale), float(dt), float(maxstep), int(mode),
                                    c.inp(record, f64), c.inp(x, f64), c.inp(y, f64), c.inp(z, f64), out(x_out), out(y_out), out(z_out),
                                    None if unstrained is None else c.out(unstrained, f64), c.space, c.stream))


def rowmat(rows, matrix, out_rows=None, out_x=None, out_y=None, out_z=None):
    """rows @ matrix with o_k = (x m_0k + y m_1k) + z m_2k, into ``out_rows`` or into three columns"""
    n = _rows("rowmat", None, rows=rows, out_rows=out_rows)
    m = np.ascontiguousarray(np.asarray(matrix, f64).reshape(3, 3))
    if out_rows is None:
        _lib.same_rows("fire.rowmat", n, out_x=out_x, out_y=out_y, out_z=out_z)
    c = Call(rows, out_rows, out_x, out_y, out_z)
    out = (lambda a: None if a is None else c.out(a, f64, upload=False))
    c.done(_lib.lib().mdh_fire_rowmat(c.inp(rows, f64), n, m.ctypes.data, out(out_rows), out(out_x), out(out_y), out(out_z), c.space, c.stream))


def scatter_rows(rows, perm, out_rows):
    """out_rows[perm[p]] = rows[p]"""
    n = _rows("scatter_rows", None, rows=rows, out_rows=out_rows)
    _lib.same_rows("fire.scatter_rows", n, perm=perm)
    c = Call(rows, perm, out_rows)
    c.done(_lib.lib().mdh_fire_scatter_rows(c.inp(rows, f64), c.inp(perm, i32), n, c.out(out_rows, f64), c.space, c.stream))


def total(values, word, record):
    """record[word] = the sum of a 1-D array, in the fixed order of the dot products"""
    _rows("total", record)
    c = Call(values, record)
    c.done(_lib.lib().mdh_fire_sum(c.inp(values, f64), int(len(values)), int(word), c.out(record, f64), c.space, c.stream))
