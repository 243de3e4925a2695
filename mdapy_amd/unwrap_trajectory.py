"""``unwrap_trajectory``: particle paths made continuous across the periodic boundaries, the behaviour of
``mdapy.unwrap_trajectory`` (src/mdapy/unwrap_trajectory.py:27-259) — what ``MeanSquaredDisplacement`` and
``LindemannParameter`` want as input.

The method is read from frame 0's columns: ``xu yu zu`` are taken as they are (``"unwrapped"``, no kernel); ``ix iy iz`` are
applied with every frame's own cell (``"image"``); otherwise the integer jumps of the fractional coordinates between
consecutive frames are summed over time (``"min_image"``) — which cannot tell a boundary crossing from a real move of more than
half a cell between two frames.  When frame 0 has an ``id`` column every frame's rows are put in the order of their ids.

Where the reference walks the frames in numpy, the whole trajectory goes through one call of ``kernels.unwrap`` (DESIGN.md
5j): the rows are gathered through ``row_of[f] = argsort(id[f])`` on the read side, so no sorted copy of the input is made.  The
work stays in HBM when frame 0's ``x`` column lives there; the stacked (frames, atoms, 3) result is kept on the returned
``Trajectory`` (``positions()``), and its frames' ``x y z`` columns are cut from it: in HBM on first use, on the host as the
contiguous copies a ``Frame`` column has to be."""
from __future__ import annotations

import warnings

import numpy as np

from . import kernels
from .frame import Column, Frame
from .system import System

_CARRIED = ("id", "type", "element")


def _in_hbm(column) -> bool:
    return column._host_arr is None and column._dev is not None


def _stack(frames, names, on_device, dtype):
    """(frames, atoms, len(names)) of the named columns, in stored row order"""
    if on_device:
        from .devarray import _NP2T, torch

        t = torch()
        return t.stack([t.stack([s.data[n].device_array().dev().to(_NP2T[np.dtype(dtype)]) for n in names], dim=1) for s in frames])
    out = np.empty((len(frames), frames[0].N, len(names)), dtype)
    for f, s in enumerate(frames):
        for d, n in enumerate(names):
            out[f, :, d] = s.data[n].to_numpy()
    return out


def _row_order(frames, on_device):
    """row_of (frames, atoms) int64 — row i of frame f in id order is its stored row row_of[f, i] — after the reference's checks
    (unwrap_trajectory.py:36-84); None when frame 0 has no ``id`` column"""
    n0 = frames[0].N
    has_id = "id" in frames[0].data.columns
    if has_id and len(np.unique(frames[0].data["id"].to_numpy())) != n0:
        raise ValueError("unwrap_trajectory: 'id' column in frame 0 contains duplicates; ids must uniquely label atoms.")
    for fi, s in enumerate(frames):
        if s.N != n0:
            raise ValueError("unwrap_trajectory: every frame must contain the same number of atoms; "
                             f"frame 0 has {n0}, frame {fi} has {s.N}.")
        if has_id and "id" not in s.data.columns:
            raise ValueError(f"unwrap_trajectory: frame {fi} is missing the 'id' column that frame 0 carries.")
    if not has_id:
        return None
    ids = _stack(frames, ["id"], on_device, np.int64)[:, :, 0]
    if on_device:
        from .devarray import torch

        in_order, row_of = torch().sort(ids, dim=1)
        same = (in_order == in_order[0]).all(dim=1).cpu().numpy()
    else:
        row_of = np.argsort(ids, axis=1, kind="stable")
        in_order = np.take_along_axis(ids, row_of, axis=1)
        same = (in_order == in_order[0]).all(axis=1)
    if not same.all():
        raise ValueError(f"unwrap_trajectory: frame {int(np.argmin(same))} has a different id set from frame 0 — atoms must be "
                         "the same across the whole trajectory.")
    return row_of


def _boundary(frames):
    """frame 0's flags; one warning when a later frame has others (unwrap_trajectory.py:87-100)"""
    pbc0 = np.asarray(frames[0].box.boundary, dtype=int)
    for fi, s in enumerate(frames):
        here = np.asarray(s.box.boundary, dtype=int)
        if not np.array_equal(here, pbc0):
            warnings.warn(f"unwrap_trajectory: PBC flags change between frame 0 ({pbc0.tolist()}) and frame {fi} "
                          f"({here.tolist()}); using frame 0's flags throughout.", RuntimeWarning, stacklevel=3)
            break
    return pbc0


def _warn_of_a_cell_flip(cells):
    """LAMMPS keeps a tilt factor within half of the edge it leans along and re-folds the cell when it drifts past: the cell
    matrix then jumps by about one edge, which the minimum-image scan cannot follow (unwrap_trajectory.py:116-136)"""
    for fi in range(1, len(cells)):
        before, now = cells[fi - 1], cells[fi]
        a_x, b_y = before[0, 0], before[1, 1]
        if a_x <= 0 or b_y <= 0:
            continue
        jumps = (abs(now[1, 0] - before[1, 0]) / a_x, abs(now[2, 0] - before[2, 0]) / a_x, abs(now[2, 1] - before[2, 1]) / b_y)
        if max(jumps) > 0.7:
            warnings.warn(f"unwrap_trajectory: detected a possible LAMMPS triclinic cell flip between frame {fi - 1} and frame "
                          f"{fi}. The minimum-image heuristic does not unflip the cell — consider re-dumping with "
                          "``dump_modify pbc yes`` so ix/iy/iz are written.", RuntimeWarning, stacklevel=3)
            return


def _gathered(column, rows, rows_host):
    """``column`` read through the frame's row order ``rows`` (None: as it is; a tensor when the order lives in HBM, where a
    numeric column that lives there too is gathered; ``rows_host()`` is the same order on the host, for every other column)"""
    if rows is None:
        return column
    if isinstance(rows, np.ndarray):
        return column.to_numpy()[rows]
    if _in_hbm(column) and np.dtype(column.dtype).kind in "iuf":
        from .devarray import HArray

        return HArray(column.device_array().dev()[rows])
    return column.to_numpy()[rows_host()]


def _cut(stacked, f, d, on_device):
    """column d of frame f of the stacked result"""
    if not on_device:
        return stacked[f, :, d]
    from .devarray import LazyHArray

    return LazyHArray(lambda: stacked.dev()[f, :, d].contiguous(), (stacked.shape[1],), np.float64)


def unwrap_trajectory(traj):
    from .devarray import HArray
    from .trajectory import Trajectory

    frames = list(traj)
    if len(frames) == 0:
        raise ValueError("unwrap_trajectory: trajectory has no frames.")
    if frames[0].N == 0:
        raise ValueError("unwrap_trajectory: frames contain no atoms.")
    have = set(frames[0].data.columns)
    on_device = _in_hbm(frames[0].data["xu" if {"xu", "yu", "zu"} <= have else "x"])
    row_of = _row_order(frames, on_device)
    pbc = _boundary(frames)
    method = "unwrapped" if {"xu", "yu", "zu"} <= have else "image" if {"ix", "iy", "iz"} <= have else "min_image"
    F, N = len(frames), frames[0].N

    if method == "unwrapped":
        stacked = _stack(frames, ["xu", "yu", "zu"], on_device, np.float64)
        if row_of is not None:
            if on_device:
                stacked = stacked.gather(1, row_of[:, :, None].expand(F, N, 3))
            else:
                stacked = np.take_along_axis(stacked, row_of[:, :, None], axis=1)
        if on_device:
            stacked = HArray(stacked.contiguous())
    else:
        cells = np.stack([np.asarray(s.box.box, dtype=np.float64).reshape(3, 3) for s in frames])
        if method == "min_image":
            _warn_of_a_cell_flip(cells)
        wrapped = _stack(frames, ["x", "y", "z"], on_device, np.float64)
        image = _stack(frames, ["ix", "iy", "iz"], on_device, np.int32) if method == "image" else None
        stacked = HArray.empty((F, N, 3), np.float64) if on_device else np.empty((F, N, 3), np.float64)
        kernels.unwrap.unwrap(wrapped, cells, pbc, stacked, row_of=row_of, image=image)

    carried = [name for name in _CARRIED if name in have]
    host_order = []

    def order_on_host():
        if not host_order:
            host_order.append(row_of.cpu().numpy())
        return host_order[0]

    out = []
    for f, s in enumerate(frames):
        rows = None if row_of is None else row_of[f]
        cols = {name: _gathered(s.data[name], rows, lambda f=f: order_on_host()[f]) for name in carried}
        for d, name in enumerate("xyz"):
            cols[name] = _cut(stacked, f, d, on_device)
        out.append(System(data=Frame({k: v if isinstance(v, Column) else Column(k, v) for k, v in cols.items()}), box=s.box))
    result = Trajectory(systems=out)
    result._unwrap_method = method
    result._positions = stacked
    return result
