"""``Trajectory``: the frames of a multi-frame LAMMPS dump or (extended) XYZ file as a list of ``System``s — the list
interface and the constructor of ``mdapy.Trajectory`` (src/mdapy/trajectory.py:35-150, 1162-1325).

One pass over the file finds the byte range of every frame (a dump frame starts at each ``ITEM: TIMESTEP`` line; an XYZ frame
is a count line, a comment line and that many rows); every frame is then parsed by the code the single-frame readers of
``load_save`` use, so a large frame's table is tokenised in HBM and a small one on the host, as there.

``save`` writes the dump format (frame after frame through ``load_save.write_dump_frame_to``).  Not built:
saving as XYZ, ``XYZTrajectory``, the ``vacuum`` padding and the progress bar — ``verbose`` is accepted and prints nothing;
``fast_mode`` is accepted for XYZ and changes nothing, there being one reader.  ``positions()`` is this project's own
addition, not the reference's."""
from __future__ import annotations

from typing import List, Optional

import numpy as np

from . import load_save
from .system import System


def _infer_format(filename: str) -> str:
    f = str(filename).lower()
    if f.endswith(".gz"):
        f = f[:-3]
    if f.endswith((".xyz", ".extxyz")):
        return "xyz"
    if f.endswith((".dump", ".lammpstrj", ".trj")):
        return "dump"
    raise ValueError(f"Cannot infer trajectory format from {filename!r}; pass format='xyz' or format='dump' explicitly.")


def _dump_starts(f) -> List[int]:
    """byte offsets of the lines that start with ``ITEM: TIMESTEP`` (blanks before it allowed), and the size of the file last.
    The file is searched in pieces that end at a line end: what follows a piece's last line end waits for the next piece."""
    needle = b"ITEM: TIMESTEP"
    starts, base, carry = [], 0, b""
    f.seek(0)
    while True:
        chunk = f.read(1 << 24)
        buf = carry + chunk
        whole = len(buf) if not chunk else buf.rfind(b"\n") + 1  # (the last piece may end without a line end)
        at = buf.find(needle, 0, whole)
        while at >= 0:
            line = buf.rfind(b"\n", 0, at) + 1
            if not buf[line:at].strip():
                starts.append(base + line)
            at = buf.find(needle, at + len(needle), whole)
        base, carry = base + whole, buf[whole:]
        if not chunk:
            return starts + [base]


def _read_dump_frames(filename: str) -> List[System]:
    with load_save._open(filename) as f:
        marks = _dump_starts(f)
        if len(marks) < 2:
            raise ValueError(f"{filename}: no ITEM: TIMESTEP header found")
        systems = []
        for k in range(len(marks) - 1):
            head, offset = load_save._header(f, 9, marks[k])
            frame, box, info = load_save._dump_frame(f, head, offset, marks[k + 1], f"{filename}[frame {k}]")
            systems.append(System(data=frame, box=box, global_info=info))
    return systems


def _xyz_ranges(f):
    """[(count line, comment line, first byte of the rows, first byte after them)] of every complete frame; like the
    reference's serial reader (trajectory.py:389-439) the walk ends at a blank count line or a frame cut short"""
    f.seek(0)
    out, offset = [], 0
    while True:
        count = f.readline()
        if not count.strip():
            break
        comment = f.readline()
        if not comment:
            break
        n = int(count.strip())
        body = offset + len(count) + len(comment)
        end, rows = body, 0
        for _ in range(n):
            ln = f.readline()
            if not ln:
                break
            end += len(ln)
            rows += 1
        if rows != n:
            break
        out.append((count.decode().rstrip("\r\n"), comment.decode().rstrip("\r\n"), body, end))
        offset = end
    return out


def _read_xyz_frames(filename: str) -> List[System]:
    with load_save._open(filename) as f:
        systems = []
        for k, (count, comment, body, end) in enumerate(_xyz_ranges(f)):
            frame, box, info = load_save._xyz_frame(f, [count, comment], body, end, f"{filename}[frame {k}]")
            systems.append(System(data=frame, box=box, global_info=info))
    return systems


def _a_frame(system, verb: str) -> System:
    if isinstance(system, System):
        return system
    raise TypeError(f"only System instances can be {verb}" if verb != "assigned" else "can only assign System instances")


class Trajectory:
    def __init__(self, filename: Optional[str] = None, systems: Optional[List[System]] = None, format: Optional[str] = None,
                 fast_mode: bool = False, verbose: bool = True) -> None:
        if systems is None and filename is None:
            raise ValueError("Trajectory needs either filename= or systems=")
        self._filename, self._format, self._fast_mode, self._verbose = filename, format, bool(fast_mode), verbose
        self._positions = None  # the stacked (frames, atoms, 3) result of unwrap_trajectory, on the object it returns
        self._systems: List[System] = [*systems] if systems is not None else self._read(str(filename))

    def _read(self, filename: str) -> List[System]:
        kind = self._format if self._format else _infer_format(filename)
        if kind == "dump" and self._fast_mode:
            raise ValueError("fast_mode is not supported for LAMMPS dump format. The dump reader already converts each "
                             "frame's table in one piece, so a separate bulk path would add complexity without measurable "
                             "speedup. Pass fast_mode=False (the default).")
        readers = {"xyz": _read_xyz_frames, "dump": _read_dump_frames}
        if kind not in readers:
            raise ValueError(f"Unsupported trajectory format: {kind!r}")
        return readers[kind](filename)

    # ---- the list interface (trajectory.py:35-150)
    def _changed(self):
        self._positions = None  # (the stacked array of unwrap() no longer describes the frames)

    def _chosen(self, idx) -> np.ndarray:
        """the frame numbers an index array picks: a boolean mask of length ``len(self)``, or integers, negative ones counting
        from the end"""
        count = len(self._systems)
        wanted = np.asarray(idx)
        if wanted.dtype == bool:
            if wanted.shape != (count,):
                raise IndexError(f"boolean mask must have length {count} to index a {count}-frame trajectory; "
                                 f"got length {wanted.shape[0] if wanted.ndim else 'scalar'}.")
            return np.flatnonzero(wanted)
        if wanted.dtype.kind not in "iu":
            raise TypeError(f"trajectory index array must be bool or integer; got dtype {wanted.dtype}.")
        wanted = wanted.astype(np.int64).ravel()
        wanted = np.where(wanted < 0, wanted + count, wanted)
        outside = (wanted < 0) | (wanted >= count)
        if outside.any():
            raise IndexError(f"frame index {int(wanted[outside][0])} out of bounds for {count}-frame trajectory.")
        return wanted

    def __getitem__(self, idx):
        """an int gives the frame (a ``System``); a slice, a list / tuple / 1-D array of integers or a boolean mask give a
        ``Trajectory`` of the chosen frames"""
        if isinstance(idx, slice):
            return type(self)(systems=self._systems[idx])
        if isinstance(idx, (np.ndarray, list, tuple)):
            return type(self)(systems=[self._systems[k] for k in self._chosen(idx)])
        return self._systems[idx]

    def __setitem__(self, idx: int, system: System) -> None:
        self._systems[idx] = _a_frame(system, "assigned")
        self._changed()

    def __len__(self) -> int:
        return len(self._systems)

    def __iter__(self):
        yield from self._systems

    def __repr__(self) -> str:
        return f"<{type(self).__name__}: {len(self._systems)} frame(s)>"

    def insert(self, index: int, system: System) -> None:
        self._systems.insert(index, _a_frame(system, "inserted"))
        self._changed()

    def append(self, system: System) -> None:
        self._systems.append(_a_frame(system, "appended"))
        self._changed()

    def extend(self, systems) -> None:
        for one in systems:
            self.append(one)

    def pop(self, index: int = -1) -> System:
        self._changed()
        return self._systems.pop(index)

    def remove(self, indices) -> None:
        """drop the frame, or the frames, with these numbers (as they are before the call)"""
        gone = {indices} if isinstance(indices, int) else set(indices)
        count = len(self._systems)
        gone = {k + count if k < 0 else k for k in gone}
        if any(k < 0 or k >= count for k in gone):
            raise IndexError("pop index out of range")
        self._systems = [s for k, s in enumerate(self._systems) if k not in gone]
        self._changed()

    def get_atoms_count(self) -> np.ndarray:
        return np.fromiter((s.N for s in self._systems), dtype=np.int64, count=len(self._systems))

    def concatenate(self, other: "Trajectory") -> "Trajectory":
        return type(self)(systems=[*self._systems, *other._systems])

    def save(self, filename: str, frames=None, mode: str = "w", format: Optional[str] = None) -> None:
        """write the frames — all of them, one (an int) or some (a list of ints) — as a multi-frame LAMMPS dump file, one frame
        after another through ``load_save.write_dump_frame_to``; ``mode='a'`` appends to an existing file; a name that ends in
        ``.gz`` is written gzipped.  Each frame's ``ITEM: TIMESTEP`` is its ``global_info['timestep']`` as an integer, 0 without
        one (trajectory.py:1147-1159, 1257-1313)."""
        if frames is None:
            chosen = self._systems
        elif isinstance(frames, int):
            chosen = [self._systems[frames]]
        else:
            chosen = [self._systems[i] for i in frames]
        if mode not in ("w", "a"):
            raise ValueError(f"mode must be 'w' or 'a', got {mode!r}")
        kind = format or _infer_format(filename)
        if kind == "xyz":
            raise NotImplementedError("Trajectory.save writes the LAMMPS dump format only: the reference's multi-frame XYZ has a header "
                                      "style of its own (and a vacuum option) that is not built here. Use format='dump', or write "
                                      "single frames with System.write_xyz.")
        if kind != "dump":
            raise ValueError(f"Unsupported trajectory format: {kind!r}")
        with load_save._open(str(filename), mode + "b") as op:
            for one in chosen:
                step = one.global_info.get("timestep", 0) if one.global_info else 0
                try:
                    step = int(step)
                except (TypeError, ValueError):
                    step = 0
                load_save.write_dump_frame_to(op, one.box, one.data, step)

    # ---- analyses
    def unwrap(self) -> "Trajectory":
        """a new ``Trajectory`` with continuous positions: ``unwrap_trajectory(self)``"""
        from .unwrap_trajectory import unwrap_trajectory

        return unwrap_trajectory(self)

    def positions(self):
        """THIS PROJECT'S ADDITION (the reference's ``Trajectory`` has no such method): the positions of all frames as one
        (frames, atoms, 3) float64 array, what ``MeanSquaredDisplacement`` and ``LindemannParameter`` take.  On the result of
        ``unwrap()`` it is the kernel's own output — an ``HArray`` in HBM when the input's columns lived there, no host round
        trip —; otherwise ``x y z`` of every frame stacked in stored row order.  ``ValueError`` when frames differ in atom count."""
        if self._positions is not None:
            return self._positions
        counts = self.get_atoms_count()
        if len(counts) == 0:
            raise ValueError("positions: trajectory has no frames.")
        if np.any(counts != counts[0]):
            f = int(np.argmax(counts != counts[0]))
            raise ValueError(f"positions: every frame must contain the same number of atoms; frame 0 has {int(counts[0])}, "
                             f"frame {f} has {int(counts[f])}.")
        out = np.empty((len(counts), int(counts[0]), 3), np.float64)
        for f, s in enumerate(self._systems):
            for d, name in enumerate("xyz"):
                out[f, :, d] = s.data[name].to_numpy()
        return out
