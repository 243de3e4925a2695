"""Input side of the hot path: LAMMPS dump and data, (extended) XYZ and ``.mp`` (parquet) files -> ``(Frame,
Box, info)``, the triple ``System(filename)`` is built from.

Behaviour follows the reference's readers — ``src/mdapy/load_save.py:66-198`` (one dump frame: the three BOX BOUNDS forms,
integer / string / float column classes, scaled and unwrapped coordinate columns), ``:653-863`` (XYZ: lower-cased
``key=value`` comment line, ``Properties=`` triples with the pos / species / vel / forces aliases, cell-less "classical"
files) and ``:610-650`` (``.mp``: a parquet file whose key-value metadata carries box / origin / boundary).  What differs is
where the atom table is converted: the reference slurps the file and calls a CSV reader on the host; here the header is
parsed on the host (a few lines) and the table's bytes are streamed into HBM, tokenised and converted there
(``_text.py`` / ``csrc/text.hip``, correctly rounded = ``float()``), so that a 10^7-atom file arrives as HBM-resident
columns without a host-side table ever existing.  Files below ``DEVICE_MIN_BYTES`` — and any file on a machine without a
GPU — take the host tokenizer instead (same values; it is I/O plumbing, not a compute fallback).  A LAMMPS data file
(``:1036-1323``) has sections in any order and a Velocities table keyed by atom id: see ``read_data`` below.

The output side is further down: ``write_dump`` / ``write_dump_frame_to``, ``write_xyz``, ``write_data``, ``write_poscar``
(``src/mdapy/load_save.py:1565-2017``) beside ``write_mp``, the inverse arrangement — headers on the host, the atom table
formatted in HBM (``_text.py`` / ``csrc/text_format.hip``, every float exactly ``format(v, ".10f")``) and streamed to the file."""
from __future__ import annotations

import gzip
import io
import os
import re
from typing import Any, Dict, List, Optional, Tuple

import numpy as np

from .box import Box
from .devarray import have_gpu
from .frame import Frame

DEVICE_MIN_BYTES = 1 << 20
FLOAT, INT, STR = 0, 1, 2
_INT_COLUMNS = {"id", "type", "ix", "iy", "iz", "mol", "proc", "procp1"}  # load_save.py:147
_STR_COLUMNS = {"element", "typelabel"}


def _open(path, mode="rb"):
    return gzip.open(path, mode) if str(path).endswith(".gz") else open(path, mode)


# ---------------------------------------------------------------------------------------------------------------------
# the atom table
# ---------------------------------------------------------------------------------------------------------------------
def _int32(values: np.ndarray) -> np.ndarray:
    """int64 -> int32, refusing what does not fit (numpy's own refusal when the reference converts such a field)"""
    out = values.astype(np.int32)
    if not np.array_equal(out, values):
        raise OverflowError(f"Python integer {int(values[out != values][0])} out of bounds for int32")
    return out


def _table_on_host(body: bytes, nrows: int, names: List[str], kinds: List[int], source: str) -> Dict[str, np.ndarray]:
    """host tokenizer: pandas' C reader with exact (round-trip) conversion where the table is plain, str.split otherwise.
    The table is the next ``nrows`` lines, as in the reference (load_save.py:141-175): a blank line is a row without fields, not
    something to skip; a row that lacks its last fields is an error even where those are strings; an integer column holds
    integers (``3.0`` and ``1e3`` are errors) that fit int32.  pandas would let each of these pass (it skips, fills in ``''``,
    reads ``3.0`` as 3 and wraps 2^31), so it only gets the tables it reads as they are: the integer columns are left to its
    type inference, and anything but int64 there — like every other doubt — sends the table to str.split, whose conversions are
    the reference's."""
    try:
        import pandas as pd

        dtypes = {n: {FLOAT: np.float64, STR: str}[k] for n, k in zip(names, kinds) if k != INT}
        df = pd.read_csv(io.BytesIO(body), sep=r"\s+", header=None, names=list(names), nrows=nrows, dtype=dtypes, engine="c",
                         float_precision="round_trip", na_filter=False, index_col=False, usecols=range(len(names)), skip_blank_lines=False)
        plain = len(df) == nrows and df.shape[1] == len(names) and all(df[n].dtype == np.int64 for n, k in zip(names, kinds) if k == INT)
        if plain and kinds[-1] == STR and (df[names[-1]] == "").any():  # (a missing number fails to convert; a missing string comes back empty)
            plain = False
        if plain:
            return {n: (df[n].to_numpy(dtype=object) if k == STR else _int32(df[n].to_numpy()) if k == INT else np.ascontiguousarray(df[n].to_numpy()))
                    for n, k in zip(names, kinds)}
    except Exception:
        pass
    rows = [ln.split()[: len(names)] for ln in body.decode().splitlines()[:nrows]]
    if len(rows) != nrows or any(len(r) != len(names) for r in rows):
        raise ValueError(f"{source}: expected {nrows} atom rows with {len(names)} fields each")
    out = {}
    for j, (n, k) in enumerate(zip(names, kinds)):
        col = [r[j] for r in rows]
        out[n] = np.array(col, dtype=object) if k == STR else np.array(col, dtype=np.float64) if k == FLOAT else _int32(np.array(col, dtype=np.int64))
    return out


class _UpTo:
    """the next ``left`` bytes of a binary file, as the file object ``_text.stream_to_device`` reads from"""

    def __init__(self, f, left: int):
        self._f, self._left = f, left

    def readinto(self, view):
        if self._left <= 0:
            return 0
        got = self._f.readinto(view[: self._left] if len(view) > self._left else view)
        self._left -= got or 0
        return got


class _At:
    """``source`` positioned ``offset`` bytes into its (decompressed) content.  A source is a path, opened here and closed
    again, or a binary file that is open already: a trajectory reads all its frames through one handle, front to back, so that a
    compressed file is inflated once."""

    def __init__(self, source, offset: int):
        self._source, self._offset, self._mine = source, offset, None

    def __enter__(self):
        f = self._source
        if isinstance(f, str):
            f = self._mine = _open(f)
        f.seek(self._offset)
        return f

    def __exit__(self, *exc):
        if self._mine is not None:
            self._mine.close()


def _name(source) -> str:
    return source if isinstance(source, str) else str(getattr(source, "name", source))


def _table(source, offset: int, nrows: int, names: List[str], kinds: List[int], end: Optional[int] = None):
    """columns of the table in bytes ``offset .. end`` of the (decompressed) source, ``end`` None: up to the end of the file;
    (columns, lines present or None)"""
    if end is not None:
        size = end - offset
    else:
        size = None if _name(source).endswith(".gz") else os.path.getsize(_name(source)) - offset
    if have_gpu() and nrows > 0 and (size is None or size >= DEVICE_MIN_BYTES):
        from . import _text

        with _At(source, offset) as f:
            text, _ = _text.stream_to_device(f if end is None else _UpTo(f, size), size)
        try:
            cols, lines = _text.parse_table(text, nrows, kinds)
            return dict(zip(names, cols)), lines
        except _text.RedoOverflow:  # e.g. a column of strings longer than 8 bytes on every atom: the host tokenizer reads it
            del text
    with _At(source, offset) as f:
        body = f.read() if end is None else f.read(size)
    return _table_on_host(body, nrows, names, kinds, _name(source)), None


def _header(source, nlines: int, start: int = 0) -> Tuple[List[str], int]:
    """the first nlines lines from byte ``start`` on (decoded, without line ends) and the byte offset of what follows"""
    out, offset = [], start
    with _At(source, start) as f:
        for _ in range(nlines):
            ln = f.readline()
            if not ln:
                break
            offset += len(ln)
            out.append(ln.decode().rstrip("\r\n"))
    return out, offset


def _frame(cols: Dict[str, Any]) -> Frame:
    ordered = {k: cols[k] for k in ("x", "y", "z")}
    ordered.update({k: v for k, v in cols.items() if k not in ordered})
    return Frame(ordered)


def _host(a) -> np.ndarray:
    return a.numpy() if hasattr(a, "numpy") else np.asarray(a)


# ---------------------------------------------------------------------------------------------------------------------
# LAMMPS dump (one frame)
# ---------------------------------------------------------------------------------------------------------------------
def _dump_box(bounds_line: str, rows: List[List[str]]):
    """BOX BOUNDS header + its three lines -> (box 4x3 with the origin last, boundary); load_save.py:84-134"""
    tokens = bounds_line.split()[3:]
    if tokens and all(t in ("pp", "ff", "ss", "mm") for t in tokens[-3:]):
        boundary = [1 if t == "pp" else 0 for t in tokens[-3:]]
        geometry = tokens[:-3]
    else:
        boundary, geometry = [1, 1, 1], tokens
    if "abc" in geometry and "origin" in geometry:  # general triclinic: three cell vectors and the origin, one per line
        cell = np.array([r[:3] for r in rows], dtype=np.float64)
        origin = np.array([r[3] for r in rows], dtype=np.float64)
        return np.vstack([cell, origin]), boundary
    num = [[float(v) for v in r] for r in rows]
    if all(t in geometry for t in ("xy", "xz", "yz")):  # restricted triclinic: bounds of the bounding box + tilts
        (xlo_b, xhi_b, xy), (ylo_b, yhi_b, xz), (zlo, zhi, yz) = (r[:3] for r in num)
        xlo, xhi = xlo_b - min(0.0, xy, xz, xy + xz), xhi_b - max(0.0, xy, xz, xy + xz)
        ylo, yhi = ylo_b - min(0.0, yz), yhi_b - max(0.0, yz)
        return np.array([[xhi - xlo, 0, 0], [xy, yhi - ylo, 0], [xz, yz, zhi - zlo], [xlo, ylo, zlo]], dtype=np.float64), boundary
    (xlo, xhi), (ylo, yhi), (zlo, zhi) = (r[:2] for r in num)
    return np.array([[xhi - xlo, 0, 0], [0, yhi - ylo, 0], [0, 0, zhi - zlo], [xlo, ylo, zlo]], dtype=np.float64), boundary


def _dump_frame(source, head: List[str], offset: int, end: Optional[int] = None, what: Optional[str] = None):
    """one dump frame -> (Frame, Box, info): ``head`` its nine header lines, its table the bytes ``offset .. end`` of the source
    (``end`` None: the single-frame reader, whose table runs to the end of the file and must not be followed by another frame)"""
    path = what or _name(source)
    if len(head) < 9:
        raise ValueError(f"{path}: dump frame has only {len(head)} lines (<9)")
    if not head[0].strip().startswith("ITEM: TIMESTEP"):
        raise ValueError(f"{path}: no 'ITEM: TIMESTEP' header found")
    try:
        timestep = int(head[1].strip())
    except ValueError:
        raise ValueError(f"{path}: malformed ITEM: TIMESTEP value")
    try:
        n = int(head[3].strip())
    except ValueError:
        raise ValueError(f"{path}: malformed ITEM: NUMBER OF ATOMS value")
    if not head[4].strip().startswith("ITEM: BOX BOUNDS"):
        raise ValueError(f"{path}: expected 'ITEM: BOX BOUNDS' on line 5")
    box, boundary = _dump_box(head[4].strip(), [head[5].split(), head[6].split(), head[7].split()])
    if not head[8].startswith("ITEM: ATOMS"):
        raise ValueError(f"{path}: expected 'ITEM: ATOMS' on line 9")
    names = head[8].split()[2:]
    kinds = [INT if nm in _INT_COLUMNS else STR if nm in _STR_COLUMNS else FLOAT for nm in names]
    cols, lines = _table(source, offset, n, names, kinds, end)
    if end is None and (lines is None or lines > n) and _has_second_frame(source, offset):  # rows beyond the frame: is it another frame?
        raise ValueError(f"{path}: multi-frame dump file. Use a trajectory reader or split the file first.")
    have = set(cols)
    if not {"x", "y", "z"} <= have:  # load_save.py:182-196
        for tag in ("xs", "xsu"):
            trio = [tag, tag.replace("x", "y"), tag.replace("x", "z")]
            if set(trio) <= have:
                scaled = np.column_stack([_host(cols.pop(t)) for t in trio])
                absolute = box[3] + scaled @ box[:3]
                cols["x"], cols["y"], cols["z"] = (np.ascontiguousarray(absolute[:, k]) for k in range(3))
                break
        else:
            if {"xu", "yu", "zu"} <= have:
                cols["x"], cols["y"], cols["z"] = cols.pop("xu"), cols.pop("yu"), cols.pop("zu")
            else:
                raise ValueError(f"{path}: the dump has no coordinate columns (x y z, xs ys zs, xu yu zu or xsu ysu zsu); got {names}")
    return _frame(cols), Box(box[:3], boundary, box[3]), {"timestep": timestep}


def read_dump(path) -> Tuple[Frame, Box, Dict[str, Any]]:
    path = str(path)
    head, offset = _header(path, 9)
    return _dump_frame(path, head, offset)


def _has_second_frame(path, offset: int) -> bool:
    needle = b"ITEM: TIMESTEP"
    with _At(path, offset) as f:
        carry = b""
        while True:
            chunk = f.read(1 << 24)
            if not chunk:
                return False
            if needle in carry + chunk:
                return True
            carry = chunk[-len(needle):]


# ---------------------------------------------------------------------------------------------------------------------
# XYZ (classical and extended)
# ---------------------------------------------------------------------------------------------------------------------
_ALIASES = [  # (names in the Properties string, type, columns) — load_save.py:760-785
    (("pos",), "R", ["x", "y", "z"]),
    (("unwrapped_position", "unwrapped_pos"), "R", ["xu", "yu", "zu"]),
    (("vel", "velo"), "R", ["vx", "vy", "vz"]),
    (("force", "forces"), "R", ["fx", "fy", "fz"]),
]


def _xyz_columns(properties: str, source: str) -> Tuple[List[str], List[int]]:
    parts = properties.strip().split(":")
    names: List[str] = []
    kinds: List[int] = []
    kind_of = {"S": STR, "R": FLOAT, "I": INT}
    for name, ptype, count in zip(parts[0::3], parts[1::3], parts[2::3]):
        if ptype not in kind_of:
            raise ValueError(f"{source}: unrecognised XYZ type {ptype!r}")
        count = int(count)
        sub = None
        if ptype == "S" and count == 1 and name in ("species", "element") and "element" not in names:
            sub = ["element"]
        for keys, want, target in _ALIASES:
            if name in keys and ptype == want and count == 3 and target[0] not in names:
                sub = target
        if sub is None:
            sub = [name] if count == 1 else [f"{name}_{j}" for j in range(count)]
        for c in sub:
            base, k = c, 0
            while c in names:  # a second occurrence of a name keeps the rows aligned under a suffixed column
                k += 1
                c = f"{base}__{k}"
            names.append(c)
            kinds.append(kind_of[ptype])
    return names, kinds


def _xyz_frame(source, head: List[str], offset: int, end: Optional[int] = None, what: Optional[str] = None):
    """one XYZ frame -> (Frame, Box, info): ``head`` its count and comment lines, its table the bytes ``offset .. end`` of the
    source (``end`` None: to the end of the file)"""
    path = what or _name(source)
    if len(head) < 2:
        raise ValueError(f"{path}: too short to be an XYZ file")
    n = int(head[0].strip())
    if n < 0:
        raise ValueError(f"{path}: negative atom count {n}")
    info: Dict[str, Any] = {}
    for key, quoted, bare in re.findall(r'(\w+)=(?:"([^"]+)"|([^ ]+))', head[1].replace("'", '"')):
        info[key.lower()] = quoted if quoted else bare
    classical = "lattice" not in info  # no cell given: the box is the extent of the coordinates
    if "properties" in info:
        names, kinds = _xyz_columns(info["properties"], path)
    elif not classical:
        raise ValueError(f"{path}: extended XYZ must contain a 'properties=' field")
    else:
        names, kinds = ["element", "x", "y", "z"], [STR, FLOAT, FLOAT, FLOAT]
    if "pbc" in info:
        boundary = [1 if t in ("T", "1") else 0 for t in info["pbc"].split()]
    else:
        boundary = [0, 0, 0] if classical else [1, 1, 1]
    origin = np.array(info["origin"].split(), dtype=np.float64) if "origin" in info else np.zeros(3)
    cols, lines = _table(source, offset, n, names, kinds, end)
    if lines is not None and lines < n:
        raise ValueError(f"{path}: header says {n} atoms but only {lines} body lines present")
    if classical:
        xyz = np.column_stack([_host(cols[c]) for c in "xyz"])
        lo = xyz.min(axis=0) if n else np.zeros(3)
        extent = (xyz.max(axis=0) - lo) if n else np.zeros(3)
        cell, origin = np.diag(np.where(extent > 0, extent, 1e-9)), lo
    else:
        cell = np.array(info["lattice"].split(), dtype=np.float64).reshape(3, 3)
    for key in ("pbc", "properties", "origin", "lattice"):
        info.pop(key, None)
    return _frame(cols), Box(cell, boundary, origin), info


def read_xyz(path) -> Tuple[Frame, Box, Dict[str, Any]]:
    path = str(path)
    head, offset = _header(path, 2)
    return _xyz_frame(path, head, offset)


# ---------------------------------------------------------------------------------------------------------------------
# LAMMPS data file (atom_style atomic / charge)
# ---------------------------------------------------------------------------------------------------------------------
# The reference (src/mdapy/load_save.py:1036-1323) slurps the file into a list of lines, finds the sections by their first
# token, and joins the Velocities rows to the Atoms rows through a dict.  Here one body (`_data_frame`) decides sections, header,
# style and errors over a text that is either the file's bytes on the host (`_HostText`) or the file streamed once into HBM
# (`_DeviceText`): there the section lines are found by one pass of ``mdh_scan_sections``, both tables are tokenised where they
# lie (views of the one text tensor), the join is ``mdh_match_ids`` + gathers, and the host copies down only what it reads as
# text — the header, the section lines, the first data row, the Masses rows.
_SECTION_WORDS = ("Atoms", "Velocities", "Masses", "Bonds", "Angles", "Dihedrals", "Impropers", "Bond", "Angle", "Dihedral", "Improper",
                  "Pair", "PairIJ", "Ellipsoids", "Lines", "Triangles", "Bodies", "Atom")  # load_save.py:1067-1076
_FORBIDDEN_HINTS = ("bond", "angle", "dihedral", "improper", "molecular", "ellipsoid")
_SECTION_LINE = re.compile(rb"^[ \t\r]*(" + b"|".join(w.encode() for w in sorted(_SECTION_WORDS, key=len, reverse=True)) + rb")(?=[ \t\r\n]|\Z)", re.M)
DATA_HEADER_MAX = 1 << 20  # an Atoms section that starts beyond this (a huge preamble, Velocities first) sends the file to the host reader
# The tables of a data file start anywhere in the text tensor, and the tokenizer's line count takes its 16-byte loads only
# from aligned addresses (byte loads otherwise).  True: a table that starts at an unaligned address is copied to an allocation
# of its own first; False: it is parsed as a view.  Measured on an MI355X with 10 061 824 rows ``id type x y z`` (546 MB) that
# start 5 bytes past a 16-byte boundary (profiles/data_reader.md): 3.30 ms as a view, 0.35 + 2.62 ms copied — the copy wins.
DATA_ALIGN_TABLES = True
_PEEK = 1 << 16


class _ToHost(Exception):
    """the device path hands the file to the host reader (which also words every error)"""


class _HostText:
    """the whole file as bytes; section lines by a loop over the lines (a multi-line regular expression)"""

    def __init__(self, path):
        with _open(path) as f:
            self.body = f.read()
        self.nbytes = len(self.body)

    def sections(self):
        out: Dict[str, int] = {}
        for m in _SECTION_LINE.finditer(self.body):
            out.setdefault(m.group(1).decode(), m.start())
        return out

    def read(self, a: int, b: int) -> bytes:
        return self.body[a:b]

    def lines_from(self, a: int) -> int:
        tail = self.nbytes - a
        return 0 if tail <= 0 else self.body.count(b"\n", a) + (0 if self.body.endswith(b"\n") else 1)

    def table(self, a: int, b: int, nrows: int, names, kinds, source):
        return _table_on_host(self.body[a:b], nrows, names, kinds, source)

    def join(self, ids, vel_ids, vel):
        rows = dict(zip(_host(vel_ids).tolist(), range(len(vel_ids))))  # (of two rows with one id the last wins)
        order = np.array([rows[a] for a in _host(ids).tolist()], dtype=np.int64)  # KeyError(id): an atom without a row
        return [np.ascontiguousarray(_host(v)[order]) for v in vel]


class _DeviceText:
    """the whole file in HBM; section lines by mdh_scan_sections"""

    def __init__(self, path):
        from . import _text

        with _open(path) as f:
            self.text, self.nbytes = _text.stream_to_device(f, None if path.endswith(".gz") else os.path.getsize(path))

    def sections(self):
        from . import _text

        found, self.nlines = _text.scan_sections(self.text, _SECTION_WORDS)
        if found.get("Atoms", 0) > DATA_HEADER_MAX:
            raise _ToHost
        return found

    def read(self, a: int, b: int) -> bytes:
        return self.text[a:b].cpu().numpy().tobytes()

    def lines_from(self, a: int) -> int:
        raise _ToHost  # (asked only where a table came up short: the host reader counts, and words the error)

    def table(self, a: int, b: int, nrows: int, names, kinds, source):
        from . import _text

        view = self.text[a:b]
        if DATA_ALIGN_TABLES and int(view.data_ptr()) % 16:
            view = view.clone()
        try:
            cols, _ = _text.parse_table(view, nrows, kinds)
        except (ValueError, _text.RedoOverflow):  # rows missing or short, a field that is no number; more fields than the hand-back list holds
            raise _ToHost from None
        return dict(zip(names, cols))

    def join(self, ids, vel_ids, vel):
        from . import kernels

        row_of, misses, first, moved = kernels.order.match_ids(ids, vel_ids)
        if misses:
            raise KeyError(int(ids.dev()[first]))
        return list(vel) if moved == 0 else [kernels.order.permute(v, row_of) for v in vel]


def _first_data(src, at: int):
    """the section whose header line starts at byte ``at``: (that line, offset of its first data line — the first one after it
    that is neither blank nor a comment —, that line), or (header line, None, None)"""
    got, upto, header, pos = b"", at, None, at
    while True:
        if upto < src.nbytes:
            step = max(_PEEK, len(got))
            got += src.read(upto, min(src.nbytes, upto + step))
            upto = at + len(got)
        done = upto >= src.nbytes
        while True:
            nl = got.find(b"\n", pos - at)
            if nl < 0 and not done:
                break  # (the line is not complete yet: read on)
            end = nl if nl >= 0 else len(got)
            if pos - at >= len(got):
                return header, None, None
            line = got[pos - at:end].decode()
            if header is None:
                header = line
            elif line.strip() and not line.strip().startswith("#"):
                return header, pos, line
            pos = at + end + 1
        if done:
            return header, None, None


def _lines_at(src, at: int, n: int) -> List[str]:
    """up to ``n`` lines from byte ``at`` on"""
    got, upto = b"", at
    while upto < src.nbytes and got.count(b"\n") < n:
        step = max(_PEEK, len(got))
        got += src.read(upto, min(src.nbytes, upto + step))
        upto = at + len(got)
    return got.decode().split("\n")[:n] if got else []


def _masses_to_elements(lines: List[str], n_types: int) -> Optional[Dict[int, str]]:
    """rows ``type mass # Element`` -> {type: element} when n_types rows carry such a comment, else None (load_save.py:276-309)"""
    mapping: Dict[int, str] = {}
    parsed = 0
    for raw in lines:
        line = raw.strip()
        if not line or line.startswith("#") or "#" not in line:
            continue
        head, comment = line.split("#", 1)
        fields, words = head.split(), comment.split()
        if len(fields) < 2 or not words:
            continue
        try:
            kind = int(fields[0])
        except ValueError:
            continue
        mapping[kind] = words[0]
        parsed += 1
        if parsed >= n_types:
            break
    return mapping if parsed == n_types else None


def _element_column(types, mapping: Dict[int, str], path: str) -> np.ndarray:
    """names indexed by type, on the host (as the dump reader builds its string columns)"""
    host = _host(types)
    if not host.size:
        return np.empty(0, dtype=object)
    lo, hi = int(host.min()), int(host.max())
    if hi - lo >= (1 << 24):  # (type numbers far apart: no table indexed by type)
        for kind in np.unique(host).tolist():
            if kind not in mapping:
                raise ValueError(f"{path}: atom type {kind} has no element in the Masses section")
        return np.array([mapping[k] for k in host.tolist()], dtype=object)
    index = host.astype(np.intp) - lo
    names = np.empty(hi - lo + 1, dtype=object)
    for kind in (np.flatnonzero(np.bincount(index)) + lo).tolist():
        if kind not in mapping:
            raise ValueError(f"{path}: atom type {kind} has no element in the Masses section")
        names[kind - lo] = mapping[kind]
    return names.take(index)


def _data_frame(src, path: str):
    found = src.sections()
    if "Atoms" not in found:
        raise ValueError(f"{path}: no 'Atoms' section found")
    marks = sorted(set(found.values()))

    def section_end(at: int) -> int:  # the next section line after byte `at` that is known of, else the end of the text
        return next((m for m in marks if m > at), src.nbytes)

    # ---- header: every line before `Atoms` (load_save.py:1097-1143)
    n = n_types = 0
    lo, hi, tilt = [0.0, 0.0, 0.0], [0.0, 0.0, 0.0], [0.0, 0.0, 0.0]
    for raw in src.read(0, found["Atoms"]).decode().split("\n"):
        tokens = raw.split()
        if not tokens:
            continue
        tail = tokens[-1]
        try:
            if tail == "atoms":
                n = int(tokens[0])
            elif tail == "types" and len(tokens) >= 2 and tokens[1] == "atom":
                n_types = int(tokens[0])
            elif tail in ("xhi", "yhi", "zhi"):
                k = "xyz".index(tail[0])
                lo[k], hi[k] = float(tokens[0]), float(tokens[1])  # (both converted before either is kept)
            elif tail == "yz":
                tilt = [float(tokens[0]), float(tokens[1]), float(tokens[2])]
        except (IndexError, ValueError):  # a line of the wrong shape is skipped: `Atoms` is the anchor
            pass
        if len(tokens) >= 2 and any(h in tokens[1].lower() for h in _FORBIDDEN_HINTS):
            raise NotImplementedError(f"{path}: only atom_style atomic / charge are supported (found header keyword '{tokens[1]}')")
    box = np.array([[hi[0] - lo[0], 0, 0], [tilt[0], hi[1] - lo[1], 0], [tilt[1], tilt[2], hi[2] - lo[2]], [lo[0], lo[1], lo[2]]], dtype=np.float64)

    # ---- the Atoms section: style from its comment or from the fields of its first row (load_save.py:1157-1217)
    header, first, row = _first_data(src, found["Atoms"])
    hint = None
    if "#" in header:
        words = header.split("#", 1)[1].split()
        hint = words[0].lower() if words else None
    if hint and hint not in ("atomic", "charge"):
        raise NotImplementedError(f"{path}: atom_style '{hint}' not supported (only atomic / charge)")
    if first is None:
        raise ValueError(f"{path}: 'Atoms' section is empty")
    n_cols = len(row.split())
    if hint is None:
        if n_cols in (5, 8):
            style = "atomic"
        elif n_cols in (6, 9):
            style = "charge"
        else:
            raise NotImplementedError(f"{path}: cannot infer atom_style from {n_cols}-column Atoms data (only atomic / charge are supported)")
    else:
        valid = (5, 8) if hint == "atomic" else (6, 9)
        if n_cols not in valid:
            raise ValueError(f"{path}: atom_style {hint!r} expects {valid} columns, got {n_cols}")
        style = hint
    names = ["id", "type", "x", "y", "z"] if style == "atomic" else ["id", "type", "q", "x", "y", "z"]
    if n_cols == len(names) + 3:
        names += ["ix", "iy", "iz"]
    kinds = [INT if c in ("id", "type", "ix", "iy", "iz") else FLOAT for c in names]

    # ---- the table: the next N lines
    end = section_end(first)
    if n > 0:
        try:
            cols = src.table(first, end, n, names, kinds, path)
        except ValueError:
            present = src.lines_from(first)
            if present < n:
                raise ValueError(f"{path}: expected {n} atom rows, found {present}") from None
            raise
    else:
        cols = {c: np.empty(0, dtype=np.int32 if k == INT else np.float64) for c, k in zip(names, kinds)}

    # ---- Velocities: joined by id when N lines follow its first data line, ignored otherwise (load_save.py:1267-1300)
    if "Velocities" in found and n > 0:
        _, vfirst, _ = _first_data(src, found["Velocities"])
        vel = None
        if vfirst is not None:
            vnames = ["id", "vx", "vy", "vz"]
            try:
                vel = src.table(vfirst, section_end(vfirst), n, vnames, [INT, FLOAT, FLOAT, FLOAT], path)
            except ValueError:
                if src.lines_from(vfirst) >= n:
                    raise
        if vel is not None:
            cols["vx"], cols["vy"], cols["vz"] = src.join(cols["id"], vel["id"], [vel["vx"], vel["vy"], vel["vz"]])

    # ---- Masses: an `element` column when every type's row names one (load_save.py:1307-1321)
    if "Masses" in found and n_types > 0:
        _, mfirst, _ = _first_data(src, found["Masses"])
        mapping = _masses_to_elements(_lines_at(src, mfirst, n_types), n_types) if mfirst is not None else None
        if mapping is not None:
            cols["element"] = _element_column(cols["type"], mapping, path)
    return Frame(cols), Box(box[:3], [1, 1, 1], box[3]), {}


def read_data(path) -> Tuple[Frame, Box, Dict[str, Any]]:
    """a single-frame LAMMPS data file of atom_style atomic or charge (load_save.py:1036-1323): columns ``id type [q] x y z
    [ix iy iz] [vx vy vz] [element]``"""
    path = str(path)
    if have_gpu() and (path.endswith(".gz") or os.path.getsize(path) >= DEVICE_MIN_BYTES):
        try:
            return _data_frame(_DeviceText(path), path)
        except _ToHost:
            pass
    return _data_frame(_HostText(path), path)


# ---------------------------------------------------------------------------------------------------------------------
# .mp (parquet with the box in the key-value metadata)
# ---------------------------------------------------------------------------------------------------------------------
def read_mp(path) -> Tuple[Frame, Box, Dict[str, Any]]:
    try:
        import pyarrow.parquet as pq
    except ImportError as e:  # pragma: no cover
        raise ImportError("reading .mp files needs pyarrow") from e
    table = pq.read_table(str(path))
    meta = {k.decode(): v.decode() for k, v in (table.schema.metadata or {}).items()}
    cols: Dict[str, Any] = {}
    for name in table.column_names:
        col = table.column(name)
        a = col.to_numpy(zero_copy_only=False) if hasattr(col, "to_numpy") else np.asarray(col)
        cols[name] = a.astype(object) if a.dtype.kind in "OUS" else np.ascontiguousarray(a)
    if not {"x", "y", "z"} <= set(cols):
        raise ValueError(f"{path}: an .mp file must hold x, y and z columns")
    if "box" in meta:
        cell = np.array(meta["box"].split(), dtype=np.float64).reshape(3, 3)
    else:  # no stored box: the bounding box of the atoms, zero extents padded (load_save.py:627-634)
        xyz = np.column_stack([cols[c] for c in "xyz"]).astype(np.float64)
        extent = xyz.max(axis=0) - xyz.min(axis=0)
        cell = np.diag(np.where(extent > 0, extent, 1e-9))
    origin = np.array(meta["origin"].split(), dtype=np.float64) if "origin" in meta else None
    boundary = np.array(meta["boundary"].split(), dtype=np.int32) if "boundary" in meta else None
    info = {k: v for k, v in meta.items() if k not in ("box", "origin", "boundary") and not k.startswith("ARROW") and k != "pandas"}
    return _frame(cols), Box(cell, boundary, origin), info


def write_mp(path, frame: Frame, box: Box, info: Optional[Dict[str, Any]] = None) -> None:
    """the reference's ``.mp`` layout (load_save.py:1534-1560): one parquet table, box / origin / boundary as strings"""
    import pyarrow as pa
    import pyarrow.parquet as pq

    arrays = {k: (frame[k].to_numpy().astype(str) if frame[k].dtype == object else frame[k].to_numpy()) for k in frame.columns}
    meta = {"box": " ".join(repr(float(v)) for v in np.asarray(box.box).ravel()),
            "origin": " ".join(repr(float(v)) for v in box.origin), "boundary": " ".join(str(int(v)) for v in box.boundary)}
    meta.update({k: str(v) for k, v in (info or {}).items()})
    pq.write_table(pa.table(arrays).replace_schema_metadata(meta), str(path))


# ---------------------------------------------------------------------------------------------------------------------
# the output side: LAMMPS dump and data, (extended) XYZ, POSCAR
# ---------------------------------------------------------------------------------------------------------------------
# The reference's writers (src/mdapy/load_save.py:1565-2017) print a few header lines and hand the atom table to a CSV writer
# (separator " ", no header, float_precision=10).  Here the header is written on the host in the reference's wording, and the
# table is formatted where its columns are: in HBM (``_text.format_chunks`` / csrc/text_format.hip), streamed to the file
# through pinned buffers while the next piece is formatted — or, below DEVICE_MIN_ROWS rows and on a machine without a GPU, by
# the host formatter (the same bytes; I/O plumbing, not a compute fallback).
# Tables with fewer rows are formatted on the host.  Measured on an MI355X with six columns on the host (profiles/text_format.md):
# the device path costs 3.7-4.0 ms up to 65 536 rows (uploads, three launches, two synchronisations, the pinned buffers), the
# host formatter 0.56 us a row — 2.3 ms at 4 096 rows, 9.2 ms at 16 384: they cross near 6 800 rows.
DEVICE_MIN_ROWS = 1 << 13


def _num(v) -> str:
    """a header number as the reference's f-strings print a numpy float64"""
    return str(np.float64(v))


def _in_hbm(col) -> bool:
    return col._host_arr is None and col._dev is not None


def _column_spec(col, device: bool):
    """(array, kind, names) of one frame column for the table formatters; the array in HBM (``device``) or numpy"""
    from . import _text
    from .devarray import HArray

    kind = np.dtype(col.dtype).kind
    if kind in "OUS":
        from . import policy

        names, codes = policy.label_codes(col.to_numpy())
        return codes, _text.CODED, _text.check_names(names)
    if kind not in "iuf":
        raise ValueError(f"column {col.name!r} of dtype {col.dtype} cannot be written to a text table")
    native = {np.dtype(np.float64): _text.F64, np.dtype(np.float32): _text.F32, np.dtype(np.int32): _text.I32, np.dtype(np.int64): _text.I64}
    dtype = np.dtype(col.dtype)
    if dtype in native:
        return (col.device_array() if device else col.to_numpy()), native[dtype], None
    host = col.to_numpy()
    if not device:
        return host, (_text.F64 if kind == "f" else _text.I64), None
    if kind == "f":
        host, code = host.astype(np.float32), _text.F32  # (float16: every value is a float32)
    elif dtype.itemsize < 4:
        host, code = host.astype(np.int32), _text.I32
    else:
        if dtype == np.uint64 and host.size and host.max() >= 2 ** 63:
            raise _text.Unformattable(int((host >= 2 ** 63).sum()))
        host, code = host.astype(np.int64), _text.I64
    return HArray.from_numpy(host), code, None


def _rewindable(op) -> bool:
    return type(op) in (io.BufferedWriter, io.BufferedRandom, io.FileIO, io.BytesIO)


def _write_table(op, columns, rows=None) -> None:
    """the rows of ``columns`` (frame Columns of equal length) as text into the binary file object ``op``"""
    import tempfile

    from . import _text

    n = len(columns[0])
    if n and have_gpu() and n >= DEVICE_MIN_ROWS:
        try:
            specs = [_column_spec(c, True) for c in columns]
            pieces = _text.format_chunks([s[0] for s in specs], [s[1] for s in specs], [s[2] for s in specs], rows)
            if _rewindable(op):
                start = op.tell()
                try:
                    _text.stream_from_device(pieces, op)
                except _text.Unformattable:
                    op.seek(start)
                    op.truncate()
                    raise
            else:  # (a handle that cannot take its bytes back — a gzip stream —: the text goes through a scratch file)
                import shutil

                with tempfile.TemporaryFile() as scratch:
                    _text.stream_from_device(pieces, scratch)
                    scratch.seek(0)
                    shutil.copyfileobj(scratch, op, 1 << 24)
            return
        except _text.Unformattable:  # the device met a field it does not format: the whole table goes to the host formatter
            pass
    host_specs = [_column_spec(c, False) for c in columns]
    if n:
        _text.format_table_host([s[0] for s in host_specs], [s[1] for s in host_specs], [s[2] for s in host_specs], op)


def _moved(frame: Frame, origin, matrix):
    """columns x, y, z of ``frame`` minus ``origin`` and (``matrix`` given) times it: in HBM when they live there or the table is
    going to be formatted there, on the host otherwise — the same bits either way"""
    from . import _text
    from .frame import Column

    cols = [frame[c] for c in "xyz"]
    n = len(cols[0])
    device = have_gpu() and n and (all(_in_hbm(c) for c in cols) or n >= DEVICE_MIN_ROWS) and all(c.dtype == np.float64 for c in cols)
    arrays = [c.device_array() for c in cols] if device else [np.asarray(c.to_numpy(), dtype=np.float64) for c in cols]
    return [Column(name, a) for name, a in zip("xyz", _text.shift_rotate(*arrays, origin, matrix))]


def _with_id(frame: Frame) -> Frame:
    """``id`` = 1 .. N as the first column when the frame has none (the reference's ``with_row_index("id", offset=1)``)"""
    if "id" in frame.columns:
        return frame
    n = frame.shape[0]
    if have_gpu() and n >= DEVICE_MIN_ROWS:
        from .devarray import HArray, torch

        ids = HArray(torch().arange(1, n + 1, dtype=torch().int32 if n < 2 ** 31 else torch().int64, device="cuda"))
    else:
        ids = np.arange(1, n + 1, dtype=np.int32 if n < 2 ** 31 else np.int64)
    cols = {"id": ids}
    cols.update({k: frame[k] for k in frame.columns})
    return Frame(cols)


def _lammps_axes(frame: Frame, box: Box):
    """a cell with a component above its diagonal is rotated into LAMMPS' axes (a along x, b in the xy plane), the positions with
    it, and the origin moves to zero (load_save.py:1797-1811, 1964-1975)"""
    m = box.box
    if m[0, 1] != 0 or m[0, 2] != 0 or m[1, 2] != 0:
        box, rotate = box.align_to_lammps_box()
        x, y, z = _moved(frame, box.origin, rotate)
        box.origin[:] = 0
        frame = frame.with_columns(x=x, y=y, z=z)
    return frame, box


def _save(write, path, compress: bool, **kwargs) -> None:
    """``write(file object, **kwargs)`` into ``path``, or gzipped into ``path`` (+ ``.gz`` when the name lacks it)"""
    path = str(path)
    if not compress:
        with open(path, "wb") as op:
            write(op, **kwargs)
        return
    with gzip.open(path if path.endswith(".gz") else path + ".gz", "wb") as op:
        write(op, **kwargs)


def _need(frame, names):
    if not isinstance(frame, Frame):
        raise TypeError("data must be a Frame")
    for col in names:
        if col not in frame.columns:
            raise ValueError(f"data must contain {col} column")


def write_dump_frame_to(op, box: Box, frame: Frame, timestep=0.0, rows=None) -> None:
    """one LAMMPS dump frame into the open binary file ``op`` (load_save.py:1954-2017): ``write_dump`` writes one, a
    ``Trajectory`` one after another"""
    frame = _with_id(frame)
    frame, box = _lammps_axes(frame, box)
    keep = [c for c in frame.columns if np.dtype(frame[c].dtype).kind in "iuf" or c == "element"]  # numeric columns + `element`
    frame = frame.select(keep)
    bound = ["pp" if i == 1 else "ss" for i in box.boundary]
    op.write(f"ITEM: TIMESTEP\n{timestep}\n".encode())
    op.write(f"ITEM: NUMBER OF ATOMS\n{frame.shape[0]}\n".encode())
    xlo, ylo, zlo = (np.float64(v) for v in box.origin)
    xhi, yhi, zhi = xlo + box.box[0, 0], ylo + box.box[1, 1], zlo + box.box[2, 2]
    xy, xz, yz = box.box[1, 0], box.box[2, 0], box.box[2, 1]
    if xy != 0 or xz != 0 or yz != 0:
        xlo_bound, xhi_bound = xlo + min(0.0, xy, xz, xy + xz), xhi + max(0.0, xy, xz, xy + xz)
        ylo_bound, yhi_bound = ylo + min(0.0, yz), yhi + max(0.0, yz)
        op.write(f"ITEM: BOX BOUNDS xy xz yz {bound[0]} {bound[1]} {bound[2]}\n".encode())
        op.write(f"{_num(xlo_bound)} {_num(xhi_bound)} {_num(xy)}\n".encode())
        op.write(f"{_num(ylo_bound)} {_num(yhi_bound)} {_num(xz)}\n".encode())
        op.write(f"{_num(zlo)} {_num(zhi)} {_num(yz)}\n".encode())
    else:
        op.write(f"ITEM: BOX BOUNDS {bound[0]} {bound[1]} {bound[2]}\n".encode())
        op.write(f"{_num(xlo)} {_num(xhi)}\n{_num(ylo)} {_num(yhi)}\n{_num(zlo)} {_num(zhi)}\n".encode())
    op.write(("ITEM: ATOMS " + " ".join(frame.columns) + " \n").encode())
    _write_table(op, [frame[c] for c in frame.columns], rows)


def write_dump(path, frame: Frame, box: Box, timestep=0.0, compress: bool = False, rows=None) -> None:
    """a single-frame LAMMPS dump file (load_save.py:1910-1952).  ``rows``: rows formatted per piece on the device path."""
    _need(frame, ["type", "x", "y", "z"])
    _save(write_dump_frame_to, path, compress, box=box, frame=frame, timestep=timestep, rows=rows)


_XYZ_TRIPLES = [(("x", "y", "z"), "pos"), (("xu", "yu", "zu"), "unwrapped_position"), (("vx", "vy", "vz"), "vel"), (("fx", "fy", "fz"), "forces")]


def _xyz_type(dtype) -> str:
    kind = np.dtype(dtype).kind
    if kind in "iu":
        return "I"
    if kind == "f":
        return "R"
    if kind in "OUS":
        return "S"
    raise ValueError(f"Unrecognised dtype {dtype} in extended XYZ output")


def _xyz_properties(columns: List[str], dtypes) -> str:
    """the ``Properties=`` token (the rules of load_save.py:201-273): a run x y z / xu yu zu / vx vy vz / fx fy fz of floats folds
    into pos / unwrapped_position / vel / forces ``:R:3``, ``element`` is ``species``, a run ``base_0 base_1 ...`` of one dtype
    folds into ``base:T:n``, everything else is ``name:T:1``"""
    tokens, i = [], 0
    while i < len(columns):
        for triple, alias in _XYZ_TRIPLES:
            if tuple(columns[i:i + 3]) == triple and all(_xyz_type(dtypes[i + j]) == "R" for j in range(3)):
                tokens.append(f"{alias}:R:3")
                i += 3
                break
        else:
            cur = columns[i]
            if cur == "element":
                tokens.append(f"species:{_xyz_type(dtypes[i])}:1")
                i += 1
                continue
            base, sep, idx = cur.rpartition("_")
            run = 1
            if sep and base and idx.isdigit() and int(idx) == 0:
                while i + run < len(columns):
                    nb, ns, ni = columns[i + run].rpartition("_")
                    if not ns or nb != base or not ni.isdigit() or int(ni) != run or np.dtype(dtypes[i + run]) != np.dtype(dtypes[i]):
                        break
                    run += 1
            if run >= 2:
                tokens.append(f"{base}:{_xyz_type(dtypes[i])}:{run}")
                i += run
            else:
                tokens.append(f"{cur}:{_xyz_type(dtypes[i])}:1")
                i += 1
    return "Properties=" + ":".join(tokens)


def _write_xyz_to(op, box: Box, frame: Frame, classical: bool, rows=None, **kargs) -> None:
    if classical:
        op.write(f"{frame.shape[0]}\n".encode())
        op.write("Classical XYZ file written by mdapy.\n".encode())
        _write_table(op, [frame[c] for c in ("element", "x", "y", "z")], rows)
        return
    properties = _xyz_properties(frame.columns, [frame[c].dtype for c in frame.columns])
    comments = ('Lattice="' + " ".join(_num(v) for v in box.box.flatten()) + '" ' + properties
                + ' pbc="' + " ".join("T" if i == 1 else "F" for i in box.boundary) + '"'
                + ' Origin="' + " ".join(_num(v) for v in box.origin) + '"')
    for key, value in kargs.items():
        if key.lower() not in ("lattice", "pbc", "properties", "origin"):
            comments += f' {key}="{value}"' if key.lower() in ("virial", "bec", "stress") else f" {key}={value}"
    op.write(f"{frame.shape[0]}\n".encode())
    op.write(f"{comments}\n".encode())
    _write_table(op, [frame[c] for c in frame.columns], rows)


def write_xyz(path, frame: Frame, box: Box, classical: bool = False, compress: bool = False, rows=None, **kargs) -> None:
    """an XYZ file (load_save.py:1565-1652): extended — Lattice, Properties, pbc, Origin and the extra keys in the comment line,
    every column in the table — or ``classical``: ``element x y z`` alone"""
    _need(frame, ["x", "y", "z", "element"])
    _save(_write_xyz_to, path, compress, box=box, frame=frame, classical=classical, rows=rows, **kargs)


def _write_poscar_to(op, box: Box, frame: Frame, reduced_pos: bool, selective_dynamics: bool, rows=None) -> None:
    from . import _text, policy
    from .frame import PermutedColumn

    if selective_dynamics:
        for col in ("sdx", "sdy", "sdz"):
            if col not in frame.columns:
                raise ValueError(f"data must contain {col} if selective_dynamics=True")
    names, codes = policy.label_codes(frame["element"].to_numpy())
    names, codes = _text.check_names(names), np.asarray(codes)  # (the names go into the header line, blank-separated)
    order = np.argsort(codes, kind="stable")  # by element; atoms of one element keep their order
    counts = np.bincount(codes, minlength=len(names))
    x, y, z = _moved(frame, box.origin, box.inverse_box if reduced_pos else None)
    table = [x, y, z] + ([frame[c] for c in ("sdx", "sdy", "sdz")] if selective_dynamics else [])
    perm = order.astype(np.int32)
    if any(_in_hbm(c) for c in table):  # (columns in HBM are gathered there: frame.PermutedColumn)
        from .devarray import HArray

        perm = HArray.from_numpy(perm)
    table = [PermutedColumn(c, perm) for c in table]
    op.write("# VASP POSCAR file written by mdapy.\n".encode())
    op.write("1.0000000000\n".encode())
    for k in range(3):
        op.write("{:.10f} {:.10f} {:.10f}\n".format(*(float(v) for v in box.box[k])).encode())
    op.write(("".join(f"{name} " for name in names) + "\n").encode())
    op.write(("".join(f"{int(c)} " for c in counts) + "\n").encode())
    if selective_dynamics:
        op.write("Selective dynamics\n".encode())
    op.write(("Direct\n" if reduced_pos else "Cartesian\n").encode())
    _write_table(op, table, rows)


def write_poscar(path, frame: Frame, box: Box, reduced_pos: bool = False, selective_dynamics: bool = False, compress: bool = False,
                 rows=None) -> None:
    """a VASP POSCAR file (load_save.py:1654-1752): atoms grouped by element (a STABLE sort: atoms of one element keep their
    order, which the reference leaves open), positions minus the origin, Cartesian or reduced"""
    _need(frame, ["element", "x", "y", "z"])
    _save(_write_poscar_to, path, compress, box=box, frame=frame, reduced_pos=reduced_pos, selective_dynamics=selective_dynamics, rows=rows)


def _write_data_to(op, box: Box, frame: Frame, element_list, num_type, data_format: str, rows=None) -> None:
    from .atomic_temperature import STANDARD_ATOMIC_WEIGHT

    frame = _with_id(frame)
    frame, box = _lammps_axes(frame, box)
    if data_format not in ["atomic", "charge"]:
        raise ValueError(f"Unrecognized data format: {data_format}. Only support atomic and charge")
    types = frame["type"]
    type_max = int(types.device_array().max() if _in_hbm(types) else types.to_numpy().max())
    if num_type is None:
        num_type = type_max
    elif num_type < type_max:
        raise ValueError(f"num_type ({num_type}) is less than the largest type in data ({type_max})")
    if element_list is not None:
        if len(element_list) < num_type:
            raise ValueError(f"element_list has {len(element_list)} entries but num_type is {num_type}; need at least {num_type}")
        if len(element_list) > num_type:
            import warnings

            warnings.warn(f"element_list has {len(element_list)} entries but num_type={num_type}; writing only the first {num_type} elements.",
                          stacklevel=2)
            element_list = list(element_list)[:num_type]
        for name in element_list:
            if name not in STANDARD_ATOMIC_WEIGHT:
                raise ValueError(f"Unrecognized element name {name}")
    op.write("# LAMMPS data file written by mdapy.\n\n".encode())
    op.write(f"{frame.shape[0]} atoms\n{num_type} atom types\n\n".encode())
    origin = [np.float64(v) for v in box.origin]
    for k, axis in enumerate("xyz"):
        op.write(f"{_num(origin[k])} {_num(origin[k] + box.box[k, k])} {axis}lo {axis}hi\n".encode())
    xy, xz, yz = box.box[1, 0], box.box[2, 0], box.box[2, 1]
    if xy != 0 or xz != 0 or yz != 0:
        op.write(f"{_num(xy)} {_num(xz)} {_num(yz)} xy xz yz\n".encode())
    op.write("\n".encode())
    if element_list is not None:
        op.write("Masses\n\n".encode())
        for k, name in enumerate(element_list, start=1):
            op.write(f"{k} {_num(STANDARD_ATOMIC_WEIGHT[name])} # {name}\n".encode())
        op.write("\n".encode())
    op.write(f"Atoms # {data_format}\n\n".encode())
    if data_format == "charge" and "q" not in frame.columns:
        n = frame.shape[0]
        if have_gpu() and n >= DEVICE_MIN_ROWS:
            from .devarray import HArray

            frame = frame.with_columns(q=HArray.full((n,), 0.0, np.float64))
        else:
            frame = frame.with_columns(q=np.zeros(n, np.float64))
    wanted = ["id", "type", "x", "y", "z"] if data_format == "atomic" else ["id", "type", "q", "x", "y", "z"]
    _write_table(op, [frame[c] for c in wanted], rows)
    if all(c in frame.columns for c in ("vx", "vy", "vz")):
        op.write("\nVelocities\n\n".encode())
        _write_table(op, [frame[c] for c in ("id", "vx", "vy", "vz")], rows)


def write_data(path, frame: Frame, box: Box, element_list=None, num_type=None, data_format: str = "atomic", compress: bool = False,
               rows=None) -> None:
    """a LAMMPS data file (load_save.py:1754-1908): header, optional Masses block, ``Atoms # atomic`` (id type x y z) or
    ``# charge`` (id type q x y z, q = 0.0 when the frame has none), and a Velocities section when vx vy vz are there"""
    _need(frame, ["type", "x", "y", "z"])
    _save(_write_data_to, path, compress, box=box, frame=frame, element_list=element_list, num_type=num_type, data_format=data_format, rows=rows)


def read_file(path: str, fmt: Optional[str] = None):
    p = str(path)
    if fmt is None:
        base = p[:-3] if p.endswith(".gz") else p
        fmt = base.rsplit(".", 1)[-1].lower()
    if fmt == "xyz":
        return read_xyz(p)
    if fmt in ("dump", "lammpstrj"):
        return read_dump(p)
    if fmt == "mp":
        return read_mp(p)
    if fmt in ("data", "lmp"):
        return read_data(p)
    raise ValueError(f"unsupported file format {fmt!r} (supported: xyz, dump, data, lmp, mp)")


class BuildSystem:
    """The reference's entry points for the input side (src/mdapy/load_save.py:356-1374) over this package's readers: the same
    names and return tuples ``(frame, box[, global_info])``.  Formats: LAMMPS dump and data, (ext)XYZ, ``.mp`` — the rows of
    SURVEY 8f.2; ``poscar`` files, which the reference also reads, are refused by name."""

    _SUPPORTED = ["data", "lmp", "dump", "poscar", "xyz", "mp"]

    @classmethod
    def from_file(cls, filename, format=None):
        if format is None:
            parts = os.path.basename(str(filename)).split(".")
            if parts[-1] == "gz":
                if len(parts) < 2:
                    raise ValueError("Cannot infer format from filename")
                format = parts[-2]
            else:
                format = parts[-1]
        format = format.lower()
        if format.endswith(".gz"):
            format = format[:-3]
        if format not in cls._SUPPORTED:
            raise ValueError(f"Format '{format}' not supported. Supported formats: {cls._SUPPORTED}")
        if format == "dump":
            return cls.read_dump(filename)
        if format == "xyz":
            return cls.read_xyz(filename)
        if format == "mp":
            return cls.read_mp(filename)
        if format in ("data", "lmp"):
            return cls.read_data(filename)
        raise ValueError(f"mdapy_amd reads dump, xyz and mp files; '{format}' files are outside its input side (SURVEY 8f.2)")

    @staticmethod
    def from_array(pos, box):
        if not isinstance(pos, np.ndarray):
            raise TypeError("pos must be numpy array")
        if pos.ndim != 2 or pos.shape[1] != 3:
            raise ValueError("pos must be N x 3 array")
        xyz = np.asarray(pos, dtype=np.float64)
        return Frame({"x": np.ascontiguousarray(xyz[:, 0]), "y": np.ascontiguousarray(xyz[:, 1]), "z": np.ascontiguousarray(xyz[:, 2])}), \
            (box if isinstance(box, Box) else Box(box))

    @staticmethod
    def from_data(data, box):
        frame = Frame.from_any(data)
        for name in ("x", "y", "z"):
            if name not in frame.columns:
                raise ValueError(f"Data must contain {name} column")
        frame = frame.with_columns(**{name: frame[name].to_numpy().astype(np.float64, copy=False) for name in ("x", "y", "z")})
        return frame, (box if isinstance(box, Box) else Box(box))

    read_dump = staticmethod(read_dump)
    read_xyz = staticmethod(read_xyz)
    read_mp = staticmethod(read_mp)
    read_data = staticmethod(read_data)
