"""A LAMMPS data file read the slow way — ``readlines``, ``str.split``, ``float()``, ``int()`` and a dict for the join of the
Velocities rows: a restatement, written for the tests, of what the reference's ``BuildSystem.read_data`` produces
(src/mdapy/load_save.py:1036-1323, 276-309).  The yardstick of test_data_reader_host.py and test_gpu_data_reader.py; it shares
nothing with mdapy_amd."""
import gzip

import numpy as np

WORDS = ["Atoms", "Velocities", "Masses", "Bonds", "Angles", "Dihedrals", "Impropers", "Bond", "Angle", "Dihedral", "Improper", "Pair",
         "PairIJ", "Ellipsoids", "Lines", "Triangles", "Bodies", "Atom"]
HINTS = ["bond", "angle", "dihedral", "improper", "molecular", "ellipsoid"]
INTS = ("id", "type", "ix", "iy", "iz")


def _is_data(line):
    s = line.strip()
    return bool(s) and not s.startswith("#")


def section_lines(lines):
    """{word: index of the first line whose first token is that word}"""
    out = {}
    for i, line in enumerate(lines):
        if _is_data(line):
            tok = line.split()[0]
            if tok in WORDS and tok not in out:
                out[tok] = i
    return out


def section_offsets(data: bytes):
    """the same in byte offsets of ``data``, and its number of lines"""
    lines = data.split(b"\n")
    if lines and lines[-1] == b"":
        lines.pop()
    starts, at = [], 0
    for ln in lines:
        starts.append(at)
        at += len(ln) + 1
    found = section_lines([ln.decode() for ln in lines])
    return {w: starts[i] for w, i in found.items()}, len(lines)


def _first_data(lines, header):
    i = header + 1
    while i < len(lines) and not _is_data(lines[i]):
        i += 1
    return i


def read_data(path, sample=None):
    """-> (columns: dict of numpy arrays in the reference's order, box 4 x 3 with the origin last, {}).  ``sample``: only
    these atom rows are converted (a big file: the join is still made over all velocity rows)."""
    opener = gzip.open if str(path).endswith(".gz") else open
    with opener(path, "rt") as f:
        lines = f.readlines()
    found = section_lines(lines)
    if "Atoms" not in found:
        raise ValueError(f"{path}: no 'Atoms' section found")
    n = ntypes = 0
    lo, hi, tilt = [0.0] * 3, [0.0] * 3, [0.0] * 3
    for line in lines[:found["Atoms"]]:
        t = line.split()
        if not t:
            continue
        try:
            if t[-1] == "atoms":
                n = int(t[0])
            elif t[-1] == "types" and len(t) >= 2 and t[1] == "atom":
                ntypes = int(t[0])
            elif t[-1] in ("xhi", "yhi", "zhi"):
                k = "xyz".index(t[-1][0])
                a, b = float(t[0]), float(t[1])
                lo[k], hi[k] = a, b
            elif t[-1] == "yz":
                tilt = [float(t[0]), float(t[1]), float(t[2])]
        except (IndexError, ValueError):
            pass
        if len(t) >= 2 and any(h in t[1].lower() for h in HINTS):
            raise NotImplementedError(f"{path}: only atom_style atomic / charge are supported (found header keyword '{t[1]}')")
    box = np.array([[hi[0] - lo[0], 0, 0], [tilt[0], hi[1] - lo[1], 0], [tilt[1], tilt[2], hi[2] - lo[2]], lo], dtype=np.float64)

    head = lines[found["Atoms"]]
    hint = None
    if "#" in head:
        after = head.split("#", 1)[1].split()
        hint = after[0].lower() if after else None
    if hint and hint not in ("atomic", "charge"):
        raise NotImplementedError(f"{path}: atom_style '{hint}' not supported (only atomic / charge)")
    first = _first_data(lines, found["Atoms"])
    if first >= len(lines):
        raise ValueError(f"{path}: 'Atoms' section is empty")
    ncols = len(lines[first].split())
    if hint is None:
        if ncols not in (5, 6, 8, 9):
            raise NotImplementedError(f"{path}: cannot infer atom_style from {ncols}-column Atoms data (only atomic / charge are supported)")
        style = "atomic" if ncols in (5, 8) else "charge"
    else:
        valid = (5, 8) if hint == "atomic" else (6, 9)
        if ncols not in valid:
            raise ValueError(f"{path}: atom_style {hint!r} expects {valid} columns, got {ncols}")
        style = hint
    names = ["id", "type", "x", "y", "z"] if style == "atomic" else ["id", "type", "q", "x", "y", "z"]
    if ncols == len(names) + 3:
        names += ["ix", "iy", "iz"]
    block = lines[first:first + n]
    if len(block) != n:
        raise ValueError(f"{path}: expected {n} atom rows, found {len(block)}")
    keep = range(n) if sample is None else sample
    rows = [block[i].split()[:len(names)] for i in keep]
    cols = {}
    for j, name in enumerate(names):
        if name in INTS:
            cols[name] = np.array([int(r[j]) for r in rows], dtype=np.int32)
        else:
            cols[name] = np.array([float(r[j]) for r in rows], dtype=np.float64)

    if "Velocities" in found:
        vfirst = _first_data(lines, found["Velocities"])
        vblock = lines[vfirst:vfirst + n]
        if len(vblock) == n:
            by_id = {}
            for row in vblock:
                t = row.split()
                by_id[int(t[0])] = (float(t[1]), float(t[2]), float(t[3]))
            joined = [by_id[int(a)] for a in cols["id"]]  # KeyError(id) for an atom without a row
            for k, name in enumerate(("vx", "vy", "vz")):
                cols[name] = np.array([v[k] for v in joined], dtype=np.float64)

    if "Masses" in found and ntypes > 0:
        mfirst = _first_data(lines, found["Masses"])
        mapping, parsed = {}, 0
        for line in lines[mfirst:mfirst + ntypes]:
            s = line.strip()
            if not s or s.startswith("#") or "#" not in s:
                continue
            left, right = s.split("#", 1)
            if len(left.split()) < 2 or not right.split():
                continue
            try:
                kind = int(left.split()[0])
            except ValueError:
                continue
            mapping[kind] = right.split()[0]
            parsed += 1
            if parsed >= ntypes:
                break
        if parsed == ntypes:
            for kind in cols["type"]:
                if int(kind) not in mapping:
                    raise ValueError(f"{path}: atom type {int(kind)} has no element in the Masses section")
            cols["element"] = np.array([mapping[int(kind)] for kind in cols["type"]], dtype=object)
    return cols, box, {}
