"""What the writers of ``mdapy_amd.load_save`` must produce, restated in the plainest Python: ``format(v, ".10f")`` for a float,
``str(int(v))`` for an integer, ``" ".join`` for a row, f-strings for the headers (the reference's wording,
src/mdapy/load_save.py:1565-2017).  The tests compare bytes with what these functions return.  Nothing here calls the library's
host formatter or its hooks.

Columns are an ordered dict ``name -> numpy array`` (object arrays for strings); ``box`` is a ``mdapy_amd.box.Box``."""
import math

import numpy as np

MASS = {"Al": 26.9815385, "Cu": 63.546, "Fe": 55.845, "Ni": 58.6934, "H": 1.008, "O": 15.999, "Zr": 91.224}


def field(v) -> str:
    if isinstance(v, str):
        return v
    if isinstance(v, (float, np.floating)):
        v = float(v)  # (exact for float32 and float16)
        if math.isnan(v):
            return "NaN"
        if math.isinf(v):
            return "inf" if v > 0 else "-inf"
        return format(v, ".10f")
    return str(int(v))


def table(columns) -> bytes:
    """rows of the given arrays: fields joined by one blank, every row ended by a line feed"""
    lists = [c.tolist() if c.dtype.kind in "iuO" else list(c) for c in columns]
    return "".join(" ".join(field(v) for v in row) + "\n" for row in zip(*lists)).encode()


def num(v) -> str:
    return str(np.float64(v))


def with_id(cols):
    if "id" in cols:
        return dict(cols)
    out = {"id": np.arange(1, len(cols["x"]) + 1)}
    out.update(cols)
    return out


def moved(cols, origin, matrix=None):
    """x, y, z minus the origin, then times the matrix: ((x - o0) m_0k + (y - o1) m_1k) + (z - o2) m_2k"""
    a, b, c = (np.asarray(cols[k], dtype=np.float64) - origin[j] for j, k in enumerate("xyz"))
    if matrix is None:
        return a, b, c
    return tuple((a * matrix[0, k] + b * matrix[1, k]) + c * matrix[2, k] for k in range(3))


def lammps_axes(cols, box):
    """(columns, 3x3 cell, origin, boundary) as a LAMMPS file states them: a cell with a component above the diagonal is rotated"""
    cell, origin = np.array(box.box), np.array(box.origin)
    if cell[0, 1] != 0 or cell[0, 2] != 0 or cell[1, 2] != 0:
        aligned, rotate = box.align_to_lammps_box()
        x, y, z = moved(cols, origin, rotate)
        cols = dict(cols, x=x, y=y, z=z)
        cell, origin = np.array(aligned.box), np.zeros(3)
    return cols, cell, origin, np.array(box.boundary)


def dump(cols, box, timestep=0.0) -> bytes:
    cols, cell, origin, boundary = lammps_axes(with_id(cols), box)
    cols = {k: v for k, v in cols.items() if v.dtype.kind in "iuf" or k == "element"}
    b = ["pp" if i == 1 else "ss" for i in boundary]
    n = len(cols["x"])
    head = f"ITEM: TIMESTEP\n{timestep}\nITEM: NUMBER OF ATOMS\n{n}\n"
    xlo, ylo, zlo = origin
    xhi, yhi, zhi = xlo + cell[0, 0], ylo + cell[1, 1], zlo + cell[2, 2]
    xy, xz, yz = cell[1, 0], cell[2, 0], cell[2, 1]
    if xy != 0 or xz != 0 or yz != 0:
        head += f"ITEM: BOX BOUNDS xy xz yz {b[0]} {b[1]} {b[2]}\n"
        head += f"{num(xlo + min(0.0, xy, xz, xy + xz))} {num(xhi + max(0.0, xy, xz, xy + xz))} {num(xy)}\n"
        head += f"{num(ylo + min(0.0, yz))} {num(yhi + max(0.0, yz))} {num(xz)}\n"
        head += f"{num(zlo)} {num(zhi)} {num(yz)}\n"
    else:
        head += f"ITEM: BOX BOUNDS {b[0]} {b[1]} {b[2]}\n{num(xlo)} {num(xhi)}\n{num(ylo)} {num(yhi)}\n{num(zlo)} {num(zhi)}\n"
    head += "ITEM: ATOMS " + " ".join(cols) + " \n"
    return head.encode() + table(list(cols.values()))


def xyz_type(a) -> str:
    return {"i": "I", "u": "I", "f": "R", "O": "S", "U": "S"}[a.dtype.kind]


def xyz_properties(cols) -> str:
    """for the frames the tests use: runs x y z -> pos, vx vy vz -> vel, fx fy fz -> forces, element -> species, base_0 base_1 ...
    of one dtype -> base:T:n, everything else name:T:1"""
    names, tokens, i = list(cols), [], 0
    alias = {("x", "y", "z"): "pos", ("xu", "yu", "zu"): "unwrapped_position", ("vx", "vy", "vz"): "vel", ("fx", "fy", "fz"): "forces"}
    while i < len(names):
        trio = tuple(names[i:i + 3])
        if trio in alias and all(xyz_type(cols[k]) == "R" for k in trio):
            tokens.append(f"{alias[trio]}:R:3")
            i += 3
        elif names[i] == "element":
            tokens.append("species:S:1")
            i += 1
        else:
            base, sep, idx = names[i].rpartition("_")
            run = 1
            if sep and base and idx == "0":
                while i + run < len(names) and names[i + run] == f"{base}_{run}" and cols[names[i + run]].dtype == cols[names[i]].dtype:
                    run += 1
            if run >= 2:
                tokens.append(f"{base}:{xyz_type(cols[names[i]])}:{run}")
            else:
                run = 1
                tokens.append(f"{names[i]}:{xyz_type(cols[names[i]])}:1")
            i += run
    return "Properties=" + ":".join(tokens)


def xyz(cols, box, classical=False, **extra) -> bytes:
    n = len(cols["x"])
    if classical:
        return f"{n}\nClassical XYZ file written by mdapy.\n".encode() + table([cols[k] for k in ("element", "x", "y", "z")])
    comment = 'Lattice="' + " ".join(num(v) for v in np.array(box.box).flatten()) + '" ' + xyz_properties(cols)
    comment += ' pbc="' + " ".join("T" if i == 1 else "F" for i in box.boundary) + '"'
    comment += ' Origin="' + " ".join(num(v) for v in box.origin) + '"'
    for key, value in extra.items():
        if key.lower() not in ("lattice", "pbc", "properties", "origin"):
            comment += f' {key}="{value}"' if key.lower() in ("virial", "bec", "stress") else f" {key}={value}"
    return f"{n}\n{comment}\n".encode() + table(list(cols.values()))


def data(cols, box, element_list=None, num_type=None, data_format="atomic") -> bytes:
    cols, cell, origin, _ = lammps_axes(with_id(cols), box)
    n = len(cols["x"])
    if num_type is None:
        num_type = int(cols["type"].max())
    head = f"# LAMMPS data file written by mdapy.\n\n{n} atoms\n{num_type} atom types\n\n"
    for k, axis in enumerate("xyz"):
        head += f"{num(origin[k])} {num(origin[k] + cell[k, k])} {axis}lo {axis}hi\n"
    xy, xz, yz = cell[1, 0], cell[2, 0], cell[2, 1]
    if xy != 0 or xz != 0 or yz != 0:
        head += f"{num(xy)} {num(xz)} {num(yz)} xy xz yz\n"
    head += "\n"
    if element_list is not None:
        head += "Masses\n\n" + "".join(f"{k} {num(MASS[e])} # {e}\n" for k, e in enumerate(list(element_list)[:num_type], start=1)) + "\n"
    head += f"Atoms # {data_format}\n\n"
    if data_format == "charge":
        q = cols["q"] if "q" in cols else np.zeros(n)
        body = table([cols["id"], cols["type"], q, cols["x"], cols["y"], cols["z"]])
    else:
        body = table([cols[k] for k in ("id", "type", "x", "y", "z")])
    if all(k in cols for k in ("vx", "vy", "vz")):
        body += b"\nVelocities\n\n" + table([cols[k] for k in ("id", "vx", "vy", "vz")])
    return head.encode() + body


def poscar(cols, box, reduced_pos=False, selective_dynamics=False) -> bytes:
    elements = [str(e) for e in cols["element"]]
    names = sorted(set(elements))
    order = sorted(range(len(elements)), key=lambda i: elements[i])  # (sorted() is stable: atoms of one element keep their order)
    x, y, z = moved(cols, np.array(box.origin), np.array(box.inverse_box) if reduced_pos else None)
    cell = np.array(box.box)
    head = "# VASP POSCAR file written by mdapy.\n1.0000000000\n"
    for k in range(3):
        head += "{:.10f} {:.10f} {:.10f}\n".format(*(float(v) for v in cell[k]))
    head += "".join(f"{e} " for e in names) + "\n" + "".join(f"{elements.count(e)} " for e in names) + "\n"
    if selective_dynamics:
        head += "Selective dynamics\n"
    head += "Direct\n" if reduced_pos else "Cartesian\n"
    columns = [x, y, z] + ([np.asarray(cols[k]) for k in ("sdx", "sdy", "sdz")] if selective_dynamics else [])
    return head.encode() + table([c[order] for c in columns])
