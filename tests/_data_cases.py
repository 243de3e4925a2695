"""LAMMPS data files as strings: the syntax variants of the reference's own samples (its tests/test_io_lammps.py:32-135, whose
files under tests/input_files/lammps/ are described there) written out again, and a few more.  Shared by
test_data_reader_host.py and test_gpu_data_reader.py."""
import gzip
import os

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "lammps_data")
SAMPLE = os.path.join(GOLDEN, "tri_box_small.data")

ATOMIC_BASIC = """# LAMMPS data file: four atoms, two types

4 atoms
2 atom types

0.0 4.0 xlo xhi
0.0 4.0 ylo yhi
0.0 4.0 zlo zhi

Masses

1 26.9815 # Al
2 63.546 # Cu

Atoms # atomic

1 1 0.0 0.0 0.0
2 2 2.0 0.0 0.0
3 1 0.0 2.0 0.0
4 2 2.0 2.0 0.0
"""

NO_STYLE_COMMENT = """# no atom style named, no element comments

4 atoms
2 atom types

0.0 4.0 xlo xhi
0.0 4.0 ylo yhi
0.0 4.0 zlo zhi

Masses

1 26.9815
2 63.546

Atoms

1 1 0.0 0.0 0.0
2 2 2.0 0.0 0.0
3 1 0.0 2.0 0.0
4 2 2.0 2.0 0.0
"""

MULTISPACE = """# column-aligned rows

4 atoms
1 atom types

0.0   4.0  xlo xhi
0.0   4.0  ylo yhi
\t0.0 \t 4.0  zlo zhi

Atoms # atomic

   1    1     0.0     0.0     0.0
   2    1     2.0     0.0     0.0
\t3\t1\t0.0\t2.0\t0.0
   4    1     2.0     2.0     0.0
"""

IMAGE_FLAGS = """# image flags

4 atoms
1 atom types

0.0 4.0 xlo xhi
0.0 4.0 ylo yhi
0.0 4.0 zlo zhi

Atoms # atomic

1 1 0.0 0.0 0.0 0 0 0
2 1 2.0 0.0 0.0 1 0 0
3 1 0.0 2.0 0.0 0 -1 0
4 1 2.0 2.0 0.0 0 0 2
"""

CHARGE_VELOCITIES = """# charge style, velocities out of order

3 atoms
2 atom types

-1.0 5.0 xlo xhi
-1.0 5.0 ylo yhi
-1.0 5.0 zlo zhi

Atoms # charge

1 1 1.0 0.0 0.0 0.0
2 2 -1.0 1.5 1.5 1.5
3 1 1.0 3.0 3.0 3.0

Velocities

3 0.0 0.0 0.0
1 0.1 0.2 0.3
2 -0.1 -0.2 -0.3
"""

TRICLINIC = """# triclinic cell

2 atoms
1 atom types

0.0 4.0 xlo xhi
0.0 4.0 ylo yhi
0.0 4.0 zlo zhi
1.0 0.5 0.3 xy xz yz

Atoms # atomic

1 1 0.0 0.0 0.0
2 1 2.0 2.0 2.0
"""

MASSES_BETWEEN = """# Masses after Atoms, before Velocities

2 atoms
1 atom types

0.0 4.0 xlo xhi
0.0 4.0 ylo yhi
0.0 4.0 zlo zhi

Atoms # atomic

1 1 0.0 0.0 0.0
2 1 2.0 2.0 2.0

Masses

1 63.546 # Cu

Velocities

1 1.0 2.0 3.0
2 4.0 5.0 6.0
"""

UNSUPPORTED_FULL = """# atom_style full

2 atoms
1 atom types
1 bonds
1 bond types

0.0 4.0 xlo xhi
0.0 4.0 ylo yhi
0.0 4.0 zlo zhi

Atoms # full

1 1 1 0.0 0.0 0.0 0.0
2 1 1 0.0 1.0 0.0 0.0

Bonds

1 1 1 2
"""

GOOD = {"atomic_basic": ATOMIC_BASIC, "no_style_comment": NO_STYLE_COMMENT, "multispace": MULTISPACE, "image_flags": IMAGE_FLAGS,
        "charge_velocities": CHARGE_VELOCITIES, "triclinic": TRICLINIC, "masses_between": MASSES_BETWEEN,
        "crlf": CHARGE_VELOCITIES.replace("\n", "\r\n"), "no_last_newline": MASSES_BETWEEN.rstrip("\n"),
        "short_velocities": CHARGE_VELOCITIES.rsplit("\n", 2)[0] + "\n"}  # (two velocity rows for three atoms: ignored)
# atoms 1, 2, 1 and velocity rows 1, 1, 2: of the two rows with id 1 the last wins
GOOD["duplicate_velocity"] = CHARGE_VELOCITIES.replace("3 0.0 0.0 0.0\n1 0.1 0.2 0.3\n2 -0.1 -0.2 -0.3\n", "1 0.1 0.2 0.3\n1 9.0 8.0 7.0\n2 -0.1 -0.2 -0.3\n").replace(
    "3 1 1.0 3.0 3.0 3.0\n", "1 1 1.0 3.0 3.0 3.0\n")


# every error of the reader: the file, the exception's type, and words its message must hold
BAD = {
    "no_atoms": ATOMIC_BASIC.replace("Atoms # atomic", "# Atoms"),
    "header_hint": UNSUPPORTED_FULL,
    "style_full": UNSUPPORTED_FULL.replace("1 bonds\n1 bond types\n", ""),
    "style_contradicts": ATOMIC_BASIC.replace("Atoms # atomic", "Atoms # charge"),
    "cannot_infer": NO_STYLE_COMMENT.replace("1 1 0.0 0.0 0.0\n", "1 1 0.0 0.0 0.0 7 7\n"),
    "few_rows": ATOMIC_BASIC.replace("4 atoms", "5 atoms"),
    "few_rows_no_newline": ATOMIC_BASIC.replace("4 atoms", "6 atoms").rstrip("\n"),
    "missing_velocity": CHARGE_VELOCITIES.replace("3 0.0 0.0 0.0\n", "7 0.0 0.0 0.0\n"),
    "type_without_element": MASSES_BETWEEN.replace("2 1 2.0 2.0 2.0", "2 5 2.0 2.0 2.0"),
    "empty_atoms": TRICLINIC.split("Atoms # atomic")[0] + "Atoms # atomic\n\n# nothing\n",
}
KIND = {"no_atoms": ValueError, "header_hint": NotImplementedError, "style_full": NotImplementedError, "style_contradicts": ValueError,
        "cannot_infer": NotImplementedError, "few_rows": ValueError, "few_rows_no_newline": ValueError, "missing_velocity": KeyError,
        "type_without_element": ValueError, "empty_atoms": ValueError}
WORDING = {"no_atoms": "no 'Atoms' section found", "header_hint": "found header keyword 'bonds'", "style_full": "atom_style 'full' not supported",
           "style_contradicts": "atom_style 'charge' expects (6, 9) columns, got 5", "cannot_infer": "cannot infer atom_style from 7-column",
           "few_rows": "expected 5 atom rows, found 4", "few_rows_no_newline": "expected 6 atom rows, found 4", "missing_velocity": "3",
           "type_without_element": "atom type 5", "empty_atoms": "'Atoms' section is empty"}


def write(tmp_path, name, text, suffix=".data"):
    """the case as a file (``suffix`` .data, .lmp or .data.gz); returns its path"""
    path = os.path.join(str(tmp_path), name + suffix)
    raw = text.encode()
    if suffix.endswith(".gz"):
        with gzip.open(path, "wb") as f:
            f.write(raw)
    else:
        with open(path, "wb") as f:
            f.write(raw)
    return path
