"""The writers of ``mdapy_amd.load_save`` on the host path (what a machine without a GPU runs): every file equals, byte for
byte, the restatement in tests/_write_ref.py; what was written reads back; every error the writers raise.  No GPU needed."""
import gzip
import warnings

import numpy as np
import pytest

import _write_ref as R
import mdapy_amd as mp
from mdapy_amd import load_save as LS
from mdapy_amd.box import Box
from mdapy_amd.frame import Frame
from mdapy_amd.trajectory import Trajectory


@pytest.fixture(autouse=True)
def host_only(monkeypatch):
    monkeypatch.setattr(LS, "have_gpu", lambda: False)


BOXES = {
    "orthogonal": lambda: Box(np.diag([10.0, 11.0, 12.5])),
    "lammps-triclinic": lambda: Box(np.array([[10.0, 0, 0], [1.25, 11.0, 0], [-2.0, 3.5, 12.0]])),
    "general-triclinic": lambda: Box(np.array([[10.0, 1.0, 0.5], [1.0, 11.0, 2.0], [2.0, 3.0, 12.0]])),
    "slab": lambda: Box(np.diag([10.0, 11.0, 12.5]), [1, 0, 1]),
    "origin": lambda: Box(np.diag([10.0, 11.0, 12.5]), [1, 1, 1], [-3.5, 0.25, 7.0]),
    "general-triclinic-origin": lambda: Box(np.array([[10.0, 1.0, 0.5], [1.0, 11.0, 2.0], [2.0, 3.0, 12.0]]), [0, 1, 1], [1.0, -2.0, 0.125]),
}


def columns(n=37, seed=0, with_id=False, small_ints=False):
    rng = np.random.default_rng(seed)
    cols = {"x": rng.uniform(-5, 15, n), "y": rng.uniform(-5, 15, n), "z": rng.uniform(-5, 15, n)}
    if with_id:
        cols["id"] = rng.permutation(n).astype(np.int32) + 1
    cols["type"] = rng.integers(1, 3, n).astype(np.int32)
    cols["element"] = np.array(["Cu", "Al"], dtype=object)[cols["type"] - 1]
    cols["c_pe"] = rng.standard_normal(n) * 1e3
    cols["cna"] = rng.integers(0, 5, n).astype(np.int32)
    cols["big"] = rng.integers(-1000, 1000, n) if small_ints else rng.integers(-2 ** 62, 2 ** 62, n)
    return cols


@pytest.mark.parametrize("box", list(BOXES))
@pytest.mark.parametrize("with_id", [False, True])
def test_four_writers_equal_the_restatement(tmp_path, box, with_id):
    cols, cell = columns(with_id=with_id), BOXES[box]()
    frame = Frame(cols)
    p = str(tmp_path / "out")
    LS.write_dump(p, frame, cell, timestep=7)
    assert open(p, "rb").read() == R.dump(cols, cell, 7)
    LS.write_xyz(p, frame, cell, energy=-1.5, stress="1 2 3")
    assert open(p, "rb").read() == R.xyz(cols, cell, energy=-1.5, stress="1 2 3")
    LS.write_xyz(p, frame, cell, classical=True)
    assert open(p, "rb").read() == R.xyz(cols, cell, classical=True)
    LS.write_data(p, frame, cell)
    assert open(p, "rb").read() == R.data(cols, cell)
    LS.write_data(p, frame, cell, element_list=["Cu", "Al"], num_type=2, data_format="charge")
    assert open(p, "rb").read() == R.data(cols, cell, ["Cu", "Al"], 2, "charge")
    LS.write_poscar(p, frame, cell)
    assert open(p, "rb").read() == R.poscar(cols, cell)
    LS.write_poscar(p, frame, cell, reduced_pos=True)
    assert open(p, "rb").read() == R.poscar(cols, cell, reduced_pos=True)


def test_header_wording(tmp_path):
    cols, cell = columns(), BOXES["orthogonal"]()
    p = str(tmp_path / "a.dump")
    LS.write_dump(p, Frame(cols), cell)
    lines = open(p, "rb").read().split(b"\n")
    assert lines[:5] == [b"ITEM: TIMESTEP", b"0.0", b"ITEM: NUMBER OF ATOMS", b"37", b"ITEM: BOX BOUNDS pp pp pp"]
    assert lines[8] == b"ITEM: ATOMS id x y z type element c_pe cna big "  # (the reference's trailing blank)
    assert lines[9].startswith(b"1 ")
    LS.write_dump(p, Frame(cols), BOXES["lammps-triclinic"]())
    assert open(p, "rb").read().split(b"\n")[4:6] == [b"ITEM: BOX BOUNDS xy xz yz pp pp pp", b"-2.0 11.25 1.25"]
    LS.write_dump(p, Frame(cols), BOXES["slab"]())
    assert open(p, "rb").read().split(b"\n")[4] == b"ITEM: BOX BOUNDS pp ss pp"


def test_velocities_charge_and_other_columns(tmp_path):
    rng = np.random.default_rng(5)
    cols = columns(n=20, with_id=True)
    cols.update(vx=rng.standard_normal(20), vy=rng.standard_normal(20), vz=rng.standard_normal(20), q=rng.standard_normal(20),
                f32=rng.standard_normal(20).astype(np.float32), i16=rng.integers(-9, 9, 20).astype(np.int16),
                u64=rng.integers(0, 2 ** 63, 20).astype(np.uint64) * np.uint64(2), flag=rng.integers(0, 2, 20).astype(bool),
                typelabel=np.array(["a", "b"], dtype=object)[rng.integers(0, 2, 20)])
    cell = BOXES["general-triclinic-origin"]()
    p = str(tmp_path / "out")
    LS.write_data(p, Frame(cols), cell, data_format="charge")
    assert open(p, "rb").read() == R.data(cols, cell, data_format="charge")
    assert b"\nVelocities\n\n" in open(p, "rb").read()
    LS.write_dump(p, Frame(cols), cell)  # the bool column and the second string column are dropped, `element` stays
    assert open(p, "rb").read() == R.dump(cols, cell)
    head = open(p, "rb").read().split(b"\n")[8]
    assert b"flag" not in head and b"typelabel" not in head and b" element " in head and b" u64 " in head
    with pytest.raises(ValueError, match="Unrecognised dtype bool in extended XYZ output"):
        LS.write_xyz(p, Frame(cols), cell)
    del cols["flag"]
    LS.write_xyz(p, Frame(cols), cell)
    assert open(p, "rb").read() == R.xyz(cols, cell)
    assert b"vel:R:3" in open(p, "rb").read() and b"species:S:1" in open(p, "rb").read() and b"typelabel:S:1" in open(p, "rb").read()


def test_xyz_properties_fold_runs():
    names = ["element", "x", "y", "z", "fx", "fy", "fz", "d_0", "d_1", "d_2", "e_0", "x2", "xu", "yu", "zu", "k_0", "k_1"]
    dtypes = [object] + [np.float64] * 6 + [np.int32] * 3 + [np.float64, np.float32] + [np.float64] * 3 + [np.int32, np.int64]
    assert LS._xyz_properties(names, dtypes) == ("Properties=species:S:1:pos:R:3:forces:R:3:d:I:3:e_0:R:1:x2:R:1:unwrapped_position:R:3"
                                                 ":k_0:I:1:k_1:I:1")
    cols = {n: np.zeros(2, dtype=d) if d is not object else np.array(["H", "H"], dtype=object) for n, d in zip(names, dtypes)}
    assert R.xyz_properties(cols) == LS._xyz_properties(names, dtypes)
    assert LS._xyz_properties(["x", "y", "z"], [np.float64, np.float64, np.int32]) == "Properties=x:R:1:y:R:1:z:I:1"


def test_selective_dynamics_and_stable_sort(tmp_path):
    cols = columns(n=30)
    cols["element"] = np.array(["Zr", "Al", "Cu"], dtype=object)[np.arange(30) % 3]
    cols.update(sdx=np.arange(30, dtype=np.int32) % 2, sdy=np.ones(30, np.int32), sdz=np.array(["T", "F"], dtype=object)[np.arange(30) % 2])
    cell = BOXES["origin"]()
    p = str(tmp_path / "POSCAR")
    LS.write_poscar(p, Frame(cols), cell, selective_dynamics=True)
    got = open(p, "rb").read()
    assert got == R.poscar(cols, cell, selective_dynamics=True)
    lines = got.decode().split("\n")
    assert lines[5:9] == ["Al Cu Zr ", "10 10 10 ", "Selective dynamics", "Cartesian"]
    first_al = format(cols["x"][1] - cell.origin[0], ".10f")  # atom 1 is the first Al: it leads the table
    assert lines[9].startswith(first_al + " ")


def _rounded(a):
    return np.array([float(format(v, ".10f")) for v in a.tolist()])


@pytest.mark.parametrize("box", ["orthogonal", "lammps-triclinic", "slab", "origin"])
@pytest.mark.parametrize("gz", [False, True])
def test_dump_and_xyz_round_trip(tmp_path, box, gz):
    cols, cell = columns(with_id=True, small_ints=True), BOXES[box]()
    frame = Frame(cols)
    name = str(tmp_path / "rt.dump")
    LS.write_dump(name, frame, cell, timestep=12, compress=gz)
    back, cell2, info = LS.read_dump(name + (".gz" if gz else ""))
    assert info == {"timestep": 12}
    assert set(back.columns) == set(cols)
    for k, v in cols.items():
        got = back[k].to_numpy()
        if v.dtype.kind == "f":
            assert got.tobytes() == _rounded(v).tobytes(), k
        elif v.dtype.kind == "O":
            assert list(got) == list(v)
        else:
            assert np.array_equal(got, v), k
    assert np.array_equal(cell2.box, cell.box) and np.array_equal(cell2.origin, cell.origin) and np.array_equal(cell2.boundary, cell.boundary)

    name = str(tmp_path / "rt.xyz")
    LS.write_xyz(name, frame, cell, compress=gz)
    back, cell2, info = LS.read_xyz(name + (".gz" if gz else ""))
    for k, v in cols.items():
        got = back[k].to_numpy()
        if v.dtype.kind == "f":
            assert got.tobytes() == _rounded(v).tobytes(), k
        elif v.dtype.kind == "O":
            assert list(got) == list(v)
        else:
            assert np.array_equal(got, v), k
    assert np.array_equal(cell2.box, cell.box) and np.array_equal(cell2.origin, cell.origin) and np.array_equal(cell2.boundary, cell.boundary)


def test_compress_appends_gz_once(tmp_path):
    cols, cell = columns(), BOXES["orthogonal"]()
    LS.write_dump(str(tmp_path / "a.dump"), Frame(cols), cell, compress=True)
    LS.write_dump(str(tmp_path / "b.dump.gz"), Frame(cols), cell, compress=True)
    want = R.dump(cols, cell)
    assert gzip.open(tmp_path / "a.dump.gz").read() == want and gzip.open(tmp_path / "b.dump.gz").read() == want
    assert not (tmp_path / "a.dump").exists() and not (tmp_path / "b.dump.gz.gz").exists()
    for writer, name, ref in ((LS.write_data, "a.data", R.data), (LS.write_poscar, "POSCAR", R.poscar), (LS.write_xyz, "a.xyz", R.xyz)):
        writer(str(tmp_path / name), Frame(cols), cell, compress=True)
        assert gzip.open(str(tmp_path / name) + ".gz").read() == ref(cols, cell)


def test_non_finite_round_trips_and_huge_values_are_written(tmp_path):
    cols = columns(n=6, small_ints=True)
    cols["c_pe"] = np.array([np.nan, np.inf, -np.inf, 1e30, -1.7976931348623157e308, 2.0 ** 64])
    cell = BOXES["orthogonal"]()
    p = str(tmp_path / "nf.dump")
    LS.write_dump(p, Frame(cols), cell, timestep=0)
    assert open(p, "rb").read() == R.dump(cols, cell, 0)
    rows = open(p).read().split("\n")[9:12]
    assert [r.split()[6] for r in rows] == ["NaN", "inf", "-inf"]
    back = LS.read_dump(p)[0]["c_pe"].to_numpy()
    assert np.isnan(back[0]) and back[1] == np.inf and back[2] == -np.inf
    assert back[3:].tobytes() == cols["c_pe"][3:].tobytes()  # (integers, all of them: ten decimals lose nothing)


def test_errors(tmp_path):
    cols, cell = columns(), BOXES["orthogonal"]()
    p = str(tmp_path / "x")
    frame = Frame(cols)
    for writer, missing in ((LS.write_dump, "type"), (LS.write_data, "type"), (LS.write_xyz, "element"), (LS.write_poscar, "element"),
                            (LS.write_dump, "x"), (LS.write_xyz, "z")):
        with pytest.raises(ValueError, match=f"data must contain {missing} column"):
            writer(p, frame.drop(missing), cell)
    for writer in (LS.write_dump, LS.write_data, LS.write_xyz, LS.write_poscar):
        with pytest.raises(TypeError, match="data must be a Frame"):
            writer(p, cols, cell)
    with pytest.raises(ValueError, match="Unrecognized data format: full. Only support atomic and charge"):
        LS.write_data(p, frame, cell, data_format="full")
    with pytest.raises(ValueError, match=r"num_type \(1\) is less than the largest type in data \(2\)"):
        LS.write_data(p, frame, cell, num_type=1)
    with pytest.raises(ValueError, match="element_list has 1 entries but num_type is 2; need at least 2"):
        LS.write_data(p, frame, cell, element_list=["Cu"])
    with pytest.raises(ValueError, match="Unrecognized element name Xx"):
        LS.write_data(p, frame, cell, element_list=["Cu", "Xx"])
    with pytest.warns(UserWarning, match="element_list has 3 entries but num_type=2; writing only the first 2 elements."):
        LS.write_data(p, frame, cell, element_list=["Cu", "Al", "Fe"])
    assert open(p, "rb").read() == R.data(cols, cell, ["Cu", "Al", "Fe"])
    with pytest.raises(ValueError, match="data must contain sdx if selective_dynamics=True"):
        LS.write_poscar(p, frame, cell, selective_dynamics=True)
    for bad in ("C u", 'C"u', "C'u", "C\nu", "C\tu"):
        named = frame.with_columns(element=np.array([bad] * 37, dtype=object))
        for writer in (LS.write_dump, LS.write_xyz, LS.write_poscar):
            with pytest.raises(ValueError, match="blank, a quote or a line break"):
                writer(p, named, cell)
    with pytest.raises(ValueError, match="Unrecognised dtype complex128 in extended XYZ output"):
        LS.write_xyz(p, frame.with_columns(w=np.zeros(37, complex)), cell)


def test_system_methods(tmp_path):
    cols, cell = columns(with_id=True, small_ints=True), BOXES["lammps-triclinic"]()
    s = mp.System(data=Frame(cols), box=cell, global_info={"energy": -3.25})
    for name in ("write_mp", "write_xyz", "write_poscar", "write_data", "write_dump"):
        assert callable(getattr(s, name))
    p = str(tmp_path / "s")
    s.write_dump(p)
    assert open(p, "rb").read() == R.dump(cols, cell, 0)  # (the method's default timestep is the integer 0, the function's 0.0)
    s.write_dump(p, timestep=5, compress=True)
    assert gzip.open(p + ".gz").read() == R.dump(cols, cell, 5)
    s.write_xyz(p)
    assert open(p, "rb").read() == R.xyz(cols, cell, energy=-3.25)
    s.write_xyz(p, classical=True)
    assert open(p, "rb").read() == R.xyz(cols, cell, classical=True)
    s.write_poscar(p, reduced_pos=True)
    assert open(p, "rb").read() == R.poscar(cols, cell, reduced_pos=True)
    s.write_data(p, element_list=["Al", "Cu"])  # `type` follows the list's order for this file; the system keeps its own
    retyped = dict(cols, type=np.where(cols["element"] == "Al", 1, 2).astype(np.int32))
    assert open(p, "rb").read() == R.data(retyped, cell, ["Al", "Cu"])
    assert np.array_equal(s.data["type"].to_numpy(), cols["type"])
    with pytest.raises(AssertionError, match="element_list must include element 'Cu'."):
        s.write_data(p, element_list=["Al"])
    pytest.importorskip("pyarrow")
    s.write_mp(p + ".mp")
    back = mp.System(p + ".mp")
    assert np.array_equal(back.data["x"].to_numpy(), cols["x"]) and back.global_info["energy"] == "-3.25"


def test_trajectory_save(tmp_path):
    frames = []
    for k in range(3):
        cols = columns(n=11 + k, seed=k, with_id=True, small_ints=True)
        frames.append(mp.System(data=Frame(cols), box=BOXES["origin"](), global_info={"timestep": 100 * k}))
    traj = Trajectory(systems=frames)
    name = str(tmp_path / "t.dump")
    traj.save(name, frames=[0, 1])
    traj.save(name, frames=2, mode="a")
    back = Trajectory(name)
    assert len(back) == 3
    for a, b in zip(frames, back):
        assert b.global_info["timestep"] == a.global_info["timestep"]
        assert np.array_equal(b.box.origin, a.box.origin) and b.N == a.N
        assert b.data["x"].to_numpy().tobytes() == _rounded(a.data["x"].to_numpy()).tobytes()
        assert np.array_equal(b.data["id"].to_numpy(), a.data["id"].to_numpy())
        assert list(b.data["element"].to_numpy()) == list(a.data["element"].to_numpy())
    want = b"".join(R.dump({c: s.data[c].to_numpy() for c in s.data.columns}, s.box, int(s.global_info["timestep"])) for s in frames)
    assert open(name, "rb").read() == want
    traj.save(str(tmp_path / "t.dump.gz"))
    assert gzip.open(tmp_path / "t.dump.gz").read() == want
    traj.save(name)  # mode 'w' starts over
    assert open(name, "rb").read() == want
    with pytest.raises(NotImplementedError, match="dump format only"):
        traj.save(str(tmp_path / "t.xyz"))
    with pytest.raises(ValueError, match="mode must be 'w' or 'a', got 'x'"):
        traj.save(name, mode="x")
    with pytest.raises(ValueError, match="Cannot infer trajectory format"):
        traj.save(str(tmp_path / "t.bin"))
