"""The LAMMPS data-file reader on a machine without a GPU: every syntax variant through ``System(path)`` and
``BuildSystem.read_data`` against the plain-Python restatement (tests/_data_ref.py), every error by type and message, the
round trip through ``write_data``, the section matcher the scan kernel shares with its host twin, and the argument checks of
the two new entries."""
import ctypes
import os

import numpy as np
import pytest

import _data_cases as C
import _data_ref as R
import mdapy_amd as mp
from mdapy_amd import _lib, _text
from mdapy_amd import load_save as LS
from mdapy_amd.load_save import BuildSystem


def same_as_ref(got, ref):
    frame, box, info = got
    cols, rbox, rinfo = ref
    assert frame.columns == list(cols) and info == rinfo == {}
    for c in frame.columns:
        a, b = frame[c].to_numpy(), cols[c]
        if b.dtype == object:
            assert a.dtype == object and list(a) == list(b), c
        else:
            assert a.dtype == b.dtype and a.tobytes() == b.tobytes(), c
    assert np.asarray(box.box).tobytes() == rbox[:3].tobytes()
    assert np.asarray(box.origin, dtype=np.float64).tobytes() == rbox[3].tobytes()
    assert list(box.boundary) == [1, 1, 1]


def both_doors(path, **kw):
    s = mp.System(path, **kw)
    yield s.data, s.box, s.global_info
    yield BuildSystem.read_data(path)
    if not kw:
        yield BuildSystem.from_file(path)


@pytest.mark.parametrize("name", sorted(C.GOOD))
def test_cases_match_restatement(name, tmp_path):
    path = C.write(tmp_path, name, C.GOOD[name])
    ref = R.read_data(path)
    for got in both_doors(path):
        same_as_ref(got, ref)


def test_reference_sample():
    ref = R.read_data(C.SAMPLE)
    assert list(ref[0]) == ["id", "type", "x", "y", "z", "vx", "vy", "vz", "element"] and list(ref[0]["element"]) == ["C"]
    for got in both_doors(C.SAMPLE):
        same_as_ref(got, ref)
    assert os.path.getsize(C.SAMPLE) == 278


def test_expected_values():
    """the restatement itself, against the values the reference's tests state"""
    import tempfile

    with tempfile.TemporaryDirectory() as d:
        cols, box, _ = R.read_data(C.write(d, "a", C.ATOMIC_BASIC))
        assert cols["type"].tolist() == [1, 2, 1, 2] and list(cols["element"]) == ["Al", "Cu", "Al", "Cu"]
        assert np.diag(box[:3]).tolist() == [4, 4, 4]
        cols, box, _ = R.read_data(C.write(d, "b", C.IMAGE_FLAGS))
        assert cols["ix"].tolist() == [0, 1, 0, 0] and cols["iy"].tolist() == [0, 0, -1, 0] and cols["iz"].tolist() == [0, 0, 0, 2]
        assert cols["ix"].dtype == np.int32 and "element" not in cols
        cols, box, _ = R.read_data(C.write(d, "c", C.CHARGE_VELOCITIES))
        assert list(cols) == ["id", "type", "q", "x", "y", "z", "vx", "vy", "vz"]
        assert cols["q"].tolist() == [1.0, -1.0, 1.0] and cols["vx"].tolist() == [0.1, -0.1, 0.0] and cols["vz"].tolist() == [0.3, -0.3, 0.0]
        assert box[3].tolist() == [-1, -1, -1]
        cols, box, _ = R.read_data(C.write(d, "d", C.TRICLINIC))
        assert box[:3].tolist() == [[4, 0, 0], [1.0, 4, 0], [0.5, 0.3, 4]]
        cols, box, _ = R.read_data(C.write(d, "e", C.MASSES_BETWEEN))
        assert cols["vx"].tolist() == [1.0, 4.0] and cols["vz"].tolist() == [3.0, 6.0] and list(cols["element"]) == ["Cu", "Cu"]
        cols, box, _ = R.read_data(C.write(d, "f", C.GOOD["duplicate_velocity"]))
        assert cols["id"].tolist() == [1, 2, 1] and cols["vx"].tolist() == [9.0, -0.1, 9.0]
        cols, box, _ = R.read_data(C.write(d, "g", C.GOOD["short_velocities"]))
        assert "vx" not in cols


def test_names_and_formats(tmp_path):
    ref = R.read_data(C.write(tmp_path, "ref", C.ATOMIC_BASIC))
    for got in both_doors(C.write(tmp_path, "a", C.ATOMIC_BASIC, ".lmp")):
        same_as_ref(got, ref)
    for got in both_doors(C.write(tmp_path, "b", C.ATOMIC_BASIC, ".data.gz")):
        same_as_ref(got, ref)
    for got in both_doors(C.write(tmp_path, "c", C.ATOMIC_BASIC, ".lmp.gz")):
        same_as_ref(got, ref)
    odd = C.write(tmp_path, "d", C.ATOMIC_BASIC, ".txt")
    for fmt in ("data", "lmp"):
        s = mp.System(odd, format=fmt)
        same_as_ref((s.data, s.box, s.global_info), ref)
        same_as_ref(BuildSystem.from_file(odd, format=fmt), ref)
    same_as_ref(LS.read_file(odd, "data"), ref)
    with pytest.raises(ValueError, match="outside its input side"):
        BuildSystem.from_file("POSCAR.poscar")


BAD, KIND, WORDING = C.BAD, C.KIND, C.WORDING


@pytest.mark.parametrize("name", sorted(BAD))
def test_errors_by_type_and_message(name, tmp_path):
    path = C.write(tmp_path, name, BAD[name])
    with pytest.raises(KIND[name]) as want:
        R.read_data(path)
    assert type(want.value) is KIND[name] and WORDING[name] in str(want.value)
    for door in (mp.System, BuildSystem.read_data):
        with pytest.raises(KIND[name]) as got:
            door(path)
        assert type(got.value) is KIND[name] and str(got.value) == str(want.value)
        if KIND[name] is not KeyError:
            assert str(got.value).startswith(path + ": ")
        else:
            assert got.value.args == (3,)


def test_wrong_shaped_header_lines_are_skipped(tmp_path):
    text = C.ATOMIC_BASIC.replace("4 atoms\n", "many atoms\n4 atoms\nx atom types\n").replace("0.0 4.0 zlo zhi\n", "0.0 4.0 zlo zhi\nzhi\n1.0 xy xz yz\n")
    path = C.write(tmp_path, "odd_header", text)
    ref = R.read_data(path)
    assert len(ref[0]["id"]) == 4 and ref[1][1, 0] == 0.0
    for got in both_doors(path):
        same_as_ref(got, ref)


# ---- write_data, then read
def _system(triclinic, velocities, charge):
    rng = np.random.default_rng(5)
    n = 57
    cell = np.array([[11.3, 0, 0], [1.7, 9.9, 0], [-0.8, 2.1, 12.4]]) if triclinic else np.diag([11.3, 9.9, 12.4])
    pos = rng.random((n, 3)) @ cell + np.array([-2.5, 0.25, 3.0])
    cols = {"id": rng.permutation(n).astype(np.int32) + 1, "type": rng.integers(1, 4, n).astype(np.int32),
            "x": pos[:, 0].copy(), "y": pos[:, 1].copy(), "z": pos[:, 2].copy()}
    if charge:
        cols["q"] = rng.choice([-1.0, 0.5, 1.0], n)
    if velocities:
        for k, c in enumerate(("vx", "vy", "vz")):
            cols[c] = rng.normal(0, 3.0, n)
    return mp.System(data=cols, box=mp.Box(cell, [1, 1, 1], [-2.5, 0.25, 3.0]))


def _printed(a):
    return np.array([float(format(v, ".10f")) for v in a], dtype=np.float64)


@pytest.mark.parametrize("triclinic", [False, True])
@pytest.mark.parametrize("velocities", [False, True])
@pytest.mark.parametrize("style", ["atomic", "charge"])
def test_round_trip(triclinic, velocities, style, tmp_path):
    s = _system(triclinic, velocities, style == "charge")
    elements = ["Al", "Cu", "Fe"]
    path = os.path.join(str(tmp_path), "out.data")
    s.write_data(path, element_list=elements, data_format=style)
    back = mp.System(path)
    want = ["id", "type"] + (["q"] if style == "charge" else []) + ["x", "y", "z"] + (["vx", "vy", "vz"] if velocities else []) + ["element"]
    assert back.data.columns == want
    for c in "xyz":
        assert back.data[c].to_numpy().tobytes() == _printed(s.data[c].to_numpy()).tobytes()
    for c in ("id", "type"):
        assert back.data[c].dtype == np.int32 and np.array_equal(back.data[c].to_numpy(), s.data[c].to_numpy())
    if style == "charge":
        assert np.array_equal(back.data["q"].to_numpy(), s.data["q"].to_numpy())
    if velocities:
        for c in ("vx", "vy", "vz"):
            assert back.data[c].to_numpy().tobytes() == _printed(s.data[c].to_numpy()).tobytes()
    assert list(back.data["element"].to_numpy()) == [elements[t - 1] for t in s.data["type"].to_numpy()]
    # the header prints every number with repr's digits: what is read back is within a rounding of a sum and a difference
    assert np.allclose(back.box.box, s.box.box, rtol=0, atol=4 * np.finfo(np.float64).eps * 16)
    assert np.array_equal(back.box.origin, s.box.origin) and list(back.box.boundary) == [1, 1, 1]
    same_as_ref((back.data, back.box, back.global_info), R.read_data(path))


def test_round_trip_gz(tmp_path):
    s = _system(True, True, True)
    path = os.path.join(str(tmp_path), "out.data.gz")
    s.write_data(path, data_format="charge", compress=True)
    back = mp.System(path)
    assert "element" not in back.data.columns
    same_as_ref((back.data, back.box, back.global_info), R.read_data(path))


# ---- the section matcher (csrc/text_sections.hpp) through its host twin
def _scan(raw):
    found, lines = _text.scan_sections(raw, R.WORDS)
    want, want_lines = R.section_offsets(raw)
    assert found == want and lines == want_lines, raw[:60]
    return found


def test_scan_hook_matches_restatement(tmp_path):
    for text in list(C.GOOD.values()) + list(BAD.values()) + [open(C.SAMPLE, "rb").read().decode()]:
        _scan(text.encode())
    assert _scan(b"Atoms\n1 1 0 0 0\n") == {"Atoms": 0}  # a keyword at byte 0
    assert _scan(b"1 atoms\nMasses") == {"Masses": 8}  # the last line, without a line feed
    assert _scan(b"x\n \t Velocities # c\n") == {"Velocities": 2}  # blanks and tabs first: the LINE's offset
    assert _scan(b"Atoms#atomic\nAtomsx\n# Atoms\n  #Atoms\nAtom\n") == {"Atom": 37}
    assert _scan(b"1 1\r\nAtoms\r\n\r\n1 1 0 0 0\r\n") == {"Atoms": 5}  # `Atoms\r` matches
    assert _scan(b"Atoms\nAtoms\nMasses\n\nMasses") == {"Atoms": 0, "Masses": 12}  # the first line counts
    assert _scan(b"PairIJ Coeffs\nPair Coeffs\nBond Coeffs\nBonds\n") == {"PairIJ": 0, "Pair": 14, "Bond": 26, "Bonds": 38}
    assert _scan(b"") == {} and _scan(b"\n") == {} and _scan(b"Atoms") == {"Atoms": 0} and _scan(b"\r \t") == {}
    assert _text.scan_sections(b"\n\n", R.WORDS)[1] == 2 and _text.scan_sections(b"a\nb", R.WORDS)[1] == 2


def test_scan_hook_random_texts():
    rng = np.random.default_rng(11)
    pieces = [w.encode() for w in R.WORDS] + [b" ", b"\t", b"\r", b"\n", b"\n", b"#", b"1 2 3", b"x", b"Atomsx", b"-0.5"]
    for _ in range(300):
        raw = b"".join(pieces[k] for k in rng.integers(0, len(pieces), rng.integers(0, 40)))
        _scan(raw)


def _words(words):
    raw = [w.encode() for w in words]
    return (ctypes.c_char_p * len(raw))(*raw)


def test_bad_arguments_are_refused_before_any_device_work():
    L = _lib.lib()
    out, lines, text = np.zeros(32, np.int64), ctypes.c_int64(0), b"Atoms\n"
    good = _words(["Atoms"])
    for entry, extra in ((L.mdh_scan_sections, (None,)), (L.mdh_debug_scan_sections, ())):
        def call(t, n, w, nw, o, ln):
            args = (t, n, _lib.HOST, w, nw, o, ln) if extra else (t, n, w, nw, o, ln)
            return entry(*args, *extra)
        assert call(text, -1, good, 1, out.ctypes.data, ctypes.addressof(lines)) == _lib.ERR_ARG
        assert call(None, 6, good, 1, out.ctypes.data, ctypes.addressof(lines)) == _lib.ERR_ARG
        assert call(text, 6, good, 0, out.ctypes.data, ctypes.addressof(lines)) == _lib.ERR_ARG
        assert call(text, 6, None, 1, out.ctypes.data, ctypes.addressof(lines)) == _lib.ERR_ARG
        assert call(text, 6, good, 1, None, ctypes.addressof(lines)) == _lib.ERR_ARG
        assert call(text, 6, good, 1, out.ctypes.data, None) == _lib.ERR_ARG
        assert call(text, 6, _words(["A" * 16]), 1, out.ctypes.data, ctypes.addressof(lines)) == _lib.ERR_ARG
        assert call(text, 6, _words([""]), 1, out.ctypes.data, ctypes.addressof(lines)) == _lib.ERR_ARG
        assert call(text, 6, _words(["A b"]), 1, out.ctypes.data, ctypes.addressof(lines)) == _lib.ERR_ARG
        assert call(text, 6, _words(["A"] * 33), 33, out.ctypes.data, ctypes.addressof(lines)) == _lib.ERR_ARG
        assert b"words" in L.mdh_last_error()
    ids, rows, status = np.arange(4, dtype=np.int32), np.zeros(4, np.int32), np.zeros(4, np.int64)
    assert L.mdh_match_ids(ids.ctypes.data, ids.ctypes.data, -1, rows.ctypes.data, status.ctypes.data, _lib.HOST, None) == _lib.ERR_ARG
    assert L.mdh_match_ids(ids.ctypes.data, ids.ctypes.data, 2 ** 31 - 1, rows.ctypes.data, status.ctypes.data, _lib.HOST, None) == _lib.ERR_ARG
    assert L.mdh_match_ids(None, ids.ctypes.data, 4, rows.ctypes.data, status.ctypes.data, _lib.HOST, None) == _lib.ERR_ARG
    assert L.mdh_match_ids(ids.ctypes.data, None, 4, rows.ctypes.data, status.ctypes.data, _lib.HOST, None) == _lib.ERR_ARG
    assert L.mdh_match_ids(ids.ctypes.data, ids.ctypes.data, 4, None, status.ctypes.data, _lib.HOST, None) == _lib.ERR_ARG
    assert L.mdh_match_ids(ids.ctypes.data, ids.ctypes.data, 4, rows.ctypes.data, None, _lib.HOST, None) == _lib.ERR_ARG
    assert b"mdh_match_ids" in L.mdh_last_error()
    # nothing to do is no error, and needs no device either
    assert L.mdh_match_ids(None, None, 0, None, status.ctypes.data, _lib.HOST, None) == 0 and status.tolist() == [0, -1, 0, 0]
    assert L.mdh_scan_sections(None, 0, _lib.HOST, good, 1, out.ctypes.data, ctypes.addressof(lines), None) == 0 and out[0] == -1
