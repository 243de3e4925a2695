"""The writers of ``mdapy_amd.load_save`` on the device path — columns in HBM, the table formatted by csrc/text_format.hip in
pieces and streamed to the file through pinned buffers — against the restatement in tests/_write_ref.py and against the host
path: bytes, no tolerance.  A monkeypatch sends every table to the device whatever its size, as tests/test_gpu_load_save.py does
for reading."""
import glob
import gzip
import io
import os

import numpy as np
import pytest

import _write_ref as R
import mdapy_amd.load_save as LS
from mdapy_amd import _text
from mdapy_amd.box import Box
from mdapy_amd.frame import Frame

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))


@pytest.fixture(autouse=True)
def device_path(monkeypatch):
    from mdapy_amd import _lib

    if _lib.device_count() < 1:
        pytest.fail("test_gpu_write needs a HIP device")
    monkeypatch.setattr(LS, "DEVICE_MIN_BYTES", 0)
    monkeypatch.setattr(LS, "DEVICE_MIN_ROWS", 0)


@pytest.fixture
def formatted(monkeypatch):
    """how many pieces the device formatter was asked for"""
    calls = []
    real = _text._format
    monkeypatch.setattr(_text, "_format", lambda *a, **k: (calls.append(1), real(*a, **k))[1])
    return calls


def on_host(writer, path, *args, **kwargs):
    with pytest.MonkeyPatch.context() as m:
        m.setattr(LS, "have_gpu", lambda: False)
        writer(path, *args, **kwargs)
    return open(path, "rb").read()


def completed(frame):
    """the frame with the columns every writer needs (``type`` from ``element`` or the other way round), and its host copy"""
    if "type" not in frame.columns:
        names = sorted(set(frame["element"].to_numpy()))
        frame = frame.with_columns(type=np.array([names.index(e) + 1 for e in frame["element"].to_numpy()], dtype=np.int32))
    if "element" not in frame.columns:
        frame = frame.with_columns(element=np.array(["Al", "Cu", "Fe", "Ni", "Zr", "H", "O"], dtype=object)[frame["type"].to_numpy() % 7])
    return frame, {c: np.asarray(frame[c].to_numpy()) for c in frame.columns}


SAMPLES = sorted(os.path.basename(f) for f in glob.glob(os.path.join(HERE, "golden", "input_files", "*")))


def test_samples_present():
    assert len(SAMPLES) >= 8


@pytest.mark.parametrize("sample", SAMPLES)
def test_sample_files_every_writer(tmp_path, formatted, sample):
    """read on the device path (columns in HBM), written by each of the four writers: the restatement's bytes, and the host path's"""
    p, q = str(tmp_path / "dev"), str(tmp_path / "host")
    frame, cell, info = LS.read_file(os.path.join(HERE, "golden", "input_files", sample))
    frame, cols = completed(frame)
    LS.write_dump(p, frame, cell, timestep=3)
    assert open(p, "rb").read() == R.dump(cols, cell, 3) == on_host(LS.write_dump, q, frame, cell, timestep=3)
    LS.write_xyz(p, frame, cell, **info)
    assert open(p, "rb").read() == R.xyz(cols, cell, **info)
    LS.write_data(p, frame, cell, data_format="charge")
    assert open(p, "rb").read() == R.data(cols, cell, data_format="charge")
    LS.write_poscar(p, frame, cell, reduced_pos=True)
    assert open(p, "rb").read() == R.poscar(cols, cell, reduced_pos=True)
    assert open(p, "rb").read() == on_host(LS.write_poscar, q, frame, cell, reduced_pos=True)
    LS.write_xyz(p, frame, cell, classical=True)
    assert open(p, "rb").read() == R.xyz(cols, cell, classical=True) == on_host(LS.write_xyz, q, frame, cell, classical=True)
    LS.write_poscar(p, frame, cell)
    assert open(p, "rb").read() == R.poscar(cols, cell) == on_host(LS.write_poscar, q, frame, cell)
    assert len(formatted) >= 6  # every table went through the kernels
    assert on_host(LS.write_xyz, q, frame, cell, **info) == R.xyz(cols, cell, **info)
    assert on_host(LS.write_data, q, frame, cell, data_format="charge") == R.data(cols, cell, data_format="charge")


@pytest.fixture(scope="module")
def large():
    n = 200_000
    rng = np.random.default_rng(21)
    cols = {"x": rng.uniform(0, 300, n), "y": rng.uniform(0, 300, n), "z": rng.uniform(-1e-7, 1e-7, n),
            "id": rng.permutation(n).astype(np.int32) + 1, "type": rng.integers(1, 4, n).astype(np.int32),
            "cna": rng.integers(0, 5, n).astype(np.int32), "wide": np.array([0.5, -123456789.25, 1.8e19])[rng.integers(0, 3, n)]}
    cols["element"] = np.array(["Al", "Cu", "Unobtainium1"], dtype=object)[cols["type"] - 1]
    cell = Box(np.diag([300.0, 300.0, 1.0]))
    return cols, cell, R.dump(cols, cell, 0)


def test_chunk_seams_and_double_buffering(tmp_path, large, formatted):
    cols, cell, want = large
    frame = Frame(cols)
    p = str(tmp_path / "big.dump")
    LS.write_dump(p, frame, cell, timestep=0)
    assert len(formatted) == 1  # one piece
    assert open(p, "rb").read() == want
    for rows, pieces in ((4099, 49), (65536, 4)):
        del formatted[:]
        LS.write_dump(p, frame, cell, timestep=0, rows=rows)
        assert len(formatted) >= pieces
        assert open(p, "rb").read() == want, rows
    body = want[want.index(b" \n") + 2:]
    columns = {c: LS._column_spec(frame[c], True) for c in frame.columns}
    order = want[: want.index(b" \n")].split(b"ITEM: ATOMS ")[1].decode().split()
    specs = [columns[c] for c in order]
    for chunk in (1 << 12, 100_003, 1 << 25):  # pinned buffers smaller than a piece, not a divisor of anything, larger than the table
        out = io.BytesIO()
        total = _text.stream_from_device(_text.format_chunks([s[0] for s in specs], [s[1] for s in specs], [s[2] for s in specs], rows=50_000), out, chunk=chunk)
        assert total == len(body) and out.getvalue() == body, chunk
    whole = _text.format_table([s[0] for s in specs], [s[1] for s in specs], [s[2] for s in specs])
    out = io.BytesIO()
    assert _text.stream_from_device(whole, out, chunk=1 << 20) == len(body) and out.getvalue() == body


def test_unformattable_value_takes_the_host_route_for_the_whole_table(tmp_path, large, formatted):
    cols, cell, _ = large
    cols = dict(cols, wide=cols["wide"].copy())
    cols["wide"][150_000] = 1e30  # met in the 37th piece: 36 pieces are in the file by then and are taken back
    want = R.dump(cols, cell, 0)
    p = str(tmp_path / "huge.dump")
    LS.write_dump(p, Frame(cols), cell, timestep=0, rows=4099)
    assert 30 <= len(formatted) <= 40  # the device was tried, and stopped where it met the field
    assert open(p, "rb").read() == want
    del formatted[:]
    LS.write_dump(p, Frame(cols), cell, timestep=0, rows=4099, compress=True)  # a gzip stream cannot take bytes back: a scratch file does
    assert formatted and gzip.open(p + ".gz").read() == want


def test_compressed_device_write(tmp_path, large):
    cols, cell, want = large
    p = str(tmp_path / "z.dump")
    LS.write_dump(p, Frame(cols), cell, timestep=0, rows=65536, compress=True)
    assert gzip.open(p + ".gz").read() == want


def test_general_triclinic_dump_round_trip(tmp_path, formatted):
    n = 5000
    rng = np.random.default_rng(22)
    cell = Box(np.array([[30.0, 2.0, 1.0], [3.0, 28.0, -2.5], [-1.0, 4.0, 33.0]]), [1, 1, 0], [5.0, -3.0, 0.5])
    frac = rng.random((n, 3))
    pos = cell.origin + frac @ cell.box
    cols = {"x": pos[:, 0].copy(), "y": pos[:, 1].copy(), "z": pos[:, 2].copy(), "type": rng.integers(1, 3, n).astype(np.int32)}
    p = str(tmp_path / "tri.dump")
    LS.write_dump(p, Frame(cols), cell, timestep=0)
    assert formatted
    assert open(p, "rb").read() == R.dump(cols, cell, 0) == on_host(LS.write_dump, str(tmp_path / "h.dump"), Frame(cols), cell, timestep=0)
    back, cell2, _ = LS.read_dump(p)
    aligned, rotate = cell.align_to_lammps_box()
    rotated = R.moved(cols, cell.origin, rotate)
    for k, name in enumerate("xyz"):
        want = np.array([float(format(v, ".10f")) for v in rotated[k].tolist()])
        assert back[name].to_numpy().tobytes() == want.tobytes()
    assert np.array_equal(back["id"].to_numpy(), np.arange(1, n + 1))
    assert np.allclose(cell2.box, aligned.box, rtol=0, atol=1e-9) and np.array_equal(cell2.origin, np.zeros(3))
    assert np.array_equal(cell2.boundary, cell.boundary)
    inside = np.column_stack([back[c].to_numpy() for c in "xyz"]) @ np.linalg.inv(cell2.box)
    assert np.allclose(inside, frac, rtol=0, atol=1e-8)  # the rotated atoms sit where they sat in the cell
