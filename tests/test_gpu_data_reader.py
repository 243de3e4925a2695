"""The LAMMPS data-file reader's device path: the file streamed into HBM once, its section lines found by ``mdh_scan_sections``,
both tables tokenised where they lie and the Velocities rows joined by ``mdh_match_ids``.

Yardsticks: the plain-Python restatement (tests/_data_ref.py), the package's own host reader (the same ``_data_frame`` body over
bytes on the host), the scan's host twin, and a dict for the join.  Every comparison is of bit patterns."""
import os

import numpy as np
import pytest

import _data_cases as C
import _data_ref as R
import _readers
import mdapy_amd as mp
from mdapy_amd import _lib, _text, kernels
from mdapy_amd import load_save as LS
from mdapy_amd.devarray import HArray

pytestmark = pytest.mark.gpu


@pytest.fixture(autouse=True)
def _need_gpu():
    if _lib.device_count() < 1:
        pytest.fail("test_gpu_data_reader needs a HIP device")


@pytest.fixture
def host_readers(monkeypatch):
    """how many times the host reader was asked: once by _readers.both itself, twice when the device path handed the file over"""
    made = []
    real = LS._HostText

    class Counted(real):
        def __init__(self, path):
            made.append(path)
            super().__init__(path)

    monkeypatch.setattr(LS, "_HostText", Counted)
    return made


def _against_ref(got, path):
    cols, box, _ = R.read_data(path)
    frame = got[0]
    assert frame.columns == list(cols)
    for c in frame.columns:
        a = frame[c].to_numpy()
        if cols[c].dtype == object:
            assert list(a) == list(cols[c]), c
        else:
            assert a.dtype == cols[c].dtype and a.tobytes() == cols[c].tobytes(), c
    assert np.asarray(got[1].box).tobytes() == box[:3].tobytes() and np.asarray(got[1].origin, dtype=np.float64).tobytes() == box[3].tobytes()


@pytest.mark.parametrize("name", sorted(C.GOOD) + ["sample", "gz", "lmp"])
def test_device_and_host_give_the_same_frame(name, tmp_path, monkeypatch, host_readers):
    if name == "sample":
        path = C.SAMPLE
    elif name == "gz":
        path = C.write(tmp_path, name, C.CHARGE_VELOCITIES, ".data.gz")
    elif name == "lmp":
        path = C.write(tmp_path, name, C.MASSES_BETWEEN, ".lmp")
    else:
        path = C.write(tmp_path, name, C.GOOD[name])
    dev, host = _readers.both(path, monkeypatch)
    _readers.same(dev, host)
    _against_ref(dev, path)
    assert list(dev[1].boundary) == [1, 1, 1]
    # a Velocities table cut short is the host reader's to judge; everything else is read in HBM
    assert len(host_readers) == (2 if name == "short_velocities" else 1)
    if name != "short_velocities":
        assert all(isinstance(dev[0][c]._dev, HArray) for c in dev[0].columns if c != "element")


@pytest.mark.parametrize("name", sorted(C.BAD))
def test_errors_are_the_host_readers(name, tmp_path, monkeypatch):
    path = C.write(tmp_path, name, C.BAD[name])
    with pytest.raises(C.KIND[name]) as want:
        R.read_data(path)
    monkeypatch.setattr(LS, "DEVICE_MIN_BYTES", 0)
    with pytest.raises(C.KIND[name]) as got:
        LS.read_file(path)
    assert type(got.value) is C.KIND[name] and str(got.value) == str(want.value) and C.WORDING[name] in str(got.value)


# ---- the scan kernel against its host twin
def _on_device(raw):
    t = _text.torch()
    return t.from_numpy(np.frombuffer(raw, dtype=np.uint8).copy()).cuda()


def _scan_both(raw, restated=True):
    want = _text.scan_sections(raw, R.WORDS)
    assert not restated or want == R.section_offsets(raw)
    assert _text.scan_sections(_on_device(raw), R.WORDS) == want
    return want[0]


def _padded(at):
    """comment lines that fill exactly ``at`` bytes"""
    full, rest = divmod(at, 61)
    return (b"#" * 60 + b"\n") * full + (b"#" * (rest - 1) + b"\n" if rest else b"")


@pytest.mark.parametrize("at", [15, 16, 17, 4095, 4096, 4097])
def test_scan_kernel_placement(at):
    for word in ("Atoms", "Masses", "Velocities"):
        for rest in (b"\n\n1 1 0 0 0\n", b" # x\n", b"\r\n1 2 3\n", b""):
            raw = _padded(at) + word.encode() + rest
            assert _scan_both(raw) == {word: at}
        assert _scan_both(_padded(at - 3) + b" \t " + word.encode() + b"\n") == {word: at - 3}  # the token itself at `at`, its line 3 earlier
        assert _scan_both(_padded(at) + word.encode() + b"x\n" + word.encode() + b"#\n# " + word.encode() + b"\n") == {}
    # the three of them around one boundary, and a second `Atoms` that must not win
    raw = _padded(at) + b"Velocities\n" + _padded(4096 - 11) + b"Atoms # atomic\n1 1 0 0 0\nMasses\n" + _padded(8192) + b"Atoms\nMasses"
    assert _scan_both(raw) == {"Velocities": at, "Atoms": at + 4096, "Masses": at + 4096 + 25}


def test_scan_kernel_edges():
    assert _scan_both(b"Atoms") == {"Atoms": 0} and _scan_both(b"\n") == {} and _scan_both(b"Atoms\r") == {"Atoms": 0}
    assert _scan_both(_padded(5000) + b"1 1 0 0 0\nBonds") == {"Bonds": 5010}  # the last line, without a line feed
    for at in (1023, 1024, 1025):  # a wavefront's 1 KB: its first lane reads the byte before, the others are handed it
        assert _scan_both(_padded(at) + b"Atoms\n" + _padded(1024 - 6) + b"Masses\n") == {"Atoms": at, "Masses": at + 1024}
    far = (16 << 20) + 4097  # past what one pass of the kernel's workgroups covers: they stride on
    assert _scan_both(_padded(far) + b"Velocities\n1 0 0 0\n" + _padded(70000) + b"Atoms", restated=False) == {"Velocities": far, "Atoms": far + 70019}
    every = b"".join(w.encode() + b" x\n" + _padded(int(k) * 37) for k, w in enumerate(R.WORDS))
    assert len(_scan_both(every)) == len(R.WORDS)
    rng = np.random.default_rng(3)
    pieces = [w.encode() for w in R.WORDS] + [b" ", b"\t", b"\r", b"\n", b"\n", b"#", b"1 2 3", b"x", b"Atomsx", b"-0.5"]
    _scan_both(b"".join(pieces[k] for k in rng.integers(0, len(pieces), 6000)))
    view = _on_device(b"xy" + b"Masses\n" + b"Atoms\n")[2:]  # a text that does not start at an aligned address
    assert _text.scan_sections(view, R.WORDS) == ({"Masses": 0, "Atoms": 7}, 2)


# ---- the join
def _dict_join(want, have):
    rows = {}
    for r, a in enumerate(have.tolist()):
        rows[a] = r
    out = np.array([rows.get(a, -1) for a in want.tolist()], dtype=np.int32)
    missing = np.flatnonzero(out < 0)
    return out, len(missing), (int(missing[0]) if len(missing) else -1), int((out != np.arange(len(out))).sum())


def _check_join(want, have, path=None):
    want, have = np.asarray(want, dtype=np.int32), np.asarray(have, dtype=np.int32)
    exp = _dict_join(want, have)
    row_of, misses, first, moved = kernels.order.match_ids(HArray.from_numpy(want), HArray.from_numpy(have))
    assert isinstance(row_of, HArray) and row_of.dtype == np.int32
    assert np.array_equal(row_of.numpy(), exp[0]) and (misses, first, moved) == exp[1:]
    if path is not None:  # which of the two ways the library took
        status, rows = np.zeros(4, np.int64), HArray.empty((len(want),), np.int32)
        a, b = HArray.from_numpy(want), HArray.from_numpy(have)
        _lib.check(_lib.lib().mdh_match_ids(a.data_ptr(), b.data_ptr(), len(want), rows.data_ptr(), status.ctypes.data, _lib.DEVICE, None))
        _text.torch().cuda.synchronize()
        assert int(status[3]) == (1 if path == "sort" else 0)


@pytest.mark.parametrize("n", [1, 63, 64, 65, 257])
def test_match_ids_against_a_dict(n):
    rng = np.random.default_rng(n)
    ids = np.arange(1, n + 1)
    _check_join(ids, ids, "table")  # identity: nothing moves
    assert kernels.order.match_ids(HArray.from_numpy(ids.astype(np.int32)), HArray.from_numpy(ids.astype(np.int32)))[3] == 0
    _check_join(ids, ids[::-1].copy(), "table")
    perm = rng.permutation(n)
    _check_join(ids, ids[perm], "table")
    _check_join(ids[rng.permutation(n)], ids[perm], "table")
    _check_join(ids + 10 ** 9, (ids + 10 ** 9)[perm], "table")
    _check_join(ids - n // 2 - 5, (ids - n // 2 - 5)[perm], "table")  # negative ids
    _check_join(-ids - 2 * 10 ** 9 + n + 5, (-ids - 2 * 10 ** 9 + n + 5)[perm], "table")
    if n > 1:
        for span, path in ((4 * n, "table"), (4 * n + 1, "sort")):  # max - min = span - 1: just below 4 N, and 4 N itself
            sparse = np.concatenate([[0, span - 1], rng.choice(np.arange(1, span - 1), n - 2, replace=False)]) - 7
            _check_join(sparse[rng.permutation(n)], sparse[rng.permutation(n)], path)
        wide = np.concatenate([[-2 ** 31, 2 ** 31 - 1], rng.integers(-2 ** 31, 2 ** 31, n - 2)])
        _check_join(wide[rng.permutation(n)], wide[perm], "sort")
        for scale, path in ((1, "table"), (50, "sort")):
            dup = rng.integers(0, n // 2 + 1, n) * scale  # duplicates in `have`: the last row wins; some ids of `want` have no row
            dup[0], dup[-1] = 0, (n // 2) * scale
            _check_join(rng.integers(0, n // 2 + 1, n) * scale, dup, path if n > 2 else None)
            one = ids[perm] * scale  # one miss, then several; the smallest missing index is reported
            want = ids * scale
            want[n // 2] = n * scale + 3
            _check_join(want, one, path if n > 2 else None)
            want[[0, n - 1]] = [-5, n * scale + 9]
            _check_join(want, one, path if n > 2 else None)
            assert kernels.order.match_ids(HArray.from_numpy(want.astype(np.int32)), HArray.from_numpy(one.astype(np.int32)))[1:3] == (3 if n > 2 else 2, 0)
    else:
        _check_join([5], [6])
        _check_join([-3], [-3], "table")


def test_match_ids_beyond_one_pass_of_the_grid():
    n = 2048 * 256 + 77  # the kernels' workgroups stride over the rows from here on
    rng = np.random.default_rng(9)
    have = rng.permutation(n).astype(np.int32) + 3
    have[rng.integers(0, n, 50)] = have[rng.integers(0, n, 50)]  # some ids twice, so some are gone
    want = rng.permutation(n).astype(np.int32) + 3
    want[n - 1] = -1
    _check_join(want, have, "table")
    _check_join(want.astype(np.int64) * 5 - 10 ** 6, have.astype(np.int64) * 5 - 10 ** 6, "sort")


def test_match_ids_host_arrays_and_empty():
    ids = np.arange(100, dtype=np.int32)
    row_of, misses, first, moved = kernels.order.match_ids(ids, ids[::-1].copy())
    assert isinstance(row_of, np.ndarray) and np.array_equal(row_of, ids[::-1]) and (misses, first, moved) == (0, -1, 100)
    row_of, misses, first, moved = kernels.order.match_ids(HArray.from_numpy(ids[:0]), HArray.from_numpy(ids[:0]))
    assert len(row_of) == 0 and (misses, first, moved) == (0, -1, 0)


# ---- one file at its real size
N_BIG = 200_000


@pytest.fixture(scope="module")
def big_file(tmp_path_factory):
    """charge style with image flags, Masses after Atoms, Velocities shuffled; every 97th row has a coordinate written with 20
    digits and every 97th velocity row a nan: fields the device hands back to the host's float()"""
    rng = np.random.default_rng(2024)
    n, edge = N_BIG, 133.0
    pos = rng.random((n, 3)) * edge
    kinds = rng.integers(1, 4, n)
    q = rng.choice([-1.0, 0.0, 1.0], n)
    img = rng.integers(-2, 3, (n, 3))
    vel = rng.normal(0.0, 2.0, (n, 3))
    ids = rng.permutation(n) + 1
    rows = list(map("%d %d %.1f %.6f %.6f %.6f %d %d %d".__mod__, zip(ids.tolist(), kinds.tolist(), q.tolist(), *pos.T.tolist(), *img.T.tolist())))
    for i in range(0, n, 97):
        xyz = ["%.6f" % v for v in pos[i]]
        xyz[(i // 97) % 3] = "%.20f" % pos[i, (i // 97) % 3]
        rows[i] = f"{ids[i]} {kinds[i]} {q[i]:.1f} {xyz[0]} {xyz[1]} {xyz[2]} {img[i, 0]} {img[i, 1]} {img[i, 2]}"
    order = rng.permutation(n)
    vrows = list(map("%d %.6f %.6f %.6f".__mod__, zip(ids[order].tolist(), *vel[order].T.tolist())))
    for k in range(5, n, 97):
        v = ["%.6f" % x for x in vel[order[k]]]
        v[k % 3] = "nan"
        vrows[k] = f"{ids[order[k]]} {v[0]} {v[1]} {v[2]}"
    text = (f"# generated\n\n{n} atoms\n3 atom types\n\n0.0 {edge} xlo xhi\n0.0 {edge} ylo yhi\n0.0 {edge} zlo zhi\n\nAtoms # charge\n\n"
            + "\n".join(rows) + "\n\nMasses\n\n1 26.9815 # Al\n2 63.546 # Cu\n3 55.845 # Fe\n\nVelocities\n\n" + "\n".join(vrows) + "\n")
    path = str(tmp_path_factory.mktemp("data") / "big.data")
    with open(path, "w") as f:
        f.write(text)
    return path


def test_big_file_at_its_real_size(big_file, monkeypatch, host_readers):
    assert os.path.getsize(big_file) > 8 * LS.DEVICE_MIN_BYTES
    s = mp.System(big_file)
    assert host_readers == [] and s.N == N_BIG
    frame = s.data
    assert frame.columns == ["id", "type", "q", "x", "y", "z", "ix", "iy", "iz", "vx", "vy", "vz", "element"]
    sample = np.sort(np.random.default_rng(1).choice(N_BIG, 5000, replace=False))
    sample[0], sample[-1] = 0, N_BIG - 1
    cols, box, _ = R.read_data(big_file, sample=sample.tolist())
    for c in ("x", "vx", "id"):  # in HBM, and nobody has copied them down: the comparisons below read other copies
        assert isinstance(frame[c]._dev, HArray) and frame[c]._host_arr is None and frame[c]._dev._host is None, c
    for c in frame.columns:
        col = frame[c]
        got = col.to_numpy()[sample] if c == "element" else col._dev.dev()[_text.torch().as_tensor(sample, device="cuda")].cpu().numpy()
        if c == "element":
            assert list(got) == list(cols[c])
        else:
            assert got.dtype == cols[c].dtype and got.tobytes() == cols[c].tobytes(), c
    assert int(np.isnan(cols["vx"]).sum() + np.isnan(cols["vy"]).sum() + np.isnan(cols["vz"]).sum()) > 20
    for c in ("x", "vx", "id"):
        assert frame[c]._host_arr is None and frame[c]._dev._host is None, c
    s.build_neighbor(rc=3.0, max_neigh=40)
    assert np.asarray(s.neighbor_number).shape == (N_BIG,) and 5 < float(np.asarray(s.neighbor_number).mean()) < 15
    with monkeypatch.context() as m:
        m.setattr(LS, "have_gpu", lambda: False)
        host = LS.read_file(big_file)
    assert len(host_readers) == 1
    _readers.same((frame, s.box, s.global_info), host)


def test_atoms_beyond_the_first_mib_takes_the_host_reader(tmp_path, monkeypatch, host_readers):
    text = C.MASSES_BETWEEN.replace("2 atoms\n", "2 atoms\n" + _padded((1 << 20) + 100).decode())
    path = C.write(tmp_path, "late_atoms", text)
    assert os.path.getsize(path) >= LS.DEVICE_MIN_BYTES
    dev = LS.read_file(path)
    assert len(host_readers) == 1  # the device path saw where `Atoms` starts and handed the file over
    _against_ref(dev, path)
    with monkeypatch.context() as m:
        m.setattr(LS, "have_gpu", lambda: False)
        _readers.same(dev, LS.read_file(path))
    early = C.write(tmp_path, "early_atoms", C.MASSES_BETWEEN + _padded((1 << 20) + 100).decode())
    got = LS.read_file(early)
    assert len(host_readers) == 2  # (this one stayed in HBM)
    _against_ref(got, early)
