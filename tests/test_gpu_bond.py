"""Bond analysis and angular distribution function on the GPU (mdapy_amd/csrc/bond.hip): every histogram bit for bit against
the numpy restatement of the reference (tests/_bond_ref.py) on the list the System built — the perfect-lattice angles that sit
exactly on bin edges included — and the reference's own water fixtures through System."""
import gzip
import os

import numpy as np
import pytest

import _bond_ref
import mdapy_amd as mp
from mdapy_amd.build_lattice import lattice_positions
from mdapy_amd.devarray import as_numpy

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
GOLDEN = os.path.join(HERE, "golden", "bond")


@pytest.fixture(autouse=True)
def _need_gpu():
    from mdapy_amd import _lib

    if _lib.device_count() < 1:
        pytest.fail("test_gpu_bond needs a HIP device")
    yield
    _lib.lib().mdh_debug_set_bond_variant(0)


def _lists(s):
    return as_numpy(s.verlet_list), as_numpy(s.distance_list), as_numpy(s.neighbor_number)


def _ref_bond(s, rc, nbin):
    cell, frame = s._get_compute_view()
    lengths, angles = np.zeros(nbin, np.int64), np.zeros(nbin, np.int64)
    _bond_ref.compute_bond(*(frame[c].to_numpy() for c in "xyz"), cell.box, cell.origin, cell.boundary, *_lists(s), lengths, angles,
                           rc / nbin, 180.0 / nbin, rc, nbin)
    return lengths, angles


def _ref_adf(s, rc_dict, nbin):
    cell, frame = s._get_compute_view()
    names = sorted(set(s.data["element"].to_numpy().tolist()))
    lut = {n: k for k, n in enumerate(names)}
    codes = np.array([lut[e] for e in frame["element"].to_numpy().tolist()], np.int32)
    pats = np.array([[lut[p] for p in k.split("-")] for k in rc_dict], np.int32)
    out = np.zeros((len(rc_dict), nbin), np.int64)
    _bond_ref.compute_adf(*(frame[c].to_numpy() for c in "xyz"), cell.box, cell.origin, cell.boundary, *_lists(s), 180.0 / nbin,
                          np.array(list(rc_dict.values()), float), pats, codes, nbin, out)
    return out


def _check_bond(s, rc, nbin):
    ba = s.cal_bond_analysis(rc, nbin)
    lengths, angles = _ref_bond(s, rc, nbin)
    assert ba.bond_length_distribution.dtype == np.int64
    assert np.array_equal(ba.bond_length_distribution, lengths)
    assert np.array_equal(ba.bond_angle_distribution, angles)
    return ba


def _check_adf(s, rc_dict, nbin):
    adf = s.cal_angular_distribution_function(rc_dict, nbin)
    assert np.array_equal(adf.bond_angle_distribution, _ref_adf(s, rc_dict, nbin))
    return adf


A = 3.615


@pytest.mark.parametrize("nbin", [36, 40, 180])
def test_fcc_knife_edges(nbin):
    pos, box = lattice_positions("fcc", A, 5, 5, 5)
    s = mp.System(pos=pos, box=box)
    ba = _check_bond(s, 0.854 * A, nbin)
    # the perfect lattice's 60 / 90 / 120 degree triplets land on both sides of bin edges: the split is the reference's
    if nbin == 40:
        assert ba.bond_angle_distribution[19] == 2160 and ba.bond_angle_distribution[20] == 3840
    if nbin == 180:
        got = ba.bond_angle_distribution
        assert (got[59], got[60], got[89], got[90], got[119], got[120]) == (5760, 6240, 2160, 3840, 4848, 7152)
    rattled = pos + np.random.default_rng(nbin).normal(0, 0.05, pos.shape)
    _check_bond(mp.System(pos=rattled, box=box), 0.854 * A, nbin)


def test_bcc_triclinic_open_and_gas():
    pos, box = lattice_positions("bcc", 2.87, 6, 6, 6)
    _check_bond(mp.System(pos=pos, box=box), 2.87 * 1.2, 180)
    pos, box = lattice_positions("fcc", A, 6, 6, 6)
    sheared = np.array(box, float)[:3].copy()
    sheared[1, 0] = 0.3 * sheared[1, 1]
    sheared[2, 0], sheared[2, 1] = 0.2 * sheared[2, 2], -0.15 * sheared[2, 2]
    frac = pos @ np.linalg.inv(np.array(box, float)[:3])
    tri = frac @ sheared + np.random.default_rng(1).normal(0, 0.04, pos.shape)
    _check_bond(mp.System(pos=tri, box=mp.Box(sheared)), 3.1, 90)
    _check_bond(mp.System(pos=pos, box=mp.Box(np.array(box, float)[:3], [0, 0, 0])), 3.1, 180)
    gas = np.random.default_rng(2).random((3000, 3)) * 25.0
    _check_bond(mp.System(pos=gas, box=25.0), 3.0, 60)


def _glass(cells, seed):
    pos, box = lattice_positions("fcc", 4.0, cells, cells, cells)
    rng = np.random.default_rng(seed)
    pos = pos + rng.normal(0, 0.35, pos.shape)
    element = np.where(rng.random(len(pos)) < 0.36, "Zr", "Cu")
    return {"x": pos[:, 0], "y": pos[:, 1], "z": pos[:, 2], "element": element}, box


CUZR = {"Cu-Cu-Cu": [0, 3.0, 2.4, 3.3], "Cu-Zr-Zr": [2.5, 3.3, 0, 3.1], "Zr-Cu-Cu": [0, 3.3, 0, 2.8], "Zr-Zr-Zr": [0, 3.3, 0, 3.3],
        "Cu-Cu-Zr": [0, 3.3, 0, 3.3], "Zr-Zr-Cu": [2.6, 3.3, 0, 3.0]}


def test_cuzr_glass_patterns_with_row_order():
    data, box = _glass(40, 0)  # 256 000 atoms
    s = mp.System(data=data, box=box)
    adf = _check_adf(s, CUZR, 72)
    assert adf.bond_angle_distribution.sum() > 0


def test_wide_rows_both_paths_and_many_patterns():
    rng = np.random.default_rng(3)
    pos = rng.random((1000, 3)) * 14.0
    el = np.where(rng.random(1000) < 0.5, "A", "B")
    s = mp.System(data={"x": pos[:, 0], "y": pos[:, 1], "z": pos[:, 2], "element": el}, box=14.0)
    s.build_neighbor(4.6)
    assert s.verlet_list.shape[1] > 128
    from mdapy_amd import _lib

    rc_dict = {"A-A-B": [0, 4.6, 1.0, 3.0], "B-B-B": [0.5, 4.0, 0, 4.6]}
    for variant in (0, 1):  # 1: every row through the wide-row path
        assert _lib.lib().mdh_debug_set_bond_variant(variant) == 0
        _check_bond(s, 4.6, 45)
        _check_adf(s, rc_dict, 45)
    _lib.lib().mdh_debug_set_bond_variant(0)
    # 40 patterns (two launches of 32 role bits), 3 x 3000 bins (histogram and step points in HBM)
    keys = [f"{a}-{b}-{c}" for a in "AB" for b in "AB" for c in "AB"]
    ordered = [(keys[m % 8], [0.1 * m, 4.6, 0.0, 4.6 - 0.05 * m]) for m in range(40)]
    from mdapy_amd import _bond_analysis

    cell, frame = s._get_compute_view()
    names = ["A", "B"]
    codes = np.array([names.index(e) for e in frame["element"].to_numpy().tolist()], np.int32)
    pats = np.array([[names.index(p) for p in k.split("-")] for k, _ in ordered], np.int32)
    ranges = np.array([r for _, r in ordered], float)
    xyz = [frame[c].to_numpy() for c in "xyz"]
    for nbin in (30, 3000):
        got = np.zeros((40, nbin), np.int64)
        want = np.zeros((40, nbin), np.int64)
        _bond_analysis.compute_adf(*xyz, cell.box, cell.origin, cell.boundary, s.verlet_list, s.distance_list, s.neighbor_number,
                                   180.0 / nbin, ranges, pats, codes, nbin, got)
        _bond_ref.compute_adf(*xyz, cell.box, cell.origin, cell.boundary, *_lists(s), 180.0 / nbin, ranges, pats, codes, nbin, want)
        assert np.array_equal(got, want)
    _check_bond(s, 4.6, 3000)


def test_duplicate_atoms_count_no_nan_triplet():
    pos, box = lattice_positions("fcc", A, 4, 4, 4)
    dup = np.vstack([pos, pos[:5]])
    s = mp.System(pos=dup, box=box)
    ba = _check_bond(s, 0.854 * A, 36)
    nn = np.asarray(as_numpy(s.neighbor_number), np.int64)
    assert ba.bond_angle_distribution.sum() < int(np.sum(nn * (nn - 1) // 2))  # the zero-distance triplets are left out


def test_shims_add_into_the_callers_arrays():
    from mdapy_amd import _bond_analysis

    pos, box = lattice_positions("fcc", A, 4, 4, 4)
    s = mp.System(pos=pos, box=box)
    s.build_neighbor(3.1)
    v, d, n = _lists(s)
    x, y, z = (np.ascontiguousarray(pos[:, k]) for k in range(3))
    args = (x, y, z, s.box.box, s.box.origin, s.box.boundary, v, d, n)
    once = [np.zeros(36, np.int64), np.zeros(36, np.int64)]
    _bond_analysis.compute_bond(*args, *once, 3.1 / 36, 5.0, 3.1, 36)
    for dtype in (np.int32, np.int64):
        acc = [np.full(36, 7, dtype), np.full(36, 7, dtype)]
        _bond_analysis.compute_bond(*args, *acc, 3.1 / 36, 5.0, 3.1, 36)
        assert acc[0].dtype == dtype and np.array_equal(acc[0], once[0] + 7) and np.array_equal(acc[1], once[1] + 7)
    near = np.full(36, 2**31 - 10, np.int32)
    keep = near.copy()
    with pytest.raises(OverflowError):
        _bond_analysis.compute_bond(*args, np.zeros(36, np.int32), near, 3.1 / 36, 5.0, 3.1, 36)
    assert np.array_equal(near, keep)
    codes = np.zeros(len(x), np.int32)
    h = np.full((1, 36), 3, np.int32)
    _bond_analysis.compute_adf(*args, 5.0, np.array([[0, 3.1, 0, 3.1]]), np.array([[0, 0, 0]], np.int32), codes, 36, h)
    assert np.array_equal(h[0], once[1] + 3)
    with pytest.raises(OverflowError):
        _bond_analysis.compute_adf(*args, 5.0, np.array([[0, 3.1, 0, 3.1]]), np.array([[0, 0, 0]], np.int32), codes, 36,
                                   np.full((1, 36), 2**31 - 10, np.int32))


WATER_ADF = {"O-H-H": "H-O-H", "O-O-H": "O-O-H", "H-H-H": "H-H-H", "H-O-O": "O-H-O", "O-O-O": "O-O-O", "H-O-H": "O-H-H"}


def test_water_fixtures_through_system(tmp_path):
    path = tmp_path / "water.xyz"
    with gzip.open(os.path.join(GOLDEN, "water.xyz.gz"), "rb") as src:
        path.write_bytes(src.read())
    want = np.load(os.path.join(GOLDEN, "bond_analysis.npz"))
    bo = mp.System(str(path)).cal_bond_analysis(float(want["cutoff"]), int(want["bins"]), max_neigh=int(want["max_neigh"]))
    assert np.array_equal(bo.bond_length_distribution, want["bond_length_distribution"].astype(np.int64))
    assert np.array_equal(bo.bond_angle_distribution, want["bond_angle_distribution"].astype(np.int64))
    want = np.load(os.path.join(GOLDEN, "adf.npz"))
    adf = mp.System(str(path)).cal_angular_distribution_function({k: [0, 2.0, 0, 2.0] for k in WATER_ADF}, int(want["bins"]))
    for row, name in enumerate(WATER_ADF.values()):
        assert np.array_equal(adf.bond_angle_distribution[row], want[f"adf_{name.replace('-', '_')}"].astype(np.int64)), name


def test_shuffled_frame_on_the_twin_equals_the_plain_one(monkeypatch):
    data, box = _glass(40, 7)
    order = np.random.default_rng(8).permutation(len(data["x"]))
    data = {k: np.asarray(v)[order] for k, v in data.items()}
    got = {}
    for mode in ("0", "1"):
        monkeypatch.setenv("MDAPY_SPATIAL_SORT", mode)
        s = mp.System(data=data, box=box)
        ba = s.cal_bond_analysis(3.3, 90)
        adf = s.cal_angular_distribution_function(CUZR, 90)
        if mode == "1":
            assert s._spatial() is not None
        got[mode] = (ba.bond_length_distribution, ba.bond_angle_distribution, adf.bond_angle_distribution)
    for a, b in zip(got["0"], got["1"]):
        assert np.array_equal(a, b)


def test_device_positions_equal_host_positions():
    import torch

    from mdapy_amd.devarray import HArray
    from mdapy_amd.frame import Frame

    pos, box = lattice_positions("fcc", A, 10, 10, 10)
    pos = pos + np.random.default_rng(4).normal(0, 0.08, pos.shape)
    host = mp.System(pos=pos, box=box).cal_bond_analysis(3.1, 180)
    cols = {c: HArray(torch.from_numpy(np.ascontiguousarray(pos[:, k])).cuda()) for k, c in enumerate("xyz")}
    dev = mp.System(data=Frame(cols), box=box).cal_bond_analysis(3.1, 180)
    assert np.array_equal(host.bond_angle_distribution, dev.bond_angle_distribution)
    assert np.array_equal(host.bond_length_distribution, dev.bond_length_distribution)


def test_ten_million_atoms_count_every_triplet_once():
    import torch

    from mdapy_amd.devarray import HArray
    from mdapy_amd.frame import Frame

    cells = 136
    base = torch.tensor([[0.0, 0.0, 0.0], [0.5, 0.5, 0.0], [0.0, 0.5, 0.5], [0.5, 0.0, 0.5]], dtype=torch.float64, device="cuda") * A
    ix = torch.arange(cells, dtype=torch.float64, device="cuda") * A
    g = torch.Generator(device="cuda")
    g.manual_seed(11)
    cols = {}
    for k, c in enumerate("xyz"):
        shape = [1, 1, 1, 1]
        shape[k] = cells
        comp = (base[:, k].view(1, 1, 1, 4) + ix.view(shape)).expand(cells, cells, cells, 4).reshape(-1)
        cols[c] = HArray((comp + torch.randn(comp.shape, generator=g, dtype=torch.float64, device="cuda") * 0.05).contiguous())
    s = mp.System(data=Frame(cols), box=mp.Box(np.diag([A * cells] * 3)))
    one = s.cal_bond_analysis(3.087, 180)
    two = s.cal_bond_analysis(3.087, 180)
    nn = s.neighbor_number.dev().to(torch.int64) if hasattr(s.neighbor_number, "dev") else torch.as_tensor(as_numpy(s.neighbor_number))
    assert int(one.bond_angle_distribution.sum()) == int((nn * (nn - 1) // 2).sum())
    assert int(one.bond_length_distribution.sum()) * 2 == int(nn.sum())
    assert np.array_equal(one.bond_angle_distribution, two.bond_angle_distribution)
    assert np.array_equal(one.bond_length_distribution, two.bond_length_distribution)
