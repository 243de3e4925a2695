"""Bond analysis and angular distribution function on the CPU: the angle step points the kernels bin against
(mdh_debug_angle_edges, host code only) against the C library's acos, and the host layer — System.cal_bond_analysis /
cal_angular_distribution_function, BondAnalysis, AngularDistributionFunction — with the neighbour build routed to the oracle
(fixture ``oracle_backend``) and ``kernels.bond_analysis`` replaced by the numpy restatement of tests/_bond_ref.py."""
import gzip
import math
import os

import numpy as np
import pytest

import _bond_ref
import mdapy_amd as mp
from mdapy_amd.build_lattice import lattice_positions

HERE = os.path.dirname(os.path.abspath(__file__))
GOLDEN = os.path.join(HERE, "golden", "bond")


def _bin(c, nbin, delta_theta):
    v = math.floor(math.acos(c) * 180.0 / _bond_ref.PI * (1.0 / delta_theta))
    return min(v, nbin - 1)


@pytest.mark.parametrize("nbin", [1, 2, 3, 7, 36, 40, 180, 1000])
def test_angle_edges_are_the_exact_step_points(nbin):
    from mdapy_amd import _lib

    delta = 180.0 / nbin
    out = np.zeros(max(nbin - 1, 1))
    assert _lib.lib().mdh_debug_angle_edges(nbin, delta, out.ctypes.data) == 0
    edges = out[: nbin - 1]
    assert np.all(np.diff(edges) > 0)
    for k, t in enumerate(edges.tolist()):
        m = nbin - 1 - k
        assert -1.0 <= t <= 1.0
        assert _bin(t, nbin, delta) < m
        if t > -1.0:
            assert _bin(math.nextafter(t, -math.inf), nbin, delta) >= m
    # every cosine's bin is the number of step points above it
    for c in np.linspace(-1, 1, 2001).tolist() + edges.tolist():
        assert _bin(c, nbin, delta) == int(np.sum(c < edges))


def test_angle_edges_reject_bad_arguments():
    from mdapy_amd import _lib

    out = np.zeros(4)
    for nbin, delta in ((0, 1.0), (5, 0.0), (5, -1.0), (5, float("nan"))):
        assert _lib.lib().mdh_debug_angle_edges(nbin, delta, out.ctypes.data) != 0


@pytest.fixture
def restated(oracle_backend, monkeypatch):
    import mdapy_amd.kernels as K

    monkeypatch.setattr(K, "bond_analysis", _bond_ref)
    return _bond_ref


def _glass(n_cells=4, seed=0):
    pos, box = lattice_positions("fcc", 4.0, n_cells, n_cells, n_cells)
    rng = np.random.default_rng(seed)
    pos = pos + rng.normal(0, 0.35, pos.shape)
    element = np.where(rng.random(len(pos)) < 0.36, "Zr", "Cu")
    return {"x": pos[:, 0], "y": pos[:, 1], "z": pos[:, 2], "element": element}, box


def _direct_adf(s, rc_dict, nbin):
    """the restatement called on the system's own list (dict order = row order, sorted element codes)"""
    names = sorted(set(s.data["element"].to_numpy().tolist()))
    codes = np.array([names.index(e) for e in s.data["element"].to_numpy().tolist()], np.int32)
    pats = np.array([[names.index(p) for p in k.split("-")] for k in rc_dict], np.int32)
    out = np.zeros((len(rc_dict), nbin), np.int64)
    cell, frame = s._get_compute_view()
    xyz = [frame[c].to_numpy() for c in "xyz"]
    if len(xyz[0]) != len(codes):
        codes = np.tile(codes, len(xyz[0]) // len(codes))
    _bond_ref.compute_adf(*xyz, cell.box, cell.origin, cell.boundary, s.verlet_list, s.distance_list, s.neighbor_number,
                          180.0 / nbin, np.array(list(rc_dict.values()), float), pats, codes, nbin, out)
    return out


def test_system_bond_analysis_shape_and_counts(restated):
    data, box = _glass()
    s = mp.System(data=data, box=box)
    ba = s.cal_bond_analysis(3.6, 50)
    assert ba.bond_length_distribution.dtype == np.int64 and ba.bond_angle_distribution.dtype == np.int64
    assert np.allclose(ba.r_length, (np.arange(50) + 0.5) * 3.6 / 50)
    assert np.allclose(ba.r_angle, (np.arange(50) + 0.5) * 180.0 / 50)
    nn = np.asarray(s.neighbor_number, np.int64)
    assert ba.bond_length_distribution.sum() * 2 == nn.sum()
    assert ba.bond_angle_distribution.sum() == int(np.sum(nn * (nn - 1) // 2))


def test_adf_dict_order_is_row_order(restated):
    data, box = _glass(seed=1)
    s = mp.System(data=data, box=box)
    rc_dict = {"Zr-Cu-Cu": [0, 3.2, 2.0, 3.6], "Cu-Cu-Zr": [0, 3.6, 0, 3.6], "Cu-Cu-Cu": [2.2, 3.0, 0.0, 3.6],
               "Zr-Zr-Cu": [0, 3.6, 0, 3.4]}
    adf = s.cal_angular_distribution_function(rc_dict, 36)
    assert adf.ele_unique == ["Cu", "Zr"]
    assert adf.bond_angle_distribution.dtype == np.int64 and adf.bond_angle_distribution.shape == (4, 36)
    assert np.allclose(adf.r_angle, (np.arange(36) + 0.5) * 5.0)
    assert np.array_equal(adf.bond_angle_distribution, _direct_adf(s, rc_dict, 36))
    flipped = dict(reversed(list(rc_dict.items())))
    again = s.cal_angular_distribution_function(flipped, 36)
    assert np.array_equal(again.bond_angle_distribution, adf.bond_angle_distribution[::-1])
    assert adf.bond_angle_distribution.sum() > 0


def test_rejected_input(restated):
    data, box = _glass()
    s = mp.System(data=data, box=box)
    with pytest.raises(ValueError):
        s.cal_bond_analysis(3.0, 0)
    with pytest.raises(ValueError):
        s.cal_bond_analysis(0.0, 10)
    with pytest.raises(ValueError):
        s.cal_bond_analysis(-1.0, 10)
    with pytest.raises(ValueError):
        s.cal_angular_distribution_function({"Cu-Cu-Cu": [0, 3.0, 0, 3.0]}, 0)
    with pytest.raises(ValueError):
        s.cal_angular_distribution_function({"Cu-Cu-Cu": [0, 0, 0, 0]}, 10)
    with pytest.raises(AssertionError):
        s.cal_angular_distribution_function({"Cu-Cu-Ni": [0, 3.0, 0, 3.0]}, 10)
    with pytest.raises(AssertionError):
        s.cal_angular_distribution_function({"Cu-Cu-Cu": [0, 3.0, 3.0]}, 10)
    with pytest.raises(AssertionError):
        s.cal_angular_distribution_function({"Cu-Cu": [0, 3.0, 0, 3.0]}, 10)
    no_element = mp.System(data={k: data[k] for k in "xyz"}, box=box)
    with pytest.raises(AssertionError):
        no_element.cal_angular_distribution_function({"Cu-Cu-Cu": [0, 3.0, 0, 3.0]}, 10)
    with pytest.raises(ValueError):
        mp.bond_analysis.BondAnalysis(s.data, s.box, 3.0, 0, None, None, None).compute()


def test_list_is_reused_when_rc_reaches(restated, monkeypatch):
    data, box = _glass()
    s = mp.System(data=data, box=box)
    s.build_neighbor(3.8)
    rows = s.verlet_list
    calls = []
    real = mp.System.build_neighbor
    monkeypatch.setattr(mp.System, "build_neighbor", lambda self, *a, **k: calls.append(a) or real(self, *a, **k))
    s.cal_bond_analysis(3.6, 30)
    s.cal_angular_distribution_function({"Cu-Zr-Zr": [0, 3.5, 0, 3.7]}, 30)
    assert calls == [] and s.verlet_list is rows
    s.cal_bond_analysis(4.0, 30)
    assert len(calls) == 1 and s.rc == 4.0
    # a k-nearest list beside a stale rc that reaches is reused too, as the reference does
    s.build_nearest_neighbor(6)
    knn_rows = s.verlet_list
    ba = s.cal_bond_analysis(3.0, 30)
    assert len(calls) == 1 and s.verlet_list is knn_rows
    assert ba.bond_angle_distribution.sum() > 0


def test_thin_box_counts_every_replica_row(restated):
    pos, box = lattice_positions("fcc", 3.615, 2, 2, 2)  # 7.23 A: a 3.7 A list is built on a replica
    rng = np.random.default_rng(5)
    pos = pos + rng.normal(0, 0.05, pos.shape)
    s = mp.System(pos=pos, box=box)
    ba = s.cal_bond_analysis(3.7, 36)
    assert "_enlarge_data" in s.__dict__
    copies = s._enlarge_box.box[0, 0] / box[0, 0], s._enlarge_box.box[1, 1] / box[1, 1], s._enlarge_box.box[2, 2] / box[2, 2]
    big_pos, big_box = s._enlarge_data.select("x", "y", "z").to_numpy(), s._enlarge_box
    big = mp.System(pos=big_pos, box=big_box)
    ref = big.cal_bond_analysis(3.7, 36)
    assert "_enlarge_data" not in big.__dict__
    assert np.array_equal(ba.bond_angle_distribution, ref.bond_angle_distribution)
    assert np.array_equal(ba.bond_length_distribution, ref.bond_length_distribution)
    assert int(round(np.prod(copies))) > 1


def _water(tmp_path):
    path = tmp_path / "water.xyz"
    with gzip.open(os.path.join(GOLDEN, "water.xyz.gz"), "rb") as src:
        path.write_bytes(src.read())
    return str(path)


# mdapy key "A-B-C" (A the centre) -> the fixture's component "B-A-C"
WATER_ADF = {"O-H-H": "H-O-H", "O-O-H": "O-O-H", "H-H-H": "H-H-H", "H-O-O": "O-H-O", "O-O-O": "O-O-O", "H-O-H": "O-H-H"}


def test_water_fixtures(restated, tmp_path):
    path = _water(tmp_path)
    want = np.load(os.path.join(GOLDEN, "bond_analysis.npz"))
    s = mp.System(path)
    bo = s.cal_bond_analysis(float(want["cutoff"]), int(want["bins"]), max_neigh=int(want["max_neigh"]))
    assert np.allclose(bo.r_length, want["r_length"]) and np.allclose(bo.r_angle, want["r_angle"])
    assert np.array_equal(bo.bond_length_distribution, want["bond_length_distribution"].astype(np.int64))
    assert np.array_equal(bo.bond_angle_distribution, want["bond_angle_distribution"].astype(np.int64))
    want = np.load(os.path.join(GOLDEN, "adf.npz"))
    s = mp.System(path)
    adf = s.cal_angular_distribution_function({k: [0, 2.0, 0, 2.0] for k in WATER_ADF}, int(want["bins"]))
    for row, name in enumerate(WATER_ADF.values()):
        assert np.array_equal(adf.bond_angle_distribution[row], want[f"adf_{name.replace('-', '_')}"].astype(np.int64)), name


def test_adf_after_an_in_place_sort_of_the_mirrored_list(restated):
    """found by ``FUZZ_TWIN=1 python tests/fuzz_system.py`` at seed 60024 (rdf_long, ..., ids, adf): an analysis that does not run
    on the cell-sorted twin sorts the front columns of the system's list in place — the list that mirrors the twin's — and the next
    ADF ran on the twin's rows, still in their old order.  A pattern with one element for both neighbours and two different
    ranges depends on the order of a row: the sort goes through the twin now, and a mirror that is out of step keeps the twin out"""
    data, box = _glass(4, seed=3)
    rc_dict = {"Cu-Cu-Cu": [0.0, 2.9, 2.0, 4.2], "Zr-Cu-Cu": [1.0, 4.2, 0.0, 3.1]}
    got = {}
    for mode in ("0", "1"):
        s = mp.System(data=dict(data), box=box)
        s._sort_mode = mode
        s.build_neighbor(4.2)
        assert (s._spatial() is not None) == (mode == "1")
        s.cal_identify_diamond_structure()  # the four nearest to the front, in place
        assert s._sorted_columns[1] >= 4
        if mode == "1":  # the twin's rows were sorted with the mirror: the two are in step and the ADF runs on the twin
            twin = s._spatial()
            assert s._mirrors_twin() and twin._sorted_columns[1] >= 4 and s._twin_for("cal_angular_distribution_function", (rc_dict, 37), {}) is twin
        got[mode] = s.cal_angular_distribution_function(rc_dict, 37).bond_angle_distribution
        want = _direct_adf(s, rc_dict, 37)
        assert np.array_equal(got[mode], want)
    assert got["0"].sum() > 1000 and np.array_equal(got["0"], got["1"])
