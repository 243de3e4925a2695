"""CHILL+ on the CPU: the host layer — ``System.cal_chill_plus``, ``ChillPlus``, list reuse, the replica of a thin box — with the
neighbour build routed to the oracle (fixture ``oracle_backend``) and ``kernels.chill_plus`` replaced by the numpy restatement
of tests/_chill_ref.py; the restatement itself against the reference's OVITO-derived fixture; and the lonsdaleite cell."""
import os

import numpy as np
import pytest

import _chill_ref
import mdapy_amd as mp
from mdapy_amd import build_lattice
from mdapy_amd.build_lattice import lattice_positions

HERE = os.path.dirname(os.path.abspath(__file__))
GOLDEN = os.path.join(HERE, "golden", "chill", "chill_water.npz")


@pytest.fixture
def restated(oracle_backend, monkeypatch):
    import mdapy_amd.kernels as K

    monkeypatch.setattr(K, "chill_plus", _chill_ref)
    return _chill_ref


def _water():
    want = np.load(GOLDEN)
    box = mp.Box(want["box"], want["boundary"])
    return mp.System(pos=want["pos"], box=box), want["chill_plus"], float(want["chill_plus_cutoff"])


def _labels(s):
    return s.data["chill_plus"].to_numpy()


def test_reference_fixture_exactly(restated):
    s, want, cutoff = _water()
    assert cutoff == 3.5 and s.N == 8000
    s.cal_chill_plus(cutoff)
    got = _labels(s)
    assert got.dtype == np.int32 and got.shape == (8000,)
    assert np.bincount(want, minlength=6).tolist() == [4392, 553, 517, 2305, 20, 213]
    assert np.array_equal(got, want)
    # the fixture keeps clear of the thresholds: no atom is ambiguous, which is what lets every test of it ask for equality
    _, c, ambiguous = _chill_ref.on_system_list(s, cutoff)
    near = np.nanmin(np.minimum(np.minimum(np.abs(c - _chill_ref.LOW), np.abs(c - _chill_ref.HIGH)), np.abs(c - _chill_ref.STAGGERED)))
    print(f"fixture: nearest approach of a bond's c to a threshold = {near:.3e}")
    assert not ambiguous.any() and near > _chill_ref.BAND


def test_default_cutoff_and_column(restated):
    s, want, _ = _water()
    assert s.cal_chill_plus() is None
    assert s.rc == 3.5 and list(s.data.columns) == ["x", "y", "z", "chill_plus"]
    assert np.array_equal(_labels(s), want)


def test_one_diamond_cell_runs_on_its_replica(restated):
    pos, box = lattice_positions("diamond", 6.37)
    s = mp.System(pos=pos, box=box)
    s.cal_chill_plus(3.5)
    assert "_enlarge_data" in s.__dict__ and s._enlarge_data.shape[0] > 8  # 6.37 < 2 x 3.5
    got = _labels(s)
    assert got.dtype == np.int32 and got.shape == (8,) and (got == 2).all()


def test_class_without_lists_builds_its_own(restated):
    s, want, cutoff = _water()
    job = mp.ChillPlus(s.data, s.box, cutoff)
    assert job.verlet_list is None and job.pattern.shape == (0,) and job.pattern.dtype == np.int32
    job.compute()
    assert job.verlet_list is not None and job.verlet_list.shape[0] == 8000 and job.cutoff == 3.5
    assert np.array_equal(np.asarray(job.pattern), want)
    assert "verlet_list" not in s.__dict__
    # the same class on a thin box: its own list is the replica's, the labels are the cell's
    pos, box = lattice_positions("diamond", 6.37)
    small = mp.System(pos=pos, box=box)
    job = mp.ChillPlus(small.data, small.box)
    job.compute()
    assert job.verlet_list.shape[0] > 8 and np.asarray(job.pattern).tolist() == [2] * 8


def test_a_longer_list_is_reused(restated):
    s, want, cutoff = _water()
    s.build_neighbor(5.0)
    rows = s.verlet_list
    assert rows.shape[1] > 16
    s.cal_chill_plus(cutoff)
    assert s.verlet_list is rows and s.rc == 5.0
    fresh, _, _ = _water()
    fresh.cal_chill_plus(cutoff)
    assert fresh.rc == 3.5
    assert np.array_equal(_labels(s), _labels(fresh)) and np.array_equal(_labels(s), want)


def test_the_noisy_ice_inputs_of_the_gpu_tests(restated):
    """documents the inputs tests/test_gpu_chill.py uses, from the yardstick alone (no coverage of the product): sigma 0.15 stays
    cubic ice throughout, sigma 0.30 gives five classes and coordinations 2 to 6, and neither has an atom within the band"""
    pos, box = lattice_positions("diamond", 6.37, 5, 5, 5)
    for sigma, seed, classes, coordinations in ((0.15, 1, [2], (4, 4)), (0.30, 2, [0, 1, 2, 3, 5], (2, 6))):
        s = mp.System(pos=pos + np.random.default_rng(seed).normal(0, sigma, pos.shape), box=box)
        s.build_neighbor(3.5)
        label, c, ambiguous = _chill_ref.on_system_list(s, 3.5)
        bonds = (~np.isnan(c)).sum(axis=1)
        assert np.flatnonzero(np.bincount(label, minlength=6)).tolist() == classes
        assert (int(bonds.min()), int(bonds.max())) == coordinations and not ambiguous.any()


def test_shuffled_atoms_run_on_the_twin(restated, monkeypatch):
    pos, box = lattice_positions("diamond", 6.37, 5, 5, 5)
    pos = pos + np.random.default_rng(2).normal(0, 0.30, pos.shape)
    order = np.random.default_rng(3).permutation(len(pos))
    monkeypatch.setenv("MDAPY_SPATIAL_SORT", "0")
    plain = mp.System(pos=pos, box=box)
    plain.cal_chill_plus()
    monkeypatch.setenv("MDAPY_SPATIAL_SORT", "1")
    s = mp.System(pos=pos[order], box=box)
    s.cal_chill_plus()
    assert s._spatial() is not None and s._twin.shown.mirror is s.verlet_list and s.rc == 3.5
    assert np.array_equal(_labels(s), _labels(plain)[order])
    # a box thinner than two cutoffs stays off the twin (the reach is read from ``cutoff``): its list is the replica's
    cell, cell_box = lattice_positions("diamond", 6.37, 3, 3, 3)  # 19.11 A
    small = mp.System(pos=cell[np.random.default_rng(4).permutation(len(cell))], box=cell_box)
    assert small._spatial() is not None and small._twin_for("cal_chill_plus", (), {}) is small._spatial()
    assert small._twin_for("cal_chill_plus", (10.0,), {}) is None and small._twin_for("cal_chill_plus", (), {"cutoff": 10.0}) is None
    small.cal_chill_plus(10.0)
    assert "_enlarge_data" in small.__dict__ and small._twin.shown is None and _labels(small).shape == (216,)


def test_lonsdaleite_cell():
    cell, basis = build_lattice.unit_cell("lonsdaleite", 4.5)
    assert np.allclose(cell, [[4.5, 0, 0], [-2.25, 2.25 * np.sqrt(3.0), 0], [0, 0, 4.5 * np.sqrt(8 / 3)]], atol=1e-15, rtol=1e-15)
    assert np.array_equal(basis, np.array([[1 / 3, 2 / 3, 0.0], [2 / 3, 1 / 3, 0.5], [1 / 3, 2 / 3, 3 / 8], [2 / 3, 1 / 3, 7 / 8]]))
    assert build_lattice.unit_cell("Lonsdaleite", 4.5, c=7.0)[0][2, 2] == 7.0
    pos, box = lattice_positions("lonsdaleite", 4.5, 3, 3, 2)
    assert pos.shape == (72, 3)
    # every site has four neighbours at the tetrahedral distance 3 c / 8
    frac = pos @ np.linalg.inv(box)
    d = frac[:, None, :] - frac[None, :, :]
    d -= np.round(d)
    dist = np.linalg.norm(d @ box, axis=2)
    bond = 0.375 * 4.5 * np.sqrt(8 / 3)
    assert ((np.abs(dist - bond) < 1e-9).sum(axis=1) == 4).all() and (dist[dist > 1e-9] > bond - 1e-9).all()


def test_lonsdaleite_is_hexagonal_ice(restated):
    pos, box = lattice_positions("lonsdaleite", 4.5, 2, 2, 2)
    s = mp.System(pos=pos, box=box)
    s.cal_chill_plus(3.5)
    assert _labels(s).tolist() == [1] * 32
