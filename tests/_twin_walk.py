"""The edges of the state machine between a ``System`` and its cell-sorted twin (mdapy_amd/_twin.py), walked in one sequence on a
MDAPY_SPATIAL_SORT=1 system and a =0 system side by side: after every step the lists and columns of the two are compared bit for
bit, WHICH calls ran on the twin is asserted (``System._run_on_twin`` watched, as tests/fuzz_system.py does) and so is the one
predicate ``System._listed_on_twin``.  tests/test_spatial_twin.py walks it over the oracle backend, tests/test_gpu_order.py over the
kernels."""
import os

import numpy as np

import mdapy_amd as mp
from mdapy_amd.build_lattice import lattice_positions
from mdapy_amd.devarray import as_numpy

LISTS = ("verlet_list", "distance_list", "neighbor_number")
ADF = {"Cu-Cu-Cu": [0.0, 2.9, 2.0, 3.8], "Zr-Cu-Cu": [1.0, 3.8, 0.0, 3.1]}  # (two different ranges: the order of a row shows)


def _pair():
    """the 7 x 6 x 6 rattled, shuffled fcc of tests/test_spatial_twin.py (1 008 atoms), with elements: analysed as it is, and on its twin"""
    pos, box = lattice_positions("fcc", 3.615, 7, 6, 6)
    rng = np.random.default_rng(3)
    pos = pos + rng.normal(0, 0.12, pos.shape)
    pos = pos[rng.permutation(len(pos))]
    element = np.where(rng.random(len(pos)) < 0.36, "Zr", "Cu")
    made = []
    before = os.environ.get("MDAPY_SPATIAL_SORT")
    try:
        for mode in ("0", "1"):
            os.environ["MDAPY_SPATIAL_SORT"] = mode
            made.append(mp.System(data={"x": pos[:, 0].copy(), "y": pos[:, 1].copy(), "z": pos[:, 2].copy(), "element": element}, box=box))
    finally:
        if before is None:
            del os.environ["MDAPY_SPATIAL_SORT"]
        else:
            os.environ["MDAPY_SPATIAL_SORT"] = before
    return made


def _same_state(p, s, where):
    assert p.N == s.N, where
    for name in LISTS + ("rc",):
        assert (name in p.__dict__) == (name in s.__dict__), (where, name)
    if "verlet_list" in p.__dict__:
        for name in LISTS:
            a, b = as_numpy(getattr(p, name)), as_numpy(getattr(s, name))
            assert a.dtype == b.dtype and np.array_equal(a, b), (where, name)
    if "rc" in p.__dict__:
        assert p.rc == s.rc, where
    assert list(p.data.columns) == list(s.data.columns), where
    for name in p.data.columns:
        a, b = p.data[name].to_numpy(), s.data[name].to_numpy()
        assert a.dtype == b.dtype and np.array_equal(a, b, equal_nan=a.dtype.kind == "f"), (where, name)


def walk():
    from fuzz_system import _watch_twin

    p, s = _pair()
    seen = set()
    _watch_twin(s, seen)

    def step(where, call, on_twin, listed):
        """``call`` on both; the calls that ran on the twin; whether the list shown is the twin's afterwards"""
        seen.clear()
        got = call(p), call(s)
        assert seen == set(on_twin), (where, seen)
        assert p._spatial() is None and p._listed_on_twin() is None
        twin = s._spatial()
        assert twin is not None and (s._listed_on_twin() is twin) == listed and s._mirrors_twin() == listed, where
        _same_state(p, s, where)
        return got

    # 1. a cutoff list, then CSP(12): the front is sorted on the twin and the mirror renewed
    step("1 build", lambda y: y.build_neighbor(3.9, max_neigh=30), {"build_neighbor"}, True)
    twin, state = s._spatial(), s._twin  # (the sorted System; the Twin that holds it)
    shown = state.shown
    assert state.system is twin and twin._twin_of() is state
    assert shown.mirror is s.verlet_list and shown.depth == 0 and s._front() == 0
    assert as_numpy(p.neighbor_number).min() >= 12  # (deep enough: the list is sorted, not replaced by a 12-nearest search)
    step("1 csp", lambda y: y.cal_centro_symmetry_parameter(12), {"cal_centro_symmetry_parameter"}, True)
    assert twin._front() == 12 and s._front() == 12 and p._front() == 12
    assert state.shown is not shown and state.shown.depth == 12 and state.shown.mirror is s.verlet_list and state.shown.rows is shown.rows
    assert s._listed_on_twin() is twin
    # 2. an angular distribution function with two different ranges runs on the twin's rows
    a, b = step("2 adf", lambda y: y.cal_angular_distribution_function(ADF, 37), {"cal_angular_distribution_function"}, True)
    assert a.bond_angle_distribution.sum() > 1000 and np.array_equal(a.bond_angle_distribution, b.bond_angle_distribution)
    assert a.bond_angle_distribution[0].sum() != a.bond_angle_distribution[1].sum()
    # 3. a 9-nearest list beside the stale rc: a bond analysis below that rc reuses it as it is, and stays off the twin
    step("3 knn", lambda y: y.build_nearest_neighbor(9), {"build_nearest_neighbor"}, True)
    assert s.rc == 3.9 and "_list_cutoff" not in s.__dict__ and s._twin_for("cal_bond_analysis", (3.0, 20), {}) is None
    a, b = step("3 bond", lambda y: y.cal_bond_analysis(3.0, 20), set(), True)
    for name in ("bond_length_distribution", "bond_angle_distribution"):
        assert getattr(a, name).sum() > 0 and np.array_equal(getattr(a, name), getattr(b, name)), name
    # 4. a cutoff list again: the twin is in use again
    step("4 build", lambda y: y.build_neighbor(3.9, max_neigh=30), {"build_neighbor"}, True)
    a, b = step("4 bond", lambda y: y.cal_bond_analysis(3.0, 20), {"cal_bond_analysis"}, True)
    assert np.array_equal(a.bond_angle_distribution, b.bond_angle_distribution)
    # 5. a list the user put there: list consumers run on the system itself, until the next build_neighbor
    def assign(y):
        y.verlet_list = as_numpy(y.verlet_list).copy()

    step("5 assign", assign, set(), False)
    step("5 cnp", lambda y: y.cal_common_neighbor_parameter(3.6), set(), False)
    step("5 csp", lambda y: y.cal_centro_symmetry_parameter(12), set(), False)
    step("5 build", lambda y: y.build_neighbor(3.9, max_neigh=30), {"build_neighbor"}, True)
    step("5 cnp again", lambda y: y.cal_common_neighbor_parameter(3.6), {"cal_common_neighbor_parameter"}, True)
    # 6. the list forgotten with the data kept: both lists are gone, the twin is the same
    step("6 reset", lambda y: y.update_data(y.data, reset_neighbor=True), set(), False)
    assert s._spatial() is twin and s._twin is state and state.shown is None
    assert not any(name in s.__dict__ or name in twin.__dict__ for name in LISTS + ("rc", "_sorted_columns", "_list_cutoff"))
    step("6 cnp", lambda y: y.cal_common_neighbor_parameter(3.6), {"cal_common_neighbor_parameter"}, True)
    # 7. a new box: a new twin
    step("7 box", lambda y: setattr(y, "box", mp.Box(y.box.box * 1.0)), set(), False)
    second = s._spatial()
    assert second is not twin and s._twin is not state and s._twin.system is second and "verlet_list" not in s.__dict__
    step("7 aja", lambda y: y.cal_ackland_jones_analysis(), {"cal_ackland_jones_analysis"}, True)
    # 8. atoms removed: a new twin of the atoms that are left, and no permutation of the old number applied
    seen.clear()
    removed = p.delete_overlap(2.3), s.delete_overlap(2.3)
    assert removed[0] == removed[1] > 0 and s.N == 1008 - removed[1] and seen == {"build_neighbor"}
    third = s._spatial()
    assert third is not None and third is not second and third.N == s.N
    assert np.array_equal(np.sort(np.asarray(as_numpy(third._perm))), np.arange(s.N))
    _same_state(p, s, "8 delete")
    assert "verlet_list" not in s.__dict__ and s._listed_on_twin() is None
    step("8 cna", lambda y: y.cal_common_neighbor_analysis(rc=0.854 * 3.615), {"cal_common_neighbor_analysis"}, True)
    step("8 csp", lambda y: y.cal_centro_symmetry_parameter(12), {"cal_centro_symmetry_parameter"}, True)
