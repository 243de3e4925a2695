"""``System.create_bonds`` and ``System.cal_chemical_species`` without a GPU: the host layer run through the oracle backend with
``kernels.build_bond`` replaced by the numpy restatement of tests/_bond_pairs_ref.py (the clustering is then the oracle's) — the
four cases of the reference's tests/test_build_bond.py with the reference's values, every assertion of the cutoff normaliser,
the bonds forgotten with the list, the formula parser, the water frame — and the argument checks of the real shim, which come
before any device work."""
import ctypes
import gzip
import os

import numpy as np
import pytest

import _bond_pairs_ref as ref
import mdapy_amd as mp
from mdapy_amd import _build_bond, vdw_radii  # noqa: F401  (what this file is about)
from mdapy_amd.system import _normalize_bond_cutoff, _parse_formula

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "bond")


@pytest.fixture
def restated(oracle_backend, monkeypatch):
    import mdapy_amd.kernels as K

    monkeypatch.setattr(K, "build_bond", ref)
    return ref


def _line(**extra):
    data = {"x": [0.0, 1.0, 2.3, 5.0], "y": [0.0] * 4, "z": [0.0] * 4}
    data.update(extra)
    return mp.System(data=data, box=mp.Box([10.0, 10.0, 10.0], boundary=[0, 0, 0]))


# ---- the reference's four cases
def test_scalar_cutoff(restated):
    system = _line(type=[1, 2, 2, 1])
    bond = system.create_bonds(1.5)
    want = np.array([[0, 1], [1, 2]], np.int32)
    assert bond.dtype == np.int32 and np.array_equal(bond, want) and np.array_equal(system.bond, want)


def test_type_pair_cutoff(restated):
    bond = _line(type=[1, 2, 2, 1]).create_bonds({(1, 1): 0.5, (1, 2): 1.1, (2, 2): 1.2})
    assert np.array_equal(bond, np.array([[0, 1]], np.int32))


def test_element_pair_cutoff(restated):
    bond = _line(element=["Cu", "Zr", "Zr", "Cu"]).create_bonds({("Cu", "Cu"): 0.5, ("Cu", "Zr"): 1.1, ("Zr", "Zr"): 1.2})
    assert np.array_equal(bond, np.array([[0, 1]], np.int32))


def test_small_periodic_box_goes_through_the_replica(restated):
    system = mp.System(pos=np.array([[0.0, 0.0, 0.0], [1.0, 0.0, 0.0]]), box=mp.Box([2.0, 2.0, 2.0]))
    bond = system.create_bonds(1.1)
    assert "_enlarge_data" in system.__dict__ and system.verlet_list.shape[0] > system.N
    assert np.array_equal(bond, np.array([[0, 1]], np.int32))


def test_matrix_cutoff_and_no_bonds(restated):
    system = _line(type=[1, 2, 2, 1])
    assert np.array_equal(system.create_bonds(np.array([[0.5, 1.1], [1.1, 1.2]])), np.array([[0, 1]], np.int32))
    assert np.array_equal(system.create_bonds(np.array([[0.5, 1.1], [1.1, 1.4]])), np.array([[0, 1], [1, 2]], np.int32))
    none = system.create_bonds(0.5)
    assert none.shape == (0, 2) and none.dtype == np.int32 and system.bond is none


def test_list_reuse(restated):
    system = _line(type=[1, 2, 2, 1])
    system.build_neighbor(3.0)
    rows = system.verlet_list
    system.create_bonds(1.5)
    assert system.verlet_list is rows and system.rc == 3.0  # (reaches 1.5: the remembered list serves)
    system.create_bonds(3.5)
    assert system.verlet_list is not rows and system.rc == 3.5


# ---- the cutoff normaliser
def test_normaliser_results():
    frame = _line(type=[3, 7, 7, 3]).data
    reach, compact, matrix = _normalize_bond_cutoff(1.5, frame)
    assert reach == 1.5 and compact.dtype == np.int32 and not compact.any() and matrix.tolist() == [[1.5]]
    reach, compact, matrix = _normalize_bond_cutoff({(7, 3): 1.1, (3, 3): 0.5, (7, 7): 1.2}, frame)
    assert reach == 1.2 and compact.tolist() == [0, 1, 1, 0] and matrix.tolist() == [[0.5, 1.1], [1.1, 1.2]]
    reach, compact, matrix = _normalize_bond_cutoff([[0.5, 1.1], [1.1, 1.3]], frame)
    assert reach == 1.3 and compact.tolist() == [0, 1, 1, 0] and matrix.dtype == np.float64
    frame = _line(element=["Zr", "Cu", "Cu", "Zr"]).data
    reach, compact, matrix = _normalize_bond_cutoff({("Cu", "Zr"): 2.0, ("Cu", "Cu"): 1.0, ("Zr", "Zr"): 3.0}, frame)
    assert reach == 3.0 and compact.tolist() == [1, 0, 0, 1] and matrix.tolist() == [[1.0, 2.0], [2.0, 3.0]]


@pytest.mark.parametrize("rc, columns, message", [
    (0.0, {}, "rc should be larger than 0."),
    (-1.0, {}, "rc should be larger than 0."),
    ({}, {"type": [1, 2, 2, 1]}, "pairwise rc should not be empty."),
    ({(1,): 1.0}, {"type": [1, 2, 2, 1]}, "pairwise rc key should have two entries."),
    ({("Cu", "Cu"): 1.0}, {"type": [1, 2, 2, 1]}, "Data must contain element column for element-pair bond cutoff."),
    ({(1, 1): 1.0}, {"element": ["Cu", "Zr", "Zr", "Cu"]}, "Data must contain type column for type-pair bond cutoff."),
    ({(1, 1): 1.0, (1, 2, 2): 1.0}, {"type": [1, 2, 2, 1]}, "pairwise rc key should have two type indices."),
    ({(1, 1): 1.0, (1, 3): 1.0}, {"type": [1, 2, 2, 1]}, r"type/element pair \(1, 3\) is not in current system."),
    ({(1, 1): 1.0, (1, 2): 0.0}, {"type": [1, 2, 2, 1]}, "pairwise rc should be larger than 0."),
    (np.ones((2, 2)), {}, "Data must contain type column for matrix bond cutoff."),
    (np.ones(4), {"type": [1, 2, 2, 1]}, "pairwise rc should be a 2D array."),
    (np.ones((3, 3)), {"type": [1, 2, 2, 1]}, r"pairwise rc shape should be \(2, 2\)."),
    (np.array([[1.0, 0.0], [0.0, 1.0]]), {"type": [1, 2, 2, 1]}, "pairwise rc should be larger than 0."),
])
def test_normaliser_assertions(rc, columns, message):
    with pytest.raises(AssertionError, match=message):
        _normalize_bond_cutoff(rc, _line(**columns).data)


def test_normaliser_names_the_missing_pairs():
    import re

    def plain(err):  # (numpy 2 prints a scalar as np.int64(1); the reference's message holds numpy scalars too)
        return re.sub(r"np\.\w+\(([^)]*)\)", r"\1", str(err.value))

    with pytest.raises(ValueError) as err:
        _normalize_bond_cutoff({(1, 1): 1.0}, _line(type=[1, 2, 2, 1]).data)
    assert plain(err) == "Missing rc for type pairs: [(1, 2), (2, 2)]"
    with pytest.raises(ValueError) as err:
        _normalize_bond_cutoff({("Cu", "Cu"): 1.0, ("Zr", "Zr"): 1.0}, _line(element=["Cu", "Zr", "Zr", "Cu"]).data)
    assert plain(err) == "Missing rc for type pairs: [('Cu', 'Zr')]"


def test_create_bonds_assertions(restated):
    with pytest.raises(AssertionError, match="rc should be larger than 0."):
        _line().create_bonds(0.0)
    with pytest.raises(AssertionError, match="Data must contain type column for matrix bond cutoff."):
        _line().create_bonds(np.ones((1, 1)))


# ---- forgotten with the list
def _close_pair():
    xs = np.array([1.0, 1.05, 5.0])
    pos = np.column_stack([xs, np.zeros(3), np.zeros(3)])
    return mp.System(pos=pos, box=mp.Box([20.0, 20.0, 20.0]))


def test_bond_goes_with_the_list(restated):
    system = _close_pair()
    system.create_bonds(0.5)
    assert hasattr(system, "bond") and np.array_equal(system.bond, [[0, 1]])
    assert system.delete_overlap(0.1) == 1
    assert not hasattr(system, "bond") and not hasattr(system, "verlet_list")
    system = _close_pair()
    system.create_bonds(0.5)
    system.build_neighbor(1.0)
    assert not hasattr(system, "bond") and hasattr(system, "verlet_list")  # (the bonds belong to the list they were read from)
    system.create_bonds(0.5)
    system.box = mp.Box([21.0, 20.0, 20.0])
    assert not hasattr(system, "bond")
    system.create_bonds(0.5)
    system.update_data(system.data, reset_neighbor=True)
    assert not hasattr(system, "bond")


# ---- the restatement against a pair loop
def test_restatement_against_a_loop():
    rng = np.random.default_rng(3)
    N, M = 40, 9
    rows = rng.integers(-1, N, (N, M)).astype(np.int32)
    dist = rng.random((N, M)) * 2.0
    nn = rng.integers(0, M + 1, N).astype(np.int32)
    types = rng.integers(-1, 3, N).astype(np.int32)  # (-1 and 2: outside a 2 x 2 matrix)
    cut = np.array([[0.8, 1.3], [1.3, 1.0]])
    want = set()
    for i in range(N):
        for q in range(nn[i]):
            j = rows[i, q]
            if j > i and 0 <= types[i] < 2 and 0 <= types[j] < 2 and dist[i, q] <= cut[types[i], types[j]]:
                want.add((i, int(j)))
    got = ref.build_bond(rows, dist, nn, types, cut)
    assert got.dtype == np.int32 and [tuple(p) for p in got.tolist()] == sorted(want) and len(want) > 5
    # a replica of 10 atoms: all rows, % 10, ends sorted, self pairs dropped, each pair once
    folded = sorted({(min(a % 10, b % 10), max(a % 10, b % 10)) for a, b in want if a % 10 != b % 10})
    assert [tuple(p) for p in ref.build_bond(rows, dist, nn, types, cut, 1, 10).tolist()] == folded


# ---- the real shim
def test_shim_checks_arguments_before_any_device_work():
    from mdapy_amd import _lib, kernels

    assert kernels.build_bond.__name__ == "mdapy_amd._build_bond" and "build_bond" not in kernels.NAMES
    build = kernels.build_bond.build_bond
    rows, dist, nn = np.zeros((5, 3), np.int32), np.ones((5, 3)), np.zeros(5, np.int32)
    types, one = np.zeros(5, np.int32), np.array([[1.0]])
    with pytest.raises(ValueError, match="rows"):
        build(rows, dist[:4], nn, types, one)
    with pytest.raises(ValueError, match="rows"):
        build(rows, dist, nn[:4], types, one)
    with pytest.raises(ValueError, match="rows"):
        build(rows, dist, nn, types[:2], one)
    with pytest.raises(ValueError, match="distance_list has shape"):
        build(rows, dist[:, :2], nn, types, one)
    with pytest.raises(ValueError, match="verlet_list has shape"):
        build(rows[0], dist, nn, types, one)
    with pytest.raises(ValueError, match="cutoff_matrix has shape"):
        build(rows, dist, nn, types, np.ones((2, 3)))
    for bad in (0.0, -1.0, float("nan"), float("inf")):
        with pytest.raises(ValueError, match="cutoff must be a positive number"):
            build(rows, dist, nn, types, np.array([[1.0, 1.0], [1.0, bad]]))
    with pytest.raises(ValueError, match="n_real"):
        build(rows, dist, nn, types, one, 1, 6)
    with pytest.raises(ValueError, match="rows"):
        kernels.build_bond.cluster_composition(np.ones(5, np.int32), np.zeros(4, np.int32), 1, 1)
    with pytest.raises(ValueError, match="want has shape"):
        kernels.build_bond.species_match(np.zeros((2, 2), np.int32), np.zeros((1, 3), np.int32))
    # the library itself
    L = _lib.lib()
    count = ctypes.c_int64(-1)
    args = (rows.ctypes.data, dist.ctypes.data, nn.ctypes.data, 5, 3, types.ctypes.data)
    assert L.mdh_build_bond(*args, one.ctypes.data, 0, 0, None, 0, ctypes.addressof(count), _lib.HOST, None) == _lib.ERR_ARG
    assert L.mdh_build_bond(*args, one.ctypes.data, 1, 0, None, 0, None, _lib.HOST, None) == _lib.ERR_ARG
    assert L.mdh_build_bond(rows.ctypes.data, dist.ctypes.data, nn.ctypes.data, 1 << 26, 64, None, one.ctypes.data, 1, 0, None, 0,
                            ctypes.addressof(count), _lib.HOST, None) == _lib.ERR_ARG  # 2^32 slots
    assert L.mdh_build_bond(None, None, None, 0, 3, None, one.ctypes.data, 1, 0, None, 0, ctypes.addressof(count), _lib.HOST, None) == 0
    assert count.value == 0  # (N == 0 is legal and needs no device)
    assert L.mdh_cluster_composition(None, None, 3, 0, 1, None, _lib.HOST, None) == _lib.ERR_ARG
    assert L.mdh_cluster_composition(None, None, 0, 0, 0, None, _lib.HOST, None) == _lib.ERR_ARG
    assert L.mdh_species_match(None, 2, 1, None, 0, None, 0, None, None, _lib.HOST, None) == _lib.ERR_ARG
    if _lib.device_count() > 0:
        return  # (with a device the valid calls compute: test_gpu_bonds.py)
    with pytest.raises(RuntimeError, match="HIP error"):
        build(rows, dist, nn, types, one)
    with pytest.raises(RuntimeError, match="HIP error"):
        kernels.build_bond.cluster_composition(np.ones(5, np.int32), np.zeros(5, np.int32), 1, 1)
    with pytest.raises(RuntimeError, match="HIP error"):
        kernels.build_bond.species_match(np.zeros((2, 2), np.int32), np.zeros((1, 2), np.int32))


# ---- the radii and the formula parser
def test_radii_table():
    from mdapy_amd.atomic_temperature import STANDARD_ATOMIC_WEIGHT

    assert set(STANDARD_ATOMIC_WEIGHT) <= set(vdw_radii.VDW_RADII)
    assert vdw_radii.vdw_radius("H") == 1.2 and vdw_radii.vdw_radius("O") == 1.5 and vdw_radii.vdw_radius(np.str_("C")) == 1.77
    assert all(1.0 < r < 3.6 for r in vdw_radii.VDW_RADII.values())
    with pytest.raises(ValueError, match="'Pm'"):
        vdw_radii.vdw_radius("Pm")


def test_formula_parser():
    assert _parse_formula("H2O") == {"H": 2, "O": 1}
    assert _parse_formula("CH3OH") == {"C": 1, "H": 4, "O": 1}
    assert _parse_formula("CO2") == {"C": 1, "O": 2}
    assert _parse_formula("Cl2") == {"Cl": 2}
    assert _parse_formula("H12C6") == {"H": 12, "C": 6}
    assert _parse_formula("") == {}


def test_grouping_of_composition_rows():
    from mdapy_amd.system import _group_rows

    rng = np.random.default_rng(9)
    for rows in (rng.integers(0, 5, (5000, 3)).astype(np.int32), rng.integers(0, 3, (70, 1)).astype(np.int32),
                 np.array([[2 ** 40, 3], [2 ** 40, 3], [1, 2 ** 40]], np.int64)):  # (the last does not fit one int64: numpy's own path)
        kinds, counts = _group_rows(rows)
        want = np.unique(rows, axis=0, return_counts=True)
        assert kinds.dtype == rows.dtype and np.array_equal(kinds, want[0]) and np.array_equal(counts, want[1])


def _molecules():
    """two waters, one of them written O first, a CO2, a lone Cl2, a lone H: 12 atoms in an open box"""
    names = ["H", "O", "H", "O", "H", "H", "O", "C", "O", "Cl", "Cl", "H"]
    pos = np.array([[0.0, 0.8, 0], [0, 0, 0], [0.8, 0, 0], [10, 0, 0], [10.8, 0, 0], [10, 0.8, 0], [20, 1.2, 0], [20, 0, 0], [20, -1.2, 0],
                    [30, 0, 0], [31.9, 0, 0], [40, 0, 0]], float)
    return mp.System(data={"x": pos[:, 0], "y": pos[:, 1], "z": pos[:, 2], "element": names}, box=mp.Box([50.0, 50.0, 50.0], boundary=[0, 0, 0]))


def test_species_search(restated):
    system = _molecules()
    found = system.cal_chemical_species(["H2O", "CO2", "Cl2", "HOH", "CH3OH", "N2", "H2O"], add_mol_id=True)
    assert list(found) == ["H2O", "CO2", "Cl2", "HOH", "CH3OH", "N2"]  # (the caller's spellings, in the caller's order)
    assert found == {"H2O": 2, "CO2": 1, "Cl2": 1, "HOH": 2, "CH3OH": 0, "N2": 0}
    assert system.data["type"].to_numpy().tolist() == [3, 4, 3, 4, 3, 3, 4, 1, 4, 2, 2, 3]  # C Cl H O
    mol = system.data["mol_id"].to_numpy()
    assert mol.dtype == np.int32 and mol.tolist() == [6, 6, 6, 6, 6, 6, 1, 1, 1, 2, 2, -1]  # (H2O is asked three times: the last index)
    assert system.cluster_number == 5
    plain = _molecules()
    assert plain.cal_chemical_species(["H2O"]) == {"H2O": 2} and "mol_id" not in plain.data.columns


def test_species_most_frequent(restated):
    system = _molecules()
    assert system.cal_chemical_species() == {"HHO": 2, "COO": 1, "ClCl": 1, "H": 1}  # (equal counts by ascending key)
    assert system.cal_chemical_species(check_most=2) == {"HHO": 2, "COO": 1}
    want = ref.most_frequent(ref.species_grouping(system.data["cluster_id"].to_numpy(), system.data["element"].to_numpy()), 10)
    assert system.cal_chemical_species() == want and list(system.cal_chemical_species()) == list(want)


def test_species_without_an_element_column(restated):
    full = _molecules()
    codes = {"H": 1, "O": 2, "C": 3, "Cl": 4}
    columns = {name: full.data[name].to_numpy() for name in "xyz"}
    box = mp.Box([50.0, 50.0, 50.0], boundary=[0, 0, 0])
    system = mp.System(data=dict(columns, type=np.array([codes[e] for e in full.data["element"].to_numpy()], np.int32)), box=box)
    assert system.cal_chemical_species(["H2O", "Cl2"], element_list=["H", "O", "C", "Cl"]) == {"H2O": 2, "Cl2": 1}
    assert system.cal_chemical_species(element_list=["H", "O", "C", "Cl"], check_most=1) == {"HHO": 2}
    with pytest.raises(AssertionError, match="'element_list' must be provided"):
        system.cal_chemical_species(["H2O"])
    with pytest.raises(AssertionError, match="must contain at least 4 elements"):
        system.cal_chemical_species(["H2O"], element_list=["H", "O", "C"])
    with pytest.raises(AssertionError, match="'type' column is required"):
        mp.System(data=columns, box=box).cal_chemical_species(["H2O"], element_list=["H"])
    with pytest.raises(ValueError, match="'Xx'"):
        system.cal_chemical_species(["H2O"], element_list=["H", "O", "C", "Xx"])


# ---- the water frame: 24 576 atoms, 8 192 molecules
@pytest.fixture(scope="module")
def water_path(tmp_path_factory):
    path = tmp_path_factory.mktemp("water") / "water.xyz"
    with gzip.open(os.path.join(GOLDEN, "water.xyz.gz"), "rb") as src:
        path.write_bytes(src.read())
    return str(path)


def test_water_frame(restated, water_path):
    system = mp.System(water_path)
    assert system.N == 24576
    assert system.cal_chemical_species(["H2O"], scale=0.4, add_mol_id=True) == {"H2O": 8192}
    assert not system.data["mol_id"].to_numpy().any()
    cut = {("H", "H"): 2.4 * 0.4, ("H", "O"): 2.7 * 0.4, ("O", "O"): 3.0 * 0.4}
    bond = system.create_bonds(cut)
    assert bond.shape == (16384, 2)
    oxygen = system.data["element"].to_numpy() == "O"
    ends = np.bincount(np.asarray(bond).ravel(), minlength=system.N)
    assert np.all(ends[oxygen] == 2) and np.all(ends[~oxygen] == 1)
    _, compact, matrix = _normalize_bond_cutoff(cut, system.data)
    edge = ref.margin(system.verlet_list, system.distance_list, system.neighbor_number, compact, matrix)
    assert 2.0e-3 < edge < 2.1e-3  # (2.05e-3 A: nothing here is a knife edge)

    system = mp.System(water_path)
    wide = np.array([[2.4, 2.7], [2.7, 3.0]]) * 0.6
    system.build_neighbor(float(wide.max()))
    _, compact, _ = _normalize_bond_cutoff({("H", "H"): 1.0, ("H", "O"): 1.0, ("O", "O"): 1.0}, system.data)
    assert ref.margin(system.verlet_list, system.distance_list, system.neighbor_number, compact, wide) > 1e-9
    assert system.cal_chemical_species(scale=0.6, check_most=3) == {"HHO": 7760, "HHHHOO": 199, "HHHHHHOOO": 10}
    full = system.cal_chemical_species(scale=0.6)
    assert sorted(full.values(), reverse=True) == [7760, 199, 10, 1] and system.cluster_number == 7970
    assert len(system.create_bonds(wide)) == 16844
