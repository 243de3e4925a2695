"""The EAM calculator on the GPU (mdapy_amd/csrc/eam.hip): energies, forces and virials bit for bit against the numpy restatement
of the reference (tests/_eam_ref.py) run on the list the System holds — ``as_numpy`` of its rows, distances and counts, in the
compute view's numbering — the reference's LAMMPS fixture through ``System.calc``, the raw shim with its accumulate semantics,
the fixed-order stress sum, and the argument errors."""
import os

import numpy as np
import pytest

import _eam_ref
import mdapy_amd as mp
from mdapy_amd.devarray import as_numpy

pytestmark = pytest.mark.gpu

GOLDEN = _eam_ref.GOLDEN
EPS = np.finfo(np.float64).eps


@pytest.fixture(autouse=True)
def _need_gpu():
    from mdapy_amd import _lib

    if _lib.device_count() < 1:
        pytest.fail("test_gpu_eam needs a HIP device")


@pytest.fixture(scope="module")
def potentials():
    return {k: mp.EAM(os.path.join(GOLDEN, _eam_ref.CASES[k][0])) for k in (1, 2, 3)}


def _system(pos, box, names, eam):
    s = mp.System(pos=pos, box=box)
    s.set_element(names)
    s.calc = eam
    return s


def _alloy(cells=6, seed=0, rattle=0.1, elements=("Co", "Ni", "Cr"), ratios=(0.2, 0.3, 0.5)):
    """rattled fcc alloy: 6 x 6 x 6 cells are 864 atoms (no multiple of 64) in a 21.6 A box"""
    pos, box, names = _eam_ref.hea(cells, list(elements), list(ratios), False)
    return pos + np.random.default_rng(seed).normal(0, rattle, pos.shape), np.array(box, float)[:3], names


def _check(s, detail=None):
    """the System's four results; the per-atom ones compared bitwise with the restatement on the System's own list"""
    got = s.get_energies(), s.get_force(), s.get_virials()
    stress = s.get_stress()
    want = _eam_ref.on_system_list(s, s.calc, detail)
    for name, g, w, shape in zip(("energies", "forces", "virials"), got, want, ((s.N,), (s.N, 3), (s.N, 9))):
        assert isinstance(g, np.ndarray) and g.dtype == np.float64 and g.shape == shape
        assert np.array_equal(g, w), f"{name}: {int((g != w).sum())} values differ, max {np.abs(g - w).max():.3e}"
    assert stress.shape == (6,) and np.isfinite(stress).all()
    return got + (stress,)


# ---------------------------------------------------------------------------------------------- bitwise cases
def test_a_rattled_alloy_in_an_orthogonal_box(potentials):
    pos, cell, names = _alloy()
    s = _system(pos, cell, names, potentials[2])
    e, f, v, stress = _check(s)
    assert len(pos) == 864 and "_enlarge_data" not in s.__dict__ and s.rc == potentials[2].rc
    assert np.abs(f).max() > 0.1 and e.max() < 0


def test_b_triclinic_box(potentials):
    pos, cell, names = _alloy(seed=1)
    sheared = cell.copy()
    sheared[1, 0] = 0.3 * sheared[1, 1]
    sheared[2, 0], sheared[2, 1] = 0.2 * sheared[2, 2], -0.15 * sheared[2, 2]
    tri = (pos @ np.linalg.inv(cell)) @ sheared
    s = _system(tri, mp.Box(sheared), names, potentials[2])
    assert s.box.triclinic
    _check(s)


@pytest.mark.parametrize("boundary", [[1, 1, 0], [0, 0, 0]])
def test_c_open_boundaries_have_short_rows(potentials, boundary):
    pos, cell, names = _alloy(seed=2)
    s = _system(pos, mp.Box(cell, boundary), names, potentials[2])
    _check(s)
    counts = as_numpy(s.neighbor_number)
    assert counts.min() < 0.7 * counts.max()


def test_d_thin_box_takes_the_replica(potentials):
    path, pos, box, names = _eam_ref.fixture_case(1)
    s = _system(pos, box, names, potentials[1])
    e, f, v, stress = _check(s)
    assert s._enlarge_data.shape[0] == 8 * len(pos) and e.shape == (108,)
    assert np.array_equal(stress, s.get_stress())


def test_e_shuffled_order_takes_the_twin(potentials, monkeypatch):
    monkeypatch.setenv("MDAPY_SPATIAL_SORT", "1")
    pos, cell, names = _alloy(seed=3)
    order = np.random.default_rng(4).permutation(len(pos))
    s = _system(pos[order], cell, names[order], potentials[2])
    e, f, v, stress = _check(s)  # (the restatement on the translated rows, in the shuffled numbering)
    assert s._spatial() is not None and s._twin.shown.mirror is s.verlet_list
    monkeypatch.setenv("MDAPY_SPATIAL_SORT", "0")
    plain = _system(pos, cell, names, potentials[2])
    # atom for atom the plain system's (its rows may list the same neighbours in another order: to rounding)
    assert np.abs(e - plain.get_energies()[order]).max() < 1e-11 and np.abs(f - plain.get_force()[order]).max() < 1e-11


def test_f_gas_with_empty_rows(potentials, tmp_path):
    """1 500 atoms in a 30 A box under a potential squeezed to rc = 2.6 A (the NiCoCr tables on a finer grid, written and read
    back): rows of 0 to about 12 entries; an isolated atom has the energy F(0) and no force and no virial"""
    src = potentials[2]
    squeezed = mp.EAM(os.path.join(GOLDEN, "NiCoCr.lammps.eam.gz"))
    squeezed.dr = 2.6 / (src.nr - 1)
    squeezed.rc = 2.6
    squeezed.write_eam_alloy(str(tmp_path / "squeezed.eam.alloy"))
    eam = mp.EAM(str(tmp_path / "squeezed.eam.alloy"))
    assert eam.rc == 2.6 and np.array_equal(eam._rphi_r, src._rphi_r)
    rng = np.random.default_rng(0)
    pos = rng.random((1500, 3)) * 30.0
    names = np.array(["Ni", "Co", "Cr"], dtype=object)[rng.integers(0, 3, 1500)]
    s = _system(pos, 30.0, names, eam)
    e, f, v, stress = _check(s)
    counts = as_numpy(s.neighbor_number)
    alone = counts == 0
    assert alone.sum() >= 10 and counts.max() >= 8
    types = _eam_ref.types_of(s.data, eam.elements_list)
    assert np.array_equal(e[alone], eam.F_rho[types[alone], 0]) and not f[alone].any() and not v[alone].any()
    assert np.isfinite(e).all() and np.isfinite(f).all()


def test_g_a_remembered_longer_list_is_reused(potentials):
    pos, cell, names = _alloy(seed=5)
    fresh = _system(pos, cell, names, potentials[2])
    e0, f0, v0 = fresh.get_energies(), fresh.get_force(), fresh.get_virials()
    s = _system(pos, cell, names, potentials[2])
    s.build_neighbor(potentials[2].rc + 1.0)
    rows = s.verlet_list
    e, f, v, stress = _check(s)  # (the restatement skips the entries with dist > rc of that same list)
    assert s.verlet_list is rows and rows.shape[1] > fresh.verlet_list.shape[1]
    assert float(as_numpy(s.distance_list)[:, 0:as_numpy(s.neighbor_number).min()].max()) > potentials[2].rc
    # and equal to the fresh list's results as sets of per-atom values: the same pairs, possibly added in another order
    assert np.abs(e - e0).max() < 1e-12 and np.abs(f - f0).max() < 1e-12 and np.abs(v - v0).max() < 1e-11


def test_h_a_pair_closer_than_dr(potentials):
    pos, cell, names = _alloy(seed=6)
    pos[1] = pos[0] + np.array([0.4 * potentials[2].dr, 0.0, 0.0])
    s = _system(pos, cell, names, potentials[2])
    e, f, v, stress = _check(s)
    d = as_numpy(s.distance_list)
    assert 0 < d.min() < potentials[2].dr  # spline interval 0
    assert np.isfinite(e).all() and np.isfinite(f).all() and np.isfinite(v).all()


def test_i_overdense_atom_reads_the_extrapolation_slot(potentials):
    path, pos, box, names = _eam_ref.fixture_case(2)
    s = _system(pos, box, names, potentials[2])
    detail = {}
    _check(s, detail)
    top = (potentials[2].nrho - 1) * potentials[2].drho
    assert detail["density"].max() > 1.2 * top  # 1.27 x the tabulated maximum: the last, linear slot of F


def test_j_two_elements_of_a_five_element_file_in_another_order(potentials):
    pos, cell, names = _alloy(seed=7, elements=("Cu", "Ni"), ratios=(0.4, 0.6))
    s = _system(pos, cell, names, potentials[1])
    e, f, v, stress = _check(s)
    types = _eam_ref.types_of(s.data, potentials[1].elements_list)
    assert sorted(set(types.tolist())) == [1, 4] and "_enlarge_data" not in s.__dict__


# ---------------------------------------------------------------------------------------------- the LAMMPS fixture
@pytest.mark.parametrize("case", [1, 2, 3])
def test_lammps_fixture(potentials, case):
    want = np.load(os.path.join(GOLDEN, "eam.npz"))
    path, pos, box, names = _eam_ref.fixture_case(case)
    s = _system(pos, box, names, potentials[case])
    got = dict(zip(("energies", "forces", "virials", "stress"), _check(s)))
    for name in got:
        print(f"case {case} {name}: max abs difference {np.abs(got[name] - want[f'case{case}__{name}']).max():.3e}")
    for name in got:
        assert np.allclose(got[name], want[f"case{case}__{name}"]), name


# ---------------------------------------------------------------------------------------------- the shim
def test_raw_shim_adds_into_its_arrays(potentials):
    import torch

    from mdapy_amd import _eam
    from mdapy_amd.devarray import HArray

    eam = potentials[2]
    pos, cell, names = _alloy(seed=8)
    s = _system(pos, cell, names, eam)
    via_system = s.get_energies(), s.get_force(), s.get_virials()
    n = len(pos)
    rows, dist, counts = (as_numpy(a) for a in (s.verlet_list, s.distance_list, s.neighbor_number))
    cols = [np.ascontiguousarray(pos[:, k]) for k in range(3)]
    types = _eam_ref.types_of(s.data, eam.elements_list)
    where = (cell, np.zeros(3), np.array([1, 1, 1], np.int32))
    tables = (eam.rc, eam.dr, eam.drho, eam.F_rho, eam.rho_r, eam._rphi_r)
    ours, ref = _eam.EAM(*tables), _eam_ref.EAM(*tables)
    got = np.zeros((n, 3)), np.zeros((n, 9)), np.zeros(n)
    want = np.zeros((n, 3)), np.zeros((n, 9)), np.zeros(n)
    ours.calculate(*cols, types, *where, rows, dist, counts, *got, 4)
    ref.calculate(*cols, types, *where, rows, dist, counts, *want, 4)
    for g, w, direct in zip(got, want, (via_system[1], via_system[2], via_system[0])):
        assert np.array_equal(g, w) and np.array_equal(g, direct)
    # a second call into the same arrays: (first + F_i) + e_pair, first + f, first + v * 0.5
    ours.calculate(*cols, types, *where, rows, dist, counts, *got, 4)
    ref.calculate(*cols, types, *where, rows, dist, counts, *want, 4)
    for g, w, once in zip(got, want, (via_system[1], via_system[2], via_system[0])):
        assert np.array_equal(g, w) and not np.array_equal(g, once)
    # arrays in HBM, into arrays that hold something already
    up = lambda a: HArray(torch.from_numpy(np.ascontiguousarray(a)).cuda())
    start = np.full((n, 3), 0.25), np.full((n, 9), -1.5), np.full(n, 3.0)
    dev = tuple(up(a) for a in start)
    want = tuple(a.copy() for a in start)
    ours.calculate(*(up(c) for c in cols), up(types), *where, s.verlet_list, s.distance_list, s.neighbor_number, *dev)
    ref.calculate(*cols, types, *where, rows, dist, counts, *want)
    for g, w in zip(dev, want):
        assert np.array_equal(g.numpy(), w)
    # a type outside the potential contributes nothing and receives nothing
    odd = types.copy()
    odd[::7] = 3
    got = np.full((n, 3), 0.25), np.full((n, 9), -1.5), np.full(n, 3.0)
    want = tuple(a.copy() for a in got)
    ours.calculate(*cols, odd, *where, rows, dist, counts, *got)
    ref.calculate(*cols, odd, *where, rows, dist, counts, *want)
    for g, w, first in zip(got, want, start):
        assert np.array_equal(g, w) and np.array_equal(g[::7], first[::7])
    # accumulate=False writes into arrays that hold anything; virial_sum is the fixed-order sum of the first n_real rows
    got = np.full((n, 3), np.nan), np.full((n, 9), np.nan), np.full(n, np.nan)
    total = np.full(9, np.nan)
    ours.calculate(*cols, types, *where, rows, dist, counts, *got, accumulate=False, n_real=500, virial_sum=total)
    assert np.array_equal(got[2], via_system[0]) and np.array_equal(got[0], via_system[1]) and np.array_equal(got[1], via_system[2])
    exact = _eam_ref.exact_column_sums(got[1][:500])
    assert np.all(np.abs(total - exact) <= 499 * EPS * np.abs(got[1][:500]).sum(axis=0))
    with pytest.raises(ValueError):
        ours.calculate(*cols[:2], cols[2][:-1], types, *where, rows, dist, counts, *got)
    with pytest.raises(ValueError):
        ours.calculate(*cols, types, *where, rows, dist, counts, got[1], got[0], got[2])


# ---------------------------------------------------------------------------------------------- the stress
@pytest.mark.parametrize("case", ["alloy", "replica"])
def test_stress_is_reproducible_and_within_the_bound_of_any_summation_order(potentials, case):
    """every component within (N - 1) eps sum|v_i| / volume of the stress from the exact sum (math.fsum) of the GPU's own virials:
    the worst case of any order of adding N numbers"""
    if case == "alloy":
        pos, cell, names = _alloy(seed=9)
        make = lambda: _system(pos, cell, names, potentials[2])
    else:
        path, pos, cell, names = _eam_ref.fixture_case(1)
        make = lambda: _system(pos, cell, names, potentials[1])
    s = make()
    stress, virials = s.get_stress().copy(), s.get_virials().copy()
    again = make()
    assert np.array_equal(again.get_stress(), stress) and np.array_equal(again.get_virials(), virials)  # the same bits
    volume, n = s.box.volume, s.N
    want = _eam_ref.stress_of(_eam_ref.exact_column_sums(virials), volume)
    size = np.abs(virials).sum(axis=0).reshape(3, 3)
    bound = ((n - 1) * EPS * 0.5 * (size + size.T) / volume).ravel()[[0, 4, 8, 5, 2, 1]]
    print(f"{case}: |stress - exact| / bound = {(np.abs(stress - want) / bound).tolist()}")
    assert np.all(np.abs(stress - want) <= bound) and np.abs(stress).max() > 0


# ---------------------------------------------------------------------------------------------- argument errors
def test_argument_errors_come_before_device_work(potentials):
    from mdapy_amd import _eam, _lib

    eam = potentials[2]
    L = _lib.lib()
    box, origin, pbc = np.eye(3) * 20.0, np.zeros(3), np.ones(3, np.int32)
    where = (box.ctypes.data, origin.ctypes.data, pbc.ctypes.data)

    def call(N=4, M=2, nelem=3, nrho=10, drho=0.1, nr=10, dr=0.1, rc=0.9, n_real=4):
        # (null array pointers: a call that got as far as touching one would not come back with an error code)
        return L.mdh_eam(None, None, None, None, N, *where, None, None, None, M, None, None, None, nelem, nrho, drho, nr, dr, rc,
                         1, None, None, None, n_real, None, _lib.HOST, None)

    for bad in (dict(nelem=0), dict(nr=1), dict(nrho=1), dict(dr=0.0), dict(drho=-0.1), dict(rc=0.0), dict(rc=float("nan")),
                dict(M=1 << 23), dict(N=-1), dict(n_real=5)):
        assert call(**bad) == _lib.ERR_ARG, bad
        with pytest.raises(ValueError):
            _lib.check(call(**bad))
    n = 8
    x = np.arange(n) * 2.0
    rows, dist, counts = np.full((n, 2), -1, np.int32), np.full((n, 2), 9.0), np.zeros(n, np.int32)
    out = np.zeros((n, 3)), np.zeros((n, 9)), np.zeros(n)
    types = np.zeros(n, np.int32)
    with pytest.raises(ValueError):
        _eam.EAM(-1.0, eam.dr, eam.drho, eam.F_rho, eam.rho_r, eam._rphi_r).calculate(x, x, x, types, box, origin, pbc, rows, dist, counts, *out)
    with pytest.raises(ValueError):
        _eam.EAM(eam.rc, 0.0, eam.drho, eam.F_rho, eam.rho_r, eam._rphi_r)
    assert not out[0].any() and not out[2].any()
