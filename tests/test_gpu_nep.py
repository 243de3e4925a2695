"""The NEP calculator on the GPU (mdapy_amd/csrc/nep.hip): energies, forces, virials, descriptors and latent space against the numpy
restatement (tests/_nep_ref.py) run on the list the System holds, the reference's fixtures through ``System.calc``, exactness (the
same bits twice, the twin's bits permuted, the fixed-order stress sum), ``FIRE`` with its state in HBM, and the raw shim.

The device's tanh, cos, sin and exp are not numpy's, so the comparison with the restatement is no bitwise one: for every case
``max |gpu - restatement| / max |restatement|`` per quantity is printed and must stay below ``BOUND`` (profiles/nep.md holds the
measured values)."""
import os

import numpy as np
import pytest

import _eam_ref
import _nep_ref
import mdapy_amd as mp
from mdapy_amd.devarray import as_numpy

pytestmark = pytest.mark.gpu

GOLDEN = _nep_ref.GOLDEN
ALCRNI = os.path.join(os.path.dirname(GOLDEN), "input_files", "AlCrNi.xyz")
EPS = np.finfo(np.float64).eps
# 16 times the largest value measured on an MI355X over all cases below (profiles/nep.md: 4.85e-14, the forces after five FIRE
# steps on the two paths; a single calculation stays below 4.6e-15), and never above 1e-9: a larger difference is another
# algorithm, not rounding
BOUND = 7.8e-13
QUANTITIES = ("energy", "force", "virial", "descriptor", "latent")


@pytest.fixture(autouse=True)
def _need_gpu():
    from mdapy_amd import _lib

    if _lib.device_count() < 1:
        pytest.fail("test_gpu_nep needs a HIP device")


@pytest.fixture(scope="module")
def unep():
    return mp.NEP(_nep_ref.UNEP)


@pytest.fixture(scope="module")
def variants(tmp_path_factory):
    where = tmp_path_factory.mktemp("nep_models")
    out = {}
    for k, (name, how) in enumerate(_nep_ref.VARIANTS.items()):
        path = str(where / f"{name}.txt")
        _nep_ref.write_model(path, seed=k, **how)
        out[name] = mp.NEP(path)
    return out


def _system(pos, box, names, calc):
    s = mp.System(pos=pos, box=box)
    s.set_element(names)
    s.calc = calc
    return s


def _alloy(cells=5, seed=0, rattle=0.1, elements=("Al", "Cr", "Ni")):
    """rattled fcc alloy: 5 x 5 x 5 cells are 500 atoms (no multiple of the 8 atoms of a workgroup, 63 workgroups) in an 18 A box"""
    pos, box, names = _eam_ref.hea(cells, list(elements), [1.0 / len(elements)] * len(elements), False)
    return pos + np.random.default_rng(seed).normal(0, rattle, pos.shape), np.array(box, float)[:3], names


def _check(s, label):
    """everything the calculator gives for ``s``, each quantity within BOUND of the restatement on the System's own list"""
    calc = s.calc
    got = {"energy": s.get_energies(), "force": s.get_force(), "virial": s.get_virials(),
           "descriptor": calc.get_descriptor(s.data, s.box), "latent": calc.get_latentspace(s.data, s.box)}
    stress = s.get_stress()
    want = _nep_ref.on_system_list(s, calc, want=QUANTITIES)
    shapes = {"energy": (s.N,), "force": (s.N, 3), "virial": (s.N, 9), "descriptor": (s.N, calc.info["num_ndim"]),
              "latent": (s.N, calc.info["num_nlatent"])}
    figures = {}
    for name in QUANTITIES:
        g, w = got[name], want[name]
        assert isinstance(g, np.ndarray) and g.dtype == np.float64 and g.shape == shapes[name] and np.isfinite(g).all(), name
        figures[name] = float(np.abs(g - w).max() / np.abs(w).max())
    print(f"closeness {label}: " + ", ".join(f"{name} {figures[name]:.2e}" for name in QUANTITIES))
    for name in QUANTITIES:
        assert figures[name] <= BOUND, (name, figures[name])
    total = _nep_ref.exact_column_sums(got["virial"])
    size = np.abs(got["virial"]).sum(axis=0).reshape(3, 3)
    room = ((s.N - 1) * EPS * 0.5 * (size + size.T) / s.box.volume).ravel()[[0, 4, 8, 5, 2, 1]]
    assert np.all(np.abs(stress - _eam_ref.stress_of(total, s.box.volume)) <= room)  # any order of adding N numbers
    return got, stress


# ---------------------------------------------------------------------------------------------- closeness to the restatement
def test_a_alcrni_triclinic_replica(unep):
    s = mp.System(ALCRNI)
    s.calc = unep
    got, stress = _check(s, "AlCrNi")
    assert s.N == 72 and s.box.triclinic and s._enlarge_data.shape[0] > 72


def test_b_alloy_108_replica(unep):
    pos, box, names = _eam_ref.hea(3, ["Al", "Cr", "Ni"], [1 / 3, 1 / 3, 1 / 3], False)
    s = _system(pos, box, names, unep)
    _check(s, "alloy108")
    assert s._enlarge_data.shape[0] == 8 * 108


def test_c_rattled_500(unep):
    pos, cell, names = _alloy()
    s = _system(pos, cell, names, unep)
    got, stress = _check(s, "rattled500")
    assert len(pos) == 500 and "_enlarge_data" not in s.__dict__ and s.rc == 6.0 and np.abs(got["force"]).max() > 0.5


def test_d_sheared_500(unep):
    pos, cell, names = _alloy(seed=1)
    sheared = cell.copy()
    sheared[1, 0] = 0.3 * sheared[1, 1]
    sheared[2, 0], sheared[2, 1] = 0.2 * sheared[2, 2], -0.15 * sheared[2, 2]
    tri = (pos @ np.linalg.inv(cell)) @ sheared
    s = _system(tri, mp.Box(sheared), names, unep)
    assert s.box.triclinic
    _check(s, "sheared500")


@pytest.mark.parametrize("boundary", [[1, 1, 0], [0, 0, 0]])
def test_e_open_boundaries_have_short_and_empty_rows(unep, boundary):
    pos, cell, names = _alloy(seed=2)
    if boundary == [0, 0, 0]:  # two atoms far outside the cluster: empty rows
        pos = np.vstack([pos, [[-40.0, -40.0, -40.0], [60.0, 60.0, 70.0]]])
        names = np.concatenate([names, ["Ni", "Al"]])
    s = _system(pos, mp.Box(cell, boundary), names, unep)
    got, stress = _check(s, f"open{''.join(map(str, boundary))}")
    counts = as_numpy(s.neighbor_number)[: s.N]
    assert counts.min() < 0.7 * counts.max()
    if boundary == [0, 0, 0]:
        assert counts.min() == 0 and not got["force"][-1].any() and not got["descriptor"][-1].any()


def test_f_close_pairs_reach_zbl(unep):
    pos, cell, names = _alloy(seed=3)
    pos[1] = pos[0] + np.array([0.8, 0.0, 0.0])
    pos[9] = pos[8] + np.array([0.0, 1.5, 0.0])
    s = _system(pos, cell, names, unep)
    got, stress = _check(s, "closepairs")
    assert np.abs(got["force"]).max() > 50.0  # ZBL's repulsion


def test_g_single_element(unep):
    pos, cell, names = _alloy(seed=4, elements=("Ni",))
    s = _system(pos, cell, names, unep)
    _check(s, "singleNi")
    assert unep._model((7,)).head[0] == 1


@pytest.mark.parametrize("name", list(_nep_ref.VARIANTS))
def test_h_synthetic_variants(variants, name):
    """4 x 4 x 4 cells: 256 atoms in a 14.4 A box, no replica under cutoffs of 5 A; the ZBL variants with the two close pairs"""
    calc = variants[name]
    pos, cell, names = _alloy(cells=4, seed=5, elements=("Al", "Ni") if name == "wide" else ("Al", "Cr", "Ni"))
    if calc.info["zbl"]:
        pos[1] = pos[0] + np.array([0.8, 0.0, 0.0])
        pos[9] = pos[8] + np.array([0.0, 1.5, 0.0])
    s = _system(pos, cell, names, calc)
    _check(s, name)
    assert "_enlarge_data" not in s.__dict__


# ---------------------------------------------------------------------------------------------- exactness
def test_two_runs_give_the_same_bits(unep):
    results = []
    for _ in range(2):
        pos, cell, names = _alloy(seed=6)
        s = _system(pos, cell, names, unep)
        results.append([np.array(a) for a in (s.get_energies(), s.get_force(), s.get_virials(), s.get_stress(),
                                               unep.get_descriptor(s.data, s.box), unep.get_latentspace(s.data, s.box))])
    for a, b in zip(*results):
        assert np.array_equal(a, b)
    results = []
    for _ in range(2):
        s = mp.System(ALCRNI)
        s.calc = unep
        results.append([np.array(a) for a in (s.get_energies(), s.get_force(), s.get_virials(), s.get_stress())])
    for a, b in zip(*results):
        assert np.array_equal(a, b)


def test_shuffled_frame_gives_the_twins_bits_permuted(unep, monkeypatch):
    import mdapy_amd.kernels as K
    from mdapy_amd import policy

    monkeypatch.setenv("MDAPY_SPATIAL_SORT", "1")
    pos, cell, names = _alloy(seed=7)
    order = np.random.default_rng(8).permutation(len(pos))
    s = _system(pos[order], cell, names[order], unep)
    got, stress = _check(s, "twin")  # (the restatement on the translated rows, in the shuffled numbering)
    assert s._spatial() is not None and s._twin.shown.mirror is s.verlet_list
    twin = s._listed_on_twin()
    perm = as_numpy(twin._perm)
    n = len(pos)
    types = np.array([unep.element_list.index(e) for e in names[order]], np.int32)
    type_map = np.full(16, -1, np.int32)
    type_map[[1, 3, 7]] = [0, 1, 2]
    out = dict(energy=np.zeros(n), force=np.zeros((n, 3)), virial=np.zeros((n, 9)))
    K.nep.calculate(*(as_numpy(c) for c in policy.positions(twin.data)), types[perm], type_map, s.box.box, s.box.origin, s.box.boundary,
                    as_numpy(twin.verlet_list), as_numpy(twin.distance_list), as_numpy(twin.neighbor_number), unep._model((1, 3, 7)), **out)
    for name in out:  # row p of the twin's run is atom perm[p] of the caller
        assert np.array_equal(got[name][perm], out[name]), name
    monkeypatch.setenv("MDAPY_SPATIAL_SORT", "0")
    plain = _system(pos, cell, names, unep)
    assert np.abs(got["energy"] - plain.get_energies()[order]).max() < 1e-11 and np.abs(got["force"] - plain.get_force()[order]).max() < 1e-11


def test_virial_sum_is_the_fixed_order_sum_of_the_real_rows(unep):
    """the raw shim on a replica's list: virial_sum9 adds the first n_real rows and no others, the same bits on every call, within
    (n - 1) eps sum|v| of the exact sum"""
    import mdapy_amd.kernels as K
    from mdapy_amd import policy

    s = mp.System(ALCRNI)
    s.calc = unep
    via_system = s.get_virials()
    cell, frame = s._get_compute_view()
    n = frame.shape[0]
    types = np.array([unep.element_list.index(e) for e in np.asarray(frame["element"].to_numpy()).astype(str)], np.int32)
    type_map = np.full(16, -1, np.int32)
    type_map[[1, 3, 7]] = [0, 1, 2]
    sums = []
    for n_real in (72, 72, n, 1):
        virial, total = np.full((n, 9), np.nan), np.full(9, np.nan)
        K.nep.calculate(*(as_numpy(c) for c in policy.positions(frame)), types, type_map, cell.box, cell.origin, cell.boundary,
                        as_numpy(s.verlet_list), as_numpy(s.distance_list), as_numpy(s.neighbor_number), unep._model((1, 3, 7)),
                        virial=virial, virial_sum=total, n_real=n_real)
        assert np.array_equal(virial[:72], via_system)
        exact = _nep_ref.exact_column_sums(virial[:n_real])
        assert np.all(np.abs(total - exact) <= max(n_real - 1, 0) * EPS * np.abs(virial[:n_real]).sum(axis=0))
        sums.append(total)
    assert np.array_equal(sums[0], sums[1]) and np.array_equal(sums[3], virial[0]) and not np.array_equal(sums[0], sums[2])
    assert np.array_equal(s.get_stress(), unep._stress_of_sums(sums[0], s.box.volume))


# ---------------------------------------------------------------------------------------------- the reference's fixtures
def test_pynep_fixture(unep):
    want = np.load(os.path.join(GOLDEN, "nep.npz"))
    s = mp.System(ALCRNI)
    s.calc = unep
    got = {"energies": s.get_energies(), "forces": s.get_force(), "stress": s.get_stress(),
           "descriptor": unep.get_descriptor(s.data, s.box), "latent": unep.get_latentspace(s.data, s.box)}
    for name in got:
        print(f"pynep {name}: max abs difference {np.abs(got[name] - want[name]).max():.3e}")
    for name in got:
        assert np.allclose(got[name], want[name]), name


@pytest.mark.parametrize("index", [0, 1])
def test_lammps_fixture(unep, index):
    want = np.load(os.path.join(GOLDEN, "nep_lmp.npz"))
    if index == 0:
        s = _system(*_eam_ref.hea(3, ["Al", "Cr", "Ni"], [1 / 3, 1 / 3, 1 / 3], False), unep)
    else:
        s = mp.System(ALCRNI)
        s.calc = unep
    got = {"energies": s.get_energies(), "forces": s.get_force(), "stress": s.get_stress(), "virials": s.get_virials()}
    for name in got:
        print(f"lammps sys{index} {name}: max abs difference {np.abs(got[name] - want[f'sys{index}__{name}']).max():.3e}")
    for name in got:
        assert np.allclose(got[name], want[f"sys{index}__{name}"]), name


# ---------------------------------------------------------------------------------------------- FIRE with its state in HBM
MODES = [(False, False, None, False, False, 0), (True, False, None, False, False, 0), (False, True, None, False, False, 0),
         (True, True, None, False, False, 0), (False, True, [1, 0, 0, 0, 0, 0], False, False, 0), (False, True, None, True, False, 0),
         (False, True, None, False, True, 0), (False, True, None, False, False, 1)]


@pytest.mark.parametrize("mode", range(8))
def test_fire_on_the_device_against_ase_and_against_the_host_path(unep, mode):
    use_abc, optimize_cell, mask, hydro, const_v, p = MODES[mode]
    want = np.load(os.path.join(GOLDEN, "minimize.npz"))
    got = {}
    for device in (True, False):
        s = mp.System(ALCRNI)
        s.calc = unep
        fire = mp.FIRE(s, use_abc=use_abc, optimize_cell=optimize_cell, mask=mask, hydrostatic_strain=hydro, constant_volume=const_v,
                       scalar_pressure=p, device=device)
        fire.run(steps=int(want["steps"]), show_process=False)
        assert fire._hbm == device
        got[device] = {"stress": s.get_stress(), "forces": s.get_force(), "energies": s.get_energies()}
    for name in got[True]:
        assert np.allclose(got[True][name], want[f"mode_{mode}__{name}"]), name
        figure = np.abs(got[True][name] - got[False][name]).max() / np.abs(got[False][name]).max()
        print(f"closeness fire mode {mode} {name}: HBM path against host path {figure:.2e}")
        assert figure <= BOUND, (name, figure)


# ---------------------------------------------------------------------------------------------- the raw shim
def test_argument_errors_come_before_device_work():
    from mdapy_amd import _lib

    tried = 0
    for bad, code in _nep_ref.argument_error_calls(_lib.lib()):
        assert code == _lib.ERR_ARG, bad
        tried += 1
    assert tried >= 20


def test_null_outputs_are_skipped_and_device_arrays_work(unep):
    import torch

    import mdapy_amd.kernels as K
    from mdapy_amd.devarray import HArray

    pos, cell, names = _alloy(cells=4, seed=9)
    s = _system(pos, cell, names, unep)
    e, f, v = s.get_energies(), s.get_force(), s.get_virials()
    q = unep.get_descriptor(s.data, s.box)
    n = len(pos)
    types = np.array([unep.element_list.index(x) for x in names], np.int32)
    type_map = np.full(16, -1, np.int32)
    type_map[[1, 3, 7]] = [0, 1, 2]
    cols = [np.ascontiguousarray(pos[:, k]) for k in range(3)]
    where = (cell, np.zeros(3), np.array([1, 1, 1], np.int32))
    rows, dist, counts = (as_numpy(a) for a in (s.verlet_list, s.distance_list, s.neighbor_number))
    model = unep._model((1, 3, 7))
    only_e = np.full(n, np.nan)
    K.nep.calculate(*cols, types, type_map, *where, rows, dist, counts, model, energy=only_e)
    assert np.array_equal(only_e, e)
    only_f, only_q = np.full((n, 3), np.nan), np.full((n, 35), np.nan)
    K.nep.calculate(*cols, types, type_map, *where, rows, dist, counts, model, force=only_f, descriptor=only_q)
    assert np.array_equal(only_f, f) and np.array_equal(only_q, q)
    up = lambda a: HArray(torch.from_numpy(np.ascontiguousarray(a)).cuda())
    dev_v, dev_l = up(np.full((n, 9), np.nan)), up(np.full((n, 80), np.nan))
    K.nep.calculate(*(up(c) for c in cols), up(types), type_map, *where, s.verlet_list, s.distance_list, s.neighbor_number, model,
                    virial=dev_v, latent=dev_l)
    assert np.array_equal(dev_v.numpy(), v) and np.array_equal(dev_l.numpy(), unep.get_latentspace(s.data, s.box))
    # a type the model was not compacted for contributes nothing and receives zeros
    type_map[3], type_map[7] = -1, 1
    out = dict(energy=np.full(n, np.nan), force=np.full((n, 3), np.nan), virial=np.full((n, 9), np.nan))
    K.nep.calculate(*cols, types, type_map, *where, rows, dist, counts, unep._model((1, 7)), **out)
    cr = types == 3
    assert cr.any() and not out["energy"][cr].any() and not out["force"][cr].any() and np.isfinite(out["force"]).all()
    with pytest.raises(ValueError):
        K.nep.calculate(*cols[:2], cols[2][:-1], types, type_map, *where, rows, dist, counts, model, energy=only_e)
    with pytest.raises(ValueError):
        K.nep.calculate(*cols, types, type_map, *where, rows, dist, counts, model, force=np.zeros((n, 9)))
    with pytest.raises(ValueError):
        K.nep.calculate(*cols, types, type_map, *where, rows, dist, counts, model, virial_sum=np.zeros(9))
