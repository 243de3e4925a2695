"""The charge-aware NEP calculator on the GPU (mdapy_amd/csrc/nep_charge.hip): energies, forces, virials, charges and Born effective
charges against the numpy restatement (tests/_qnep_ref.py) run on the list the System holds, GPUMD's recorded predictions through
``System.calc``, exactness (the same bits twice, the fixed-order stress sum), ``FIRE`` with its state in HBM, and the raw shim.

The device's tanh, sincos, erfc and exp are not numpy's, so the comparison with the restatement is no bitwise one: for every case
``max |gpu - restatement| / max |restatement|`` per quantity is printed and must stay below ``BOUND`` (profiles/qnep.md holds the
measured values)."""
import os

import numpy as np
import pytest

import _eam_ref
import _nep_ref
import _qnep_ref
import mdapy_amd as mp
from mdapy_amd.devarray import as_numpy

pytestmark = pytest.mark.gpu

GOLDEN = _qnep_ref.GOLDEN
EPS = np.finfo(np.float64).eps
# 16 times the largest value measured on an MI355X over all cases below (profiles/qnep.md), and never above 1e-9: a larger
# difference is another algorithm, not rounding
BOUND = 9.8e-14
QUANTITIES = ("energy", "force", "virial", "charge", "bec")
# cutoffs of 6 and 5 A, as UNEP-v1 has them: the 10.8 A box of the 108-atom alloy is a thin one
MODELS = {"charge1": dict(charge_mode=1, cutoffs=(6.0, 5.0)), "charge2": dict(charge_mode=2, cutoffs=(6.0, 5.0)),
          "charge3": dict(charge_mode=3, cutoffs=(6.0, 5.0)), "zbl_charge1": dict(charge_mode=1, zbl=(1.0, 2.0)),
          "typewise_cutoffs": dict(charge_mode=1, cutoffs=((5.0, 4.0), (4.5, 3.5), (4.8, 4.2)), neurons=4)}


@pytest.fixture(autouse=True)
def _need_gpu():
    from mdapy_amd import _lib

    if _lib.device_count() < 1:
        pytest.fail("test_gpu_qnep needs a HIP device")


@pytest.fixture(scope="module")
def models(tmp_path_factory):
    where = tmp_path_factory.mktemp("qnep_models")
    out = {}
    for k, (name, how) in enumerate(MODELS.items()):
        path = str(where / f"{name}.txt")
        _qnep_ref.write_model(path, seed=100 + k, **how)
        out[name] = mp.QNEP(path)
    return out


@pytest.fixture(scope="module")
def frames():
    return list(mp.Trajectory(os.path.join(GOLDEN, "train.xyz.gz"), verbose=False))


def _system(pos, box, names, calc):
    s = mp.System(pos=pos, box=box)
    s.set_element(names)
    s.calc = calc
    return s


def _alloy(cells=5, seed=0, rattle=0.1):
    """rattled fcc alloy: 5 x 5 x 5 cells are 500 atoms (no multiple of the 8 atoms of a workgroup, nor of the 64 of the k-space
    pass) in an 18 A box"""
    pos, box, names = _eam_ref.hea(cells, ["Al", "Cr", "Ni"], [1.0 / 3] * 3, False)
    return pos + np.random.default_rng(seed).normal(0, rattle, pos.shape), np.array(box, float)[:3], names


def _check(s, label):
    """everything the calculator gives for ``s``, each quantity within BOUND of the restatement on the System's own list"""
    calc = s.calc
    calc.results = {}
    got = {"energy": s.get_energies(), "force": s.get_force(), "virial": s.get_virials(), "charge": calc.get_charges(s.data, s.box),
           "bec": calc.get_bec(s.data, s.box)}
    stress = s.get_stress()
    want = _qnep_ref.on_system_list(s, calc, want=QUANTITIES)
    shapes = {"energy": (s.N,), "force": (s.N, 3), "virial": (s.N, 9), "charge": (s.N,), "bec": (s.N, 9)}
    figures = {}
    for name in QUANTITIES:
        g, w = got[name], want[name]
        assert isinstance(g, np.ndarray) and g.dtype == np.float64 and g.shape == shapes[name] and np.isfinite(g).all(), name
        figures[name] = float(np.abs(g - w).max() / np.abs(w).max())
    print(f"closeness {label}: " + ", ".join(f"{name} {figures[name]:.2e}" for name in QUANTITIES))
    for name in QUANTITIES:
        assert figures[name] <= BOUND, (name, figures[name])
    assert abs(got["charge"].sum()) <= s.N * EPS * np.abs(got["charge"]).max()
    total = _nep_ref.exact_column_sums(got["virial"])
    size = np.abs(got["virial"]).sum(axis=0).reshape(3, 3)
    room = ((s.N - 1) * EPS * 0.5 * (size + size.T) / s.box.volume).ravel()[[0, 4, 8, 5, 2, 1]]
    assert np.all(np.abs(stress - _eam_ref.stress_of(total, s.box.volume)) <= room)  # any order of adding N numbers
    return got, stress


# ---------------------------------------------------------------------------------------------- closeness to the restatement
@pytest.mark.parametrize("mode", [1, 2])
def test_a_water_frame(frames, mode):
    calc = mp.QNEP(os.path.join(GOLDEN, f"nep_mode{mode}.txt.gz"))
    s = mp.System(data=frames[0].data, box=frames[0].box)
    s.calc = calc
    got, stress = _check(s, f"water mode{mode}")
    assert s.N == 384 and "_enlarge_data" not in s.__dict__ and np.abs(got["charge"]).max() > 0.1


@pytest.mark.parametrize("name", ["charge1", "charge2", "charge3"])
def test_b_alloy_108_replica(models, name):
    """10.8 A wide under a cutoff of 6 A: the replica of 8 x 108 atoms; the structure factor sums the 108 real ones over the real cell"""
    pos, box, names = _eam_ref.hea(3, ["Al", "Cr", "Ni"], [1 / 3, 1 / 3, 1 / 3], False)
    pos = pos + np.random.default_rng(11).normal(0, 0.05, pos.shape)
    s = _system(pos, box, names, models[name])
    _check(s, f"alloy108 {name}")
    assert s._enlarge_data.shape[0] == 8 * 108


@pytest.mark.parametrize("name", ["charge1", "charge3"])
def test_c_rattled_500(models, name):
    pos, cell, names = _alloy()
    s = _system(pos, cell, names, models[name])
    got, stress = _check(s, f"rattled500 {name}")
    assert len(pos) == 500 and "_enlarge_data" not in s.__dict__ and s.rc == 6.0 and np.abs(got["force"]).max() > 0.5


def test_d_sheared_500(models):
    pos, cell, names = _alloy(seed=1)
    sheared = np.diag(cell) if np.ndim(cell) == 1 else cell.copy()
    sheared[1, 0] = 0.3 * sheared[1, 1]
    sheared[2, 0], sheared[2, 1] = 0.2 * sheared[2, 2], -0.15 * sheared[2, 2]
    tri = (pos @ np.linalg.inv(np.diag(cell) if np.ndim(cell) == 1 else cell)) @ sheared
    s = _system(tri, mp.Box(sheared), names, models["charge1"])
    assert s.box.triclinic
    _check(s, "sheared500")
    k, G = _qnep_ref.k_points(models["charge1"]._ewald_cell(s.box), np.pi / 6.0)
    assert len(k) % 64 != 0 and len(k) % 256 != 0


def test_e_one_open_axis(models):
    pos, cell, names = _alloy(seed=2)
    calc = models["charge1"]
    s = _system(pos, mp.Box(cell, [1, 1, 0]), names, calc)
    _check(s, "open110")
    padded = calc._ewald_cell(s.box)
    assert np.isclose(np.linalg.norm(padded[2]), np.linalg.norm(np.array(s.box.box)[2]) + 18.0)
    counts = as_numpy(s.neighbor_number)[: s.N]
    assert counts.min() < 0.7 * counts.max()


def test_f_shuffled_frame_runs_on_the_twin(models, monkeypatch):
    monkeypatch.setenv("MDAPY_SPATIAL_SORT", "1")
    pos, cell, names = _alloy(seed=7)
    order = np.random.default_rng(8).permutation(len(pos))
    calc = models["charge2"]
    s = _system(pos[order], cell, names[order], calc)
    got, stress = _check(s, "twin")
    assert s._spatial() is not None and s._twin.shown.mirror is s.verlet_list
    monkeypatch.setenv("MDAPY_SPATIAL_SORT", "0")
    plain = _system(pos, cell, names, calc)
    calc.results = {}
    assert np.abs(got["energy"] - plain.get_energies()[order]).max() < 1e-10 and np.abs(got["force"] - plain.get_force()[order]).max() < 1e-10
    assert np.abs(got["charge"] - calc.results["charges"][order]).max() < 1e-12 and np.abs(got["bec"] - calc.results["bec"][order]).max() < 1e-11


def test_g_zbl_charge_model_with_close_pairs(models):
    pos, cell, names = _alloy(cells=4, seed=3)
    pos[1] = pos[0] + np.array([0.8, 0.0, 0.0])
    pos[9] = pos[8] + np.array([0.0, 1.5, 0.0])
    s = _system(pos, cell, names, models["zbl_charge1"])
    got, stress = _check(s, "zbl closepairs")
    assert np.abs(got["force"]).max() > 50.0  # ZBL's repulsion


def test_h_per_type_cutoffs(models):
    pos, cell, names = _alloy(cells=4, seed=5)
    s = _system(pos, cell, names, models["typewise_cutoffs"])
    _check(s, "typewise cutoffs")
    assert "_enlarge_data" not in s.__dict__


# ---------------------------------------------------------------------------------------------- GPUMD's recorded predictions
@pytest.mark.parametrize("mode", [1, 2])
def test_gpumd_fixture(frames, mode):
    """the reference's own comparison at its own tolerance, atol = 1e-4 (tests/_qnep_ref.py::gpumd_differences)"""
    calc = mp.QNEP(os.path.join(GOLDEN, f"nep_mode{mode}.txt.gz"))
    worst = _qnep_ref.gpumd_differences(calc, frames, np.load(os.path.join(GOLDEN, f"gpumd_mode{mode}.npz")))
    print(f"gpumd mode {mode}: " + ", ".join(f"{name} {value:.1e}" for name, value in worst.items()))
    for name, value in worst.items():
        assert value <= 1e-4, name


# ---------------------------------------------------------------------------------------------- exactness
def test_two_runs_give_the_same_bits(models, frames):
    for make in (lambda: _system(*_alloy(seed=6), models["charge1"]),
                 lambda: _system(*_eam_ref.hea(3, ["Al", "Cr", "Ni"], [1 / 3, 1 / 3, 1 / 3], False), models["charge3"])):
        results = []
        for _ in range(2):
            s = make()
            s.calc.results = {}
            results.append([np.array(a) for a in (s.get_energies(), s.get_force(), s.get_virials(), s.get_stress(),
                                                   s.calc.get_charges(s.data, s.box), s.calc.get_bec(s.data, s.box))])
        for a, b in zip(*results):
            assert np.array_equal(a, b)


def test_virial_sum_is_the_fixed_order_sum_of_the_real_rows(models):
    """the raw shim on a replica's list: virial_sum9 adds the first n_real rows and no others, the same bits on every call, within
    (n - 1) eps sum|v| of the exact sum; the stress follows from it"""
    import mdapy_amd.kernels as K
    from mdapy_amd import policy

    calc = models["charge1"]
    pos, box, names = _eam_ref.hea(3, ["Al", "Cr", "Ni"], [1 / 3, 1 / 3, 1 / 3], False)
    s = _system(pos, box, names, calc)
    via_system = s.get_virials()
    cell, frame = s._get_compute_view()
    n = frame.shape[0]
    types = np.array([calc.element_list.index(e) for e in np.asarray(frame["element"].to_numpy()).astype(str)], np.int32)
    type_map = np.arange(3, dtype=np.int32)
    sums = []
    for _ in range(2):
        virial, total = np.full((n, 9), np.nan), np.full(9, np.nan)
        K.nep.calculate_charge(*(as_numpy(c) for c in policy.positions(frame)), types, type_map, cell.box, cell.origin, cell.boundary,
                               as_numpy(s.verlet_list), as_numpy(s.distance_list), as_numpy(s.neighbor_number), calc._model((0, 1, 2)),
                               calc._ewald_cell(s.box), 6.0, virial=virial, virial_sum=total, n_real=108)
        assert np.array_equal(virial[:108], via_system)
        exact = _nep_ref.exact_column_sums(virial[:108])
        assert np.all(np.abs(total - exact) <= 107 * EPS * np.abs(virial[:108]).sum(axis=0))
        sums.append(total)
    assert np.array_equal(sums[0], sums[1])
    assert np.array_equal(s.get_stress(), calc._stress_of_sums(sums[0], s.box.volume))


# ---------------------------------------------------------------------------------------------- FIRE with its state in HBM
def test_fire_on_the_device_against_the_host_path(models):
    got = {}
    for device in (True, False):
        pos, box, names = _eam_ref.hea(3, ["Al", "Cr", "Ni"], [1 / 3, 1 / 3, 1 / 3], False)
        pos = pos + np.random.default_rng(12).normal(0, 0.05, pos.shape)
        s = _system(pos, box, names, models["charge1"])
        fire = mp.FIRE(s, optimize_cell=True, device=device)
        fire.run(steps=5, show_process=False)
        assert fire._hbm == device
        got[device] = {"stress": s.get_stress(), "forces": s.get_force(), "energies": s.get_energies(),
                       "charges": np.array(s.calc.results["charges"]), "bec": np.array(s.calc.results["bec"])}
    for name in got[True]:
        figure = np.abs(got[True][name] - got[False][name]).max() / np.abs(got[False][name]).max()
        print(f"closeness fire {name}: HBM path against host path {figure:.2e}")
        assert figure <= BOUND, (name, figure)


# ---------------------------------------------------------------------------------------------- the raw shim
def test_argument_errors_come_before_device_work():
    from mdapy_amd import _lib

    tried = 0
    for bad, code in _qnep_ref.argument_error_calls(_lib.lib()):
        assert code == _lib.ERR_ARG, bad
        tried += 1
    assert tried >= 25
