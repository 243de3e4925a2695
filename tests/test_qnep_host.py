"""The charge-aware NEP calculator (``QNEP``) on the CPU: the reader, the host layer with the neighbour build routed to the oracle and
``kernels.nep`` replaced by the numpy restatement of tests/_qnep_ref.py; and the restatement itself against GPUMD's recorded
predictions (tests/golden/qnep/README.md) and against physics it did not produce itself: the Madelung constant of rock salt, the
energy's gradient, the strained box."""
import gzip
import os

import numpy as np
import pytest

import _eam_ref
import _nep_ref
import _qnep_ref
import mdapy_amd as mp

GOLDEN = _qnep_ref.GOLDEN
# the seeded small charge models: every charge mode, with and without ZBL
VARIANTS = {"charge1": dict(charge_mode=1), "charge2": dict(charge_mode=2), "charge3": dict(charge_mode=3),
            "zbl_charge1": dict(charge_mode=1, zbl=(1.0, 2.0)), "zbl_charge2": dict(charge_mode=2, zbl=(1.0, 2.0, 0.7)),
            "zbl_charge3": dict(charge_mode=3, zbl=(1.0, 2.0))}


@pytest.fixture
def restated(oracle_backend, monkeypatch):
    import mdapy_amd.kernels as K

    monkeypatch.setattr(K, "nep", _qnep_ref)
    monkeypatch.setitem(_qnep_ref.calls, "calculate", 0)
    return _qnep_ref


@pytest.fixture(scope="module")
def variants(tmp_path_factory):
    """name -> (the QNEP read back, what write_model wrote, the file)"""
    where = tmp_path_factory.mktemp("qnep_models")
    out = {}
    for k, (name, how) in enumerate(VARIANTS.items()):
        path = str(where / f"{name}.txt")
        wrote = _qnep_ref.write_model(path, seed=100 + k, **how)
        out[name] = (mp.QNEP(path), wrote, path)
    return out


@pytest.fixture(scope="module")
def frames():
    return list(mp.Trajectory(os.path.join(GOLDEN, "train.xyz.gz"), verbose=False))


def _system(pos, box, names, calc=None, boundary=None):
    s = mp.System(pos=pos, box=box if boundary is None else mp.Box(box, boundary))
    s.set_element(names)
    if calc is not None:
        s.calc = calc
    return s


def _cell32(seed, rattle=0.1):
    """2 x 2 x 2 fcc cells, a = 3.6 A: 32 atoms in a 7.2 A box (the cutoff of 5 A makes it a replica), rattled"""
    pos, box, names = _eam_ref.hea(2, ["Al", "Cr", "Ni"], [1.0 / 3] * 3, False)
    return pos + np.random.default_rng(seed).normal(0, rattle, pos.shape), np.array(box, float)[:3], names


def _energy(pos, box, names, calc, charge_mean=None):
    """the restatement's total energy alone on a System's list"""
    s = _system(pos, box, names)
    s._require_cutoff_list(calc.rc, None)
    return float(_qnep_ref.on_system_list(s, calc, want=("energy",), charge_mean=charge_mean)["energy"].sum())


# ---------------------------------------------------------------------------------------------- the reader
@pytest.mark.parametrize("mode", [1, 2])
def test_reader_fixture_models(mode):
    calc = mp.QNEP(os.path.join(GOLDEN, f"nep_mode{mode}.txt.gz"))
    info = calc.info
    assert (info["version"], info["zbl"], info["model_type"], info["charge_mode"]) == (4, False, 0, mode)
    assert (info["num_para"], info["num_ndim"], info["num_nlatent"], info["element_list"]) == (2342, 30, 30, ["H", "O"])
    assert (info["radial_cutoff"], info["angular_cutoff"], calc.rc) == (4.0, 4.0, 4.0) and calc.results == {}
    with gzip.open(os.path.join(GOLDEN, f"nep_mode{mode}.txt.gz"), "rt") as f:
        lines = [line for line in f.read().split("\n") if line.strip()]
    assert len(lines) == 6 + 2342 + 30 and float(lines[6]) == calc.w0[0][0, 0] and float(lines[-1]) == calc.q_scaler[-1]
    per = 30 * 33  # w0, b0 and the two rows of w1 of one type
    assert float(lines[6 + 30 * 31]) == calc.w1[0][0] and float(lines[6 + 30 * 32]) == calc.w1_charge[0][0]
    assert float(lines[6 + 2 * per]) == calc.sqrt_epsilon_inf and float(lines[6 + 2 * per + 1]) == calc.b1
    assert isinstance(calc, mp.NEP) and "QNEP" in mp.__all__


@pytest.mark.parametrize("name", list(VARIANTS))
def test_reader_reads_back_what_was_written(variants, name):
    calc, wrote, _ = variants[name]
    T, H, dim = len(wrote["elements"]), wrote["neurons"], wrote["dim"]
    info = calc.info
    assert info["version"] == 4 and info["charge_mode"] == wrote["charge_mode"] and info["num_ndim"] == dim and info["num_nlatent"] == H
    assert info["num_para"] == len(wrote["numbers"]) and np.array_equal(calc.q_scaler, wrote["scalers"])
    assert info["zbl"] == bool(wrote["zbl"]) and calc.zbl_mode == (0 if not wrote["zbl"] else len(wrote["zbl"]) - 1)
    numbers, per = wrote["numbers"], H * (dim + 3)
    for t in range(T):
        net = numbers[t * per:][:per]
        assert np.array_equal(calc.w0[t].ravel(), net[:H * dim]) and np.array_equal(calc.b0[t], net[H * dim:H * dim + H])
        assert np.array_equal(calc.w1[t], net[H * dim + H:H * dim + 2 * H]) and np.array_equal(calc.w1_charge[t], net[H * dim + 2 * H:])
        assert calc.bias[t] == 0.0
    assert calc.sqrt_epsilon_inf == numbers[wrote["n_ann"] - 2] == 1.3 and calc.b1 == numbers[wrote["n_ann"] - 1]
    NR, KR = wrote["n_max"][0] + 1, wrote["basis"][0] + 1
    c = numbers[wrote["n_ann"]:]
    for (n, k, a, b) in ((0, 0, 0, 0), (NR - 1, KR - 1, T - 1, 0), (1, 2, 0, T - 1)):
        assert calc.c_radial[a, b, n, k] == c[((n * KR + k) * T + a) * T + b]
    m = _qnep_ref.Model(*calc._model_arrays((0, 2))).unpack()
    assert m["T"] == 2 and m["charge"] == wrote["charge_mode"] and np.array_equal(m["w1q"][1], calc.w1_charge[2]) and m["sqrt_eps"] == 1.3


def test_reader_errors_and_the_two_doors(variants, tmp_path):
    calc, wrote, path = variants["zbl_charge1"]
    with open(path) as f:
        lines = f.read().split("\n")

    def model(changed, name="bad.txt"):
        (tmp_path / name).write_text("\n".join(changed))
        return str(tmp_path / name)

    plain = tmp_path / "plain.txt"
    _nep_ref.write_model(str(plain), zbl=(1.0, 2.0))
    body = plain.read_text().split("\n")
    # a charge head on a charge-free body: too short by the charge's weights and sqrt(epsilon_inf)
    with pytest.raises(ValueError, match="ended at line"):
        mp.QNEP(model(["nep4_zbl_charge2 3 Al Cr Ni"] + body[1:]))
    with pytest.raises(ValueError, match="ended at line"):
        mp.QNEP(model(lines[:200]))
    with pytest.raises(ValueError, match="line 50: not a number: 'abc'"):
        mp.QNEP(model(lines[:49] + ["abc"] + lines[50:]))
    for head in ("nep4_charge2", "nep4_zbl_charge1", "nep4_charge3"):
        with pytest.raises(NotImplementedError, match=r"charge models .*use mdapy_amd\.QNEP"):
            mp.NEP(model([head + " 3 Al Cr Ni"] + body[1:]))
    for cls in (mp.NEP, mp.QNEP):
        for head, what in (("nep4_dipole", "dipole models"), ("nep3_polarizability", "polarizability models"),
                           ("nep4_temperature", "temperature-dependent models")):
            with pytest.raises(NotImplementedError, match=what):
                cls(model([head + " 3 Al Cr Ni"] + body[1:]))
    with pytest.raises(ValueError, match=r"no charge model; use mdapy_amd\.NEP"):
        mp.QNEP(str(plain))
    with pytest.raises(ValueError, match="'nep3_charge1' is no NEP model"):
        mp.QNEP(model(["nep3_charge1 3 Al Cr Ni"] + lines[1:]))
    with pytest.raises(ValueError, match="'nep4_charge4' is no NEP model"):
        mp.QNEP(model(["nep4_charge4 3 Al Cr Ni"] + lines[1:]))
    with pytest.raises(NotImplementedError, match="flexible ZBL"):
        mp.QNEP(model(lines[:1] + ["zbl 0 0"] + lines[2:]))
    with pytest.raises(FileNotFoundError):
        mp.QNEP("no_such_model.txt")
    # the door by the head line
    from mdapy_amd import nep

    assert type(nep.load(str(plain))) is mp.NEP and type(nep.load(path)) is mp.QNEP
    assert type(nep.load(os.path.join(GOLDEN, "nep_mode2.txt.gz"))) is mp.QNEP and type(nep.load(_nep_ref.UNEP)) is mp.NEP
    with pytest.raises(FileNotFoundError):
        nep.load("no_such_model.txt")
    packed = tmp_path / "charge.txt.gz"
    with gzip.open(packed, "wt") as f:
        f.write("\n".join(lines))
    a, b = mp.QNEP(path), nep.load(str(packed))
    assert type(b) is mp.QNEP and np.array_equal(a.w1_charge[2], b.w1_charge[2]) and a.info == b.info


def test_per_type_cutoffs_are_read(tmp_path):
    wrote = _qnep_ref.write_model(str(tmp_path / "m.txt"), charge_mode=1, cutoffs=((5.0, 4.0), (4.5, 3.5), (4.8, 4.2)), seed=7)
    calc = mp.QNEP(str(tmp_path / "m.txt"))
    assert list(calc.rc_radial) == [5.0, 4.5, 4.8] and list(calc.rc_angular) == [4.0, 3.5, 4.2] and calc.info["radial_cutoff"] == 5.0
    assert calc.info["num_para"] == len(wrote["numbers"])


# ---------------------------------------------------------------------------------------------- GPUMD's recorded predictions
@pytest.mark.parametrize("mode", [1, 2])
def test_gpumd_fixture_through_system_calc(restated, frames, mode):
    """GPUMD's predictions for the three 384-atom water frames at the reference's own tolerance, atol = 1e-4 (GPUMD writes single
    precision).  Measured here (restatement), largest absolute differences over the three frames:
    mode 1: energy 7.0e-07, force 6.8e-05, virial 6.7e-07, charge 7.2e-07, bec 5.3e-06;
    mode 2: energy 2.2e-07, force 6.6e-05, virial 4.8e-07, charge 9.1e-07, bec 6.4e-06"""
    calc = mp.QNEP(os.path.join(GOLDEN, f"nep_mode{mode}.txt.gz"))
    worst = _qnep_ref.gpumd_differences(calc, frames, np.load(os.path.join(GOLDEN, f"gpumd_mode{mode}.npz")))
    print(f"mode {mode}: " + ", ".join(f"{name} {value:.1e}" for name, value in worst.items()))
    for name, value in worst.items():
        assert value <= 1e-4, name
    assert sorted(calc.results) == ["bec", "charges", "energies", "forces", "stress", "virials"]


# ---------------------------------------------------------------------------------------------- the Madelung constant
def test_madelung_constant_of_rock_salt():
    """charges +1 and -1 on a 4 x 4 x 4 rock-salt cell (512 ions, nearest distance 2.8 A): the mode-1 energy per ion pair is
    -K M / d with M = 1.747565.  The format's choice alpha rc = pi truncates the real-space sum at erfc(pi) = 9e-6 and the
    k-space sum at exp(-pi^2): within 1e-4 relative.  Measured here: 1.5e-05 with rc = 6 A."""
    a, n = 5.6, 4
    cells = np.array([(i, j, k) for i in range(2 * n) for j in range(2 * n) for k in range(2 * n)], float)
    pos = cells * (a / 2)
    q = np.where(cells.sum(1) % 2 == 0, 1.0, -1.0)
    E, D, F, V = _qnep_ref.electrostatics(pos, q, np.eye(3) * a * n, 6.0, 1)
    madelung = -E.sum() / (len(q) / 2) * (a / 2) / _qnep_ref.COULOMB
    print(f"Madelung constant {madelung:.8f}: {abs(madelung / 1.747565 - 1):.2e} relative")
    assert abs(madelung / 1.747565 - 1.0) <= 1e-4
    assert np.abs(F).max() < 1e-9 and np.allclose(D * q, 2.0 * E, rtol=1e-12)  # a lattice at rest; E_i = q_i D_i / 2


# ---------------------------------------------------------------------------------------------- forces and virials are derivatives
H = 1e-4
MODES = ["charge1", "charge2", "charge3"]


def _mean_removed(pos, box, names, calc):
    detail = {}
    s = _system(pos, box, names)
    s._require_cutoff_list(calc.rc, None)
    _qnep_ref.on_system_list(s, calc, want=("energy",), detail=detail)
    return detail["charge_mean"]


def _force_gap(calc, held):
    """central differences of the restatement's total energy, step 1e-4 A, every coordinate of 6 atoms, against -f, exactly as
    tests/test_nep_host.py::test_forces_are_the_energy_gradient takes them.  held: the number removed from the charges stays the
    unmoved frame's.  -> (max |dE/dx + f|, the largest force)"""
    pos, box, names = _cell32(31)
    f = _system(pos, box, names, calc).get_force()
    mean = _mean_removed(pos, box, names, calc) if held else None
    worst = 0.0
    for atom in (0, 1, 8, 9, 17, 30):
        for axis in range(3):
            e = []
            for sign in (+1.0, -1.0):
                moved = pos.copy()
                moved[atom, axis] += sign * H
                e.append(_energy(moved, box, names, calc, mean))
            worst = max(worst, abs((e[0] - e[1]) / (2.0 * H) + f[atom, axis]))
    return worst, np.abs(f).max()


def _virial_gap(calc, held):
    """r -> (1 + h E_ab) r for the six (a, b) = xx, yy, zz, yz, xz, xy: -dE/dh against sum_i virial_i[b, a], exactly as
    tests/test_nep_host.py::test_virial_sum_is_the_strain_derivative.  -> (the largest gap, the largest entry of the summed virial)"""
    pos, box, names = _cell32(31)
    s = _system(pos, box, names, calc)
    total = s.get_virials().sum(0).reshape(3, 3)
    assert np.allclose(s.get_stress(), _eam_ref.stress_of(total.ravel(), s.box.volume), rtol=1e-12, atol=1e-15)
    mean = _mean_removed(pos, box, names, calc) if held else None
    worst = 0.0
    for a, b in ((0, 0), (1, 1), (2, 2), (1, 2), (0, 2), (0, 1)):
        e = []
        for sign in (+1.0, -1.0):
            F = np.eye(3)
            F[a, b] += sign * H
            e.append(_energy(pos @ F.T, np.diag(box) @ F.T if np.ndim(box) == 1 else box @ F.T, names, calc, mean))
        worst = max(worst, abs(-(e[0] - e[1]) / (2.0 * H) - total[b, a]))
    return worst, np.abs(total).max()


@pytest.mark.parametrize("name", MODES + ["zbl_charge1"])
def test_forces_are_the_energy_gradient(restated, variants, name):
    """Central differences against -f, within 1e-6 of the largest force.  The energy that is differenced holds the number removed
    from the charges at the unmoved frame's value: the format's forces are D_i dq_i/dr of every atom's own network output, and the
    mean that is removed from the charges is not differentiated.  (GPUMD's recorded forces are met with this convention and with no
    other: with the mean of D subtracted as well, the restatement misses them by up to 8.6e-2 eV/A.)  Measured here: charge1 1.9e-09,
    charge2 2.7e-09, charge3 1.8e-09, zbl_charge1 6.1e-09 of the largest force.  With the mean removed anew in every displaced frame
    the same quotients are 5.1e-04, 1.2e-02 and 4.2e-03: the term of ``test_what_the_format_leaves_out_of_the_forces``."""
    worst, largest = _force_gap(variants[name][0], True)
    print(f"{name}: max |dE/dx + f| = {worst:.3e} eV/A = {worst / largest:.3e} of the largest force {largest:.4g}")
    assert largest > 0.05
    assert worst <= 1e-6 * largest


@pytest.mark.parametrize("name", MODES + ["zbl_charge1"])
def test_virial_sum_is_the_strain_derivative(restated, variants, name):
    """the same for the strained box.  Measured here: charge1 1.1e-08, charge2 3.2e-08, charge3 2.8e-08, zbl_charge1 7.7e-08 of the
    largest entry of the summed virial (9.6e-04, 1.3e-02, 2.2e-03 with the mean removed anew in every strained frame)."""
    worst, largest = _virial_gap(variants[name][0], True)
    print(f"{name}: max |-dE/dh - W| = {worst:.3e} eV = {worst / largest:.3e} of the largest entry {largest:.4g}")
    assert worst <= 1e-6 * largest


@pytest.mark.parametrize("name", MODES)
def test_what_the_format_leaves_out_of_the_forces(restated, variants, name):
    """With the mean c of the charges removed anew in every frame the energy's gradient has one more term, (dE/dc) (dc/dx) with
    dE/dc = -sum_i D_i over the real atoms.  The central difference of that energy must miss -f by exactly this term: to 1e-6 of
    the largest force again.  This pins the convention, and shows that nothing else is missing."""
    calc = variants[name][0]
    pos, box, names = _cell32(31)
    s = _system(pos, box, names, calc)
    f = s.get_force()
    detail = {}
    _qnep_ref.on_system_list(s, calc, want=("energy",), detail=detail)
    slope = -detail["D"][: s.N].sum()
    worst, size = 0.0, 0.0
    for atom, axis in ((0, 0), (9, 1), (30, 2)):
        e, c = [], []
        for sign in (+1.0, -1.0):
            moved = pos.copy()
            moved[atom, axis] += sign * H
            e.append(_energy(moved, box, names, calc))
            c.append(_mean_removed(moved, box, names, calc))
        gap = (e[0] - e[1]) / (2.0 * H) + f[atom, axis]
        term = slope * (c[0] - c[1]) / (2.0 * H)
        worst, size = max(worst, abs(gap - term)), max(size, abs(term))
    print(f"{name}: the missing term is up to {size:.3e} eV/A; what is left beside it {worst:.3e} eV/A")
    assert size > 1e-4 and worst <= 1e-6 * np.abs(f).max()


# ---------------------------------------------------------------------------------------------- invariances
@pytest.mark.parametrize("mode", [1, 2])
def test_charges_sum_to_zero_and_replicated_frame_is_tiled(restated, frames, mode):
    calc = mp.QNEP(os.path.join(GOLDEN, f"nep_mode{mode}.txt.gz"))
    s = mp.System(data=frames[0].data, box=frames[0].box)
    s.calc = calc
    e, f, q, z = s.get_energies(), s.get_force(), calc.get_charges(s.data, s.box), calc.get_bec(s.data, s.box)
    assert restated.calls["calculate"] == 1 and calc.get_charges(s.data, s.box) is q
    assert abs(q.sum()) <= 384 * np.finfo(float).eps * np.abs(q).max() and np.abs(q).max() > 0.1
    pos = s.data.select("x", "y", "z").to_numpy()
    names = np.asarray(s.data["element"].to_numpy())
    cell = np.array(s.box.box)
    big = _system(np.vstack([pos, pos + cell[0]]), mp.Box(cell * np.array([[2.0], [1.0], [1.0]])), np.tile(names, 2), calc)
    calc.results = {}
    E, F = big.get_energies(), big.get_force()
    Q, Z = calc.results["charges"], calc.results["bec"]
    # the same neighbourhoods; twice the k-points, of which every other one has S = 0 to rounding
    for got, want, name in ((E, np.tile(e, 2), "energy"), (F, np.tile(f, (2, 1)), "force"), (Q, np.tile(q, 2), "charge"), (Z, np.tile(z, (2, 1)), "bec")):
        print(f"mode {mode} {name}: replicated against tiled {np.abs(got - want).max():.2e}")
        assert np.abs(got - want).max() < 1e-10, name


def test_shuffled_frame_gives_the_permuted_results(restated, variants, monkeypatch):
    monkeypatch.setenv("MDAPY_SPATIAL_SORT", "1")
    calc = variants["charge1"][0]
    pos, box, names = _eam_ref.hea(5, ["Al", "Cr", "Ni"], [0.3, 0.3, 0.4], False)  # 18 A: wide enough for a twin
    pos = pos + np.random.default_rng(5).normal(0, 0.1, pos.shape)
    order = np.random.default_rng(6).permutation(len(pos))
    s = _system(pos[order], box, names[order], calc)
    e, f, v = s.get_energies(), s.get_force(), s.get_virials()
    q, z = calc.results["charges"].copy(), calc.results["bec"].copy()
    assert s._spatial() is not None and s._twin.shown.mirror is s.verlet_list
    want = _qnep_ref.on_system_list(s, calc)
    for got, name in ((e, "energy"), (f, "force"), (v, "virial"), (q, "charge"), (z, "bec")):
        assert np.abs(got - want[name]).max() <= 1e-11 * np.abs(want[name]).max(), name
    monkeypatch.setenv("MDAPY_SPATIAL_SORT", "0")
    plain = _system(pos, box, names, calc)
    assert np.abs(e - plain.get_energies()[order]).max() < 1e-10 and np.abs(f - plain.get_force()[order]).max() < 1e-10
    assert np.abs(q - calc.results["charges"][order]).max() < 1e-12 and np.abs(z - calc.results["bec"][order]).max() < 1e-11


def test_absent_type_and_isolated_atom(restated, variants):
    calc = variants["charge1"][0]
    pos, box, names = _cell32(3)
    two = np.where(names == "Cr", "Ni", names)  # no Cr in the frame: the block is compacted to Al and Ni
    s = _system(pos, box, two, calc)
    e, f = s.get_energies(), s.get_force()
    want = _qnep_ref.on_system_list(s, calc)
    assert np.array_equal(e, want["energy"]) and np.array_equal(f, want["force"])
    assert np.array_equal(calc.results["bec"], want["bec"]) and len(calc._present[1]) == 2
    q = calc.get_descriptor(s.data, s.box)  # (NEP's further outputs go through the charge pass as well)
    assert q.shape == (32, calc.info["num_ndim"]) and np.abs(q).max() > 0.0 and calc.get_latentspace(s.data, s.box).shape == (32, 6)
    # two atoms out of each other's reach in an open box (periodic for the k-space sum in the padded cell): charges that are
    # each other's negative, BEC tensors that are their charge alone
    far = _system(np.array([[10.0, 10.0, 10.0], [30.0, 30.0, 30.0]]), np.eye(3) * 40.0, ["Ni", "Al"], calc, boundary=[0, 0, 0])
    e = far.get_energies()
    q, z = calc.results["charges"], calc.results["bec"]
    raw = [float((calc.w1_charge[t] * np.tanh(-calc.b0[t])).sum()) for t in (2, 0)]  # the network at a zero descriptor
    assert np.allclose(q, np.array(raw) - np.mean(raw), rtol=1e-13) and abs(q.sum()) < 1e-16
    assert np.allclose(z, q[:, None] * np.eye(3).ravel() * calc.sqrt_epsilon_inf, rtol=1e-13, atol=0) and np.isfinite(e).all()


# ---------------------------------------------------------------------------------------------- the C entry's argument errors
def test_argument_errors_need_no_device():
    """the C entry refuses bad arguments before any device work (the same calls are made on the GPU in test_gpu_qnep.py)"""
    from mdapy_amd import _lib

    tried = 0
    for bad, code in _qnep_ref.argument_error_calls(_lib.lib()):
        assert code == _lib.ERR_ARG, bad
        with pytest.raises(ValueError):
            _lib.check(code)
        tried += 1
    assert tried >= 25
