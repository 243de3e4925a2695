"""The NEP calculator on the CPU: the reader, the host layer (``System.calc``, the replica and twin paths, ``FIRE``) with the neighbour
build routed to the oracle (fixture ``oracle_backend``) and ``kernels.nep`` replaced by the numpy restatement of tests/_nep_ref.py;
and the restatement itself against the reference's fixtures (pynep, LAMMPS, ASE's FIRE2: tests/golden/nep/README.md) and against
physics it did not produce itself: the addition theorem, the energy's gradient, the strained box."""
import gzip
import os

import numpy as np
import pytest

import _eam_ref
import _nep_ref
import mdapy_amd as mp

GOLDEN = _nep_ref.GOLDEN
ALCRNI = os.path.join(os.path.dirname(GOLDEN), "input_files", "AlCrNi.xyz")
ELEMENTS16 = ["Ag", "Al", "Au", "Cr", "Cu", "Mg", "Mo", "Ni", "Pb", "Pd", "Pt", "Ta", "Ti", "V", "W", "Zr"]


@pytest.fixture
def restated(oracle_backend, monkeypatch):
    import mdapy_amd.kernels as K

    monkeypatch.setattr(K, "nep", _nep_ref)
    monkeypatch.setitem(_nep_ref.calls, "calculate", 0)
    return _nep_ref


@pytest.fixture(scope="module")
def unep():
    return mp.NEP(_nep_ref.UNEP)


@pytest.fixture(scope="module")
def variants(tmp_path_factory):
    """name -> (the NEP read back, what write_model wrote)"""
    where = tmp_path_factory.mktemp("nep_models")
    out = {}
    for k, (name, how) in enumerate(_nep_ref.VARIANTS.items()):
        path = str(where / f"{name}.txt")
        wrote = _nep_ref.write_model(path, seed=k, **how)
        out[name] = (mp.NEP(path), wrote)
    return out


def _system(pos, box, names, calc=None, boundary=None):
    s = mp.System(pos=pos, box=box if boundary is None else mp.Box(box, boundary))
    s.set_element(names)
    if calc is not None:
        s.calc = calc
    return s


def _cell32(seed, elements=("Al", "Cr", "Ni"), rattle=0.1):
    """2 x 2 x 2 fcc cells, a = 3.6 A: 32 atoms in a 7.2 A box (every model's cutoff makes it a replica), rattled"""
    pos, box, names = _eam_ref.hea(2, list(elements), [1.0 / len(elements)] * len(elements), False)
    return pos + np.random.default_rng(seed).normal(0, rattle, pos.shape), np.array(box, float)[:3], names


def _close_pairs(seed, elements=("Al", "Cr", "Ni")):
    """the 32-atom cell with one pair 0.8 A apart and one 1.5 A apart: inside ZBL's inner radius and inside its switch"""
    pos, box, names = _cell32(seed, elements)
    pos[1] = pos[0] + np.array([0.8, 0.0, 0.0])
    pos[9] = pos[8] + np.array([0.0, 1.5, 0.0])
    return pos, box, names


def _energy(pos, box, names, calc):
    """the restatement's total energy alone (pass A) on a System's list"""
    s = _system(pos, box, names)
    s._require_cutoff_list(calc.rc, None)
    return float(_nep_ref.on_system_list(s, calc, want=("energy",))["energy"].sum())


# ---------------------------------------------------------------------------------------------- the reader
def test_reader_unep(unep):
    info = unep.info
    assert (info["version"], info["zbl"], info["model_type"], info["charge_mode"]) == (4, True, 0, 0)
    assert (info["radial_cutoff"], info["angular_cutoff"], unep.rc) == (6.0, 5.0, 6.0)
    assert (info["n_max_radial"], info["n_max_angular"], info["basis_size_radial"], info["basis_size_angular"]) == (4, 4, 8, 8)
    assert (info["l_max_3body"], info["l_max_4body"], info["l_max_5body"]) == (4, 2, 1)
    assert (info["num_ndim"], info["num_nlatent"]) == (35, 80) and info["element_list"] == ELEMENTS16
    with gzip.open(_nep_ref.UNEP, "rt") as f:
        lines = [line for line in f.read().split("\n") if line.strip()]
    assert info["num_para"] == len(lines) - 7 - 35 == 70401  # seven head lines, then the parameters, then the 35 scalers
    assert (unep.zbl_mode, unep.zbl_inner, unep.zbl_outer) == (1, 1.0, 2.0) and unep.results == {}
    assert float(lines[7]) == unep.w0[0][0, 0] and float(lines[-1]) == unep.q_scaler[-1]
    assert issubclass(mp.NEP, mp.CalculatorMP)
    for getter in (unep.get_charges, unep.get_bec):
        with pytest.raises(ValueError, match="only available for qNEP"):
            getter(None, None)
    with pytest.raises(FileNotFoundError):
        mp.NEP("no_such_model.txt")


@pytest.mark.parametrize("name", list(_nep_ref.VARIANTS))
def test_reader_reads_back_what_was_written(variants, name):
    nep, wrote = variants[name]
    T, H, dim, version = len(wrote["elements"]), wrote["neurons"], wrote["dim"], wrote["version"]
    info = nep.info
    assert info["version"] == version and info["element_list"] == wrote["elements"] and info["num_ndim"] == dim and info["num_nlatent"] == H
    assert (info["l_max_3body"], info["l_max_4body"], info["l_max_5body"]) == tuple(wrote["l_max"])
    assert info["num_para"] == len(wrote["numbers"]) and np.array_equal(nep.q_scaler, wrote["scalers"])
    assert info["zbl"] == bool(wrote["zbl"]) and nep.zbl_mode == (0 if not wrote["zbl"] else len(wrote["zbl"]) - 1)
    cut = wrote["cutoffs"]
    assert np.array_equal(nep.rc_radial, np.broadcast_to(cut[:, 0], (T,))) and np.array_equal(nep.rc_angular, np.broadcast_to(cut[:, 1], (T,)))
    assert nep.rc == cut.max()
    numbers, per = wrote["numbers"], H * (dim + 2) + (version == 5)
    for t in range(T):
        net = numbers[(0 if version == 3 else t) * per:][:per]
        assert np.array_equal(nep.w0[t].ravel(), net[:H * dim]) and np.array_equal(nep.b0[t], net[H * dim:H * dim + H])
        assert np.array_equal(nep.w1[t], net[H * dim + H:H * dim + 2 * H]) and nep.bias[t] == (net[-1] if version == 5 else 0.0)
    assert nep.b1 == numbers[wrote["n_ann"] - 1]
    NR, KR = wrote["n_max"][0] + 1, wrote["basis"][0] + 1
    c = numbers[wrote["n_ann"]:]
    for (n, k, a, b) in ((0, 0, 0, 0), (NR - 1, KR - 1, T - 1, 0), (1, 2, 0, T - 1)):  # c[n][k][t1][t2] in the file
        assert nep.c_radial[a, b, n, k] == c[((n * KR + k) * T + a) * T + b]
    NA, KA = wrote["n_max"][1] + 1, wrote["basis"][1] + 1
    assert nep.c_angular[T - 1, 0, NA - 1, 1] == c[T * T * NR * KR + (((NA - 1) * KA + 1) * T + T - 1) * T]


def test_reader_errors(tmp_path):
    good = tmp_path / "good.txt"
    _nep_ref.write_model(str(good), zbl=(1.0, 2.0))
    lines = good.read_text().split("\n")
    assert mp.NEP(str(good)).info["zbl"]

    def model(changed, name="bad.txt"):
        (tmp_path / name).write_text("\n".join(changed))
        return str(tmp_path / name)

    with pytest.raises(ValueError, match="ended at line"):
        mp.NEP(model(lines[:200]))
    with pytest.raises(ValueError, match="ended at line"):
        mp.NEP(model(lines[:4]))
    with pytest.raises(ValueError, match=r"line 1: 3 element symbols expected, 2 found: 'nep4_zbl 3 Al Cr'"):
        mp.NEP(model(["nep4_zbl 3 Al Cr"] + lines[1:]))
    with pytest.raises(ValueError, match="line 1: 'nep9' is no NEP model"):
        mp.NEP(model(["nep9 3 Al Cr Ni"] + lines[1:]))
    with pytest.raises(ValueError, match="line 1: 'mep4' is no NEP model"):
        mp.NEP(model(["mep4 3 Al Cr Ni"] + lines[1:]))
    with pytest.raises(ValueError, match="line 3: expected 'cutoff'"):
        mp.NEP(model(lines[:2] + ["cutoff 5 4 100"] + lines[3:]))
    with pytest.raises(ValueError, match="line 50: not a number: 'abc'"):
        mp.NEP(model(lines[:49] + ["abc"] + lines[50:]))
    for head, what in (("nep4_dipole", "dipole"), ("nep3_polarizability", "polarizability"), ("nep4_charge2", "charge"), ("nep4_zbl_charge1", "charge")):
        with pytest.raises(NotImplementedError, match=what):
            mp.NEP(model([head + " 3 Al Cr Ni"] + lines[1:]))
    with pytest.raises(NotImplementedError, match="flexible ZBL"):
        mp.NEP(model(lines[:1] + ["zbl 0 0"] + lines[2:]))
    with pytest.raises(NotImplementedError, match="l_max 5"):
        mp.NEP(model(lines[:5] + ["l_max 5 2 1"] + lines[6:]))
    packed = tmp_path / "good.txt.gz"
    with gzip.open(packed, "wt") as f:
        f.write("\n".join(lines))
    a, b = mp.NEP(str(good)), mp.NEP(str(packed))
    assert np.array_equal(a.c_angular, b.c_angular) and np.array_equal(a.w0[2], b.w0[2]) and a.info == b.info


def test_model_block_is_compacted_to_the_types_present(unep):
    head, zbl, block = unep._model_arrays((1, 3, 7))  # Al, Cr, Ni
    m = _nep_ref.Model(head, zbl, block).unpack()
    assert m["T"] == 3 and list(m["z"]) == [13.0, 24.0, 28.0] and m["dim"] == 35
    assert m["c_r"].nbytes + m["c_a"].nbytes == 2 * 9 * 5 * 9 * 8 == 6480 and sum(w.nbytes for w in m["w0"]) == 3 * 80 * 35 * 8 == 67200
    assert np.array_equal(m["c_a"][0, 2], unep.c_angular[1, 7]) and np.array_equal(m["w0"][1], unep.w0[3])
    assert unep.c_radial.nbytes + unep.c_angular.nbytes == 184320


# ---------------------------------------------------------------------------------------------- the reference's fixtures
def test_pynep_fixture_through_system_calc(restated, unep):
    """tests/test_nep.py::test_nep_reference with its own criterion, np.allclose at its defaults.  Measured here (restatement):
    energies 1.8e-14, forces 6.1e-14, stress 3.9e-16, descriptor 2.1e-15, latent 2.1e-15 (largest absolute differences)"""
    want = np.load(os.path.join(GOLDEN, "nep.npz"))
    s = mp.System(ALCRNI)
    s.calc = unep
    got = {"energies": s.get_energies(), "forces": s.get_force(), "stress": s.get_stress(),
           "descriptor": unep.get_descriptor(s.data, s.box), "latent": unep.get_latentspace(s.data, s.box)}
    assert s.N == 72 and s.box.triclinic and s._enlarge_data.shape[0] > 72  # 6.97 A wide: the replica path
    assert got["descriptor"].shape == (72, 35) and got["latent"].shape == (72, 80) and got["forces"].shape == (72, 3)
    for name in got:
        print(f"pynep {name}: max abs difference {np.abs(got[name] - want[name]).max():.3e}")
    for name in got:
        assert np.allclose(got[name], want[name]), name
    assert s.get_energy() == got["energies"].sum()


@pytest.mark.parametrize("index", [0, 1])
def test_lammps_fixture_through_system_calc(restated, unep, index):
    """tests/test_nep.py::test_nep_lmp.  System 0 is build_hea(["Al","Cr","Ni"], [1/3,1/3,1/3], "fcc", a=3.6, 3,3,3, random_seed=1),
    which _eam_ref.hea regenerates (the energies below would not agree otherwise).  Measured here: sys0 energies 1.4e-14, forces
    6.2e-15, stress 5.2e-09, virials 2.6e-07; sys1 energies 2.8e-14, forces 1.1e-13, stress 6.9e-09, virials 6.5e-07 (the virials
    and the stress carry the precision LAMMPS recorded them with)."""
    want = np.load(os.path.join(GOLDEN, "nep_lmp.npz"))
    if index == 0:
        pos, box, names = _eam_ref.hea(3, ["Al", "Cr", "Ni"], [1 / 3, 1 / 3, 1 / 3], False)
        s = _system(pos, box, names, unep)
        assert s.N == 108
    else:
        s = mp.System(ALCRNI)
        s.calc = unep
    got = {"energies": s.get_energies(), "forces": s.get_force(), "stress": s.get_stress(), "virials": s.get_virials()}
    for name in got:
        print(f"lammps sys{index} {name}: max abs difference {np.abs(got[name] - want[f'sys{index}__{name}']).max():.3e}")
    for name in got:
        assert np.allclose(got[name], want[f"sys{index}__{name}"]), name


# ---------------------------------------------------------------------------------------------- the addition theorem
@pytest.mark.parametrize("neighbours", [2, 3])
def test_three_body_invariants_are_legendre_sums(restated, variants, neighbours):
    """q_n^l = (2l+1)/(4 pi) sum_jk g_n(r_j) g_n(r_k) P_l(cos theta_jk), j and k over all neighbours (j = k included), with numpy's
    Legendre polynomials.  The factor (2l+1)/(4 pi) is the reference's normalisation: it is fixed by the descriptor of the pynep
    fixture above, which holds with it and with no other.  Sums of at most nine terms of size |g|^2: within 64 eps of their size."""
    nep, wrote = variants["nep3"]
    rng = np.random.default_rng(neighbours)
    around = rng.normal(size=(neighbours, 3))
    around *= (np.array([2.1, 2.9, 3.6])[:neighbours] / np.linalg.norm(around, axis=1))[:, None]
    pos = np.vstack([np.zeros((1, 3)), around]) + 20.0
    names = np.array(["Cr"] + ["Al", "Ni", "Cr"][:neighbours], dtype=object)
    s = _system(pos, np.eye(3) * 40.0, names, nep, boundary=[0, 0, 0])
    q = nep.get_descriptor(s.data, s.box)[0] / nep.q_scaler
    NR, NA = nep.info["n_max_radial"] + 1, nep.info["n_max_angular"] + 1
    d = np.linalg.norm(around, axis=1)
    tj = np.array([nep.element_list.index(e) for e in names[1:]])
    g_r, _ = _nep_ref.radial_functions(d, np.full(neighbours, 5.0), nep.c_radial[1, tj])
    g_a, _ = _nep_ref.radial_functions(d, np.full(neighbours, 4.0), nep.c_angular[1, tj])
    assert np.all(np.abs(q[:NR] - g_r.sum(0)) <= 64 * np.finfo(float).eps * np.abs(g_r).sum(0))
    cos = (around @ around.T) / np.outer(d, d)
    for l in range(1, 5):
        P = np.polynomial.legendre.legval(cos, [0] * l + [1])
        want = (2 * l + 1) / (4 * np.pi) * np.einsum("jn,kn,jk->n", g_a, g_a, P)
        size = (2 * l + 1) / (4 * np.pi) * np.einsum("jn,kn->n", np.abs(g_a), np.abs(g_a))
        got = q[NR + (l - 1) * NA:NR + l * NA]
        print(f"l = {l}: |q - sum| / size = {(np.abs(got - want) / size).max():.2e}")
        assert np.all(np.abs(got - want) <= 64 * np.finfo(float).eps * size) and np.abs(want).max() > 1e-3


def test_weights_have_their_closed_form():
    """W_k of the restatement, from the addition theorem, against the closed rational factors the kernels carry"""
    factors = [1, 1, 1, 1 / 4, 3, 3, 3 / 4, 3 / 4, 1 / 4, 3 / 8, 3 / 8, 15 / 4, 15 / 4, 5 / 8, 5 / 8, 1 / 64, 5 / 8, 5 / 8, 5 / 16, 5 / 16, 35 / 8, 35 / 8,
               35 / 64, 35 / 64]
    want = np.array(factors) * (2 * _nep_ref.L_OF_K + 1) / (4 * np.pi)
    assert np.allclose(_nep_ref.W, want, rtol=4e-16, atol=0)


# ---------------------------------------------------------------------------------------------- forces and virials are derivatives
H = 1e-4
CASES = ["unep", "unep_close"] + list(_nep_ref.VARIANTS) + ["nep5_zbl_close", "zbl_factor_close"]


def _case(name, unep, variants):
    close = name.endswith("_close")
    key = name[:-6] if close else name
    calc = unep if key == "unep" else variants[key][0]
    elements = ("Al", "Ni") if key == "wide" else ("Al", "Cr", "Ni")
    pos, box, names = (_close_pairs if close else _cell32)(31, elements)
    return calc, pos, box, names


@pytest.mark.parametrize("name", CASES)
def test_forces_are_the_energy_gradient(restated, unep, variants, name):
    """central differences of the restatement's total energy, step 1e-4 A, every coordinate of 6 atoms (in the close-pair frames
    the four atoms of the two pairs among them), against -f: within 1e-6 of the largest force.  The difference is h^2 E''' / 6 plus
    eps E / h.  Measured here: at most 1.1e-08 of the largest force in the fcc frames, 5.8e-08 in the close-pair frames."""
    calc, pos, box, names = _case(name, unep, variants)
    s = _system(pos, box, names, calc)
    f = s.get_force()
    worst, largest = 0.0, np.abs(f).max()
    for atom in (0, 1, 8, 9, 17, 30):
        for axis in range(3):
            e = []
            for sign in (+1.0, -1.0):
                moved = pos.copy()
                moved[atom, axis] += sign * H
                e.append(_energy(moved, box, names, calc))
            worst = max(worst, abs((e[0] - e[1]) / (2.0 * H) + f[atom, axis]))
    print(f"{name}: max |dE/dx + f| = {worst:.3e} eV/A = {worst / largest:.3e} of the largest force {largest:.4g}")
    assert largest > (50.0 if name.endswith("_close") and calc.info["zbl"] else 0.05)
    assert worst <= 1e-6 * largest


@pytest.mark.parametrize("name", CASES)
def test_virial_sum_is_the_strain_derivative(restated, unep, variants, name):
    """r -> (1 + h E_ab) r for the six (a, b) = xx, yy, zz, yz, xz, xy: -dE/dh = sum_i virial_i[b, a], to the same bound relative to
    the largest entry of the summed virial.  Measured here: at most 2.9e-07 (fcc), 4.2e-08 (close pairs)."""
    calc, pos, box, names = _case(name, unep, variants)
    s = _system(pos, box, names, calc)
    total = s.get_virials().sum(0).reshape(3, 3)
    assert np.allclose(s.get_stress(), _eam_ref.stress_of(total.ravel(), s.box.volume), rtol=1e-12, atol=1e-15)
    worst, largest = 0.0, np.abs(total).max()
    for a, b in ((0, 0), (1, 1), (2, 2), (1, 2), (0, 2), (0, 1)):
        e = []
        for sign in (+1.0, -1.0):
            F = np.eye(3)
            F[a, b] += sign * H
            e.append(_energy(pos @ F.T, np.diag(box) @ F.T if np.ndim(box) == 1 else box @ F.T, names, calc))
        worst = max(worst, abs(-(e[0] - e[1]) / (2.0 * H) - total[b, a]))
    print(f"{name}: max |-dE/dh - W| = {worst:.3e} eV = {worst / largest:.3e} of the largest entry {largest:.4g}")
    assert worst <= 1e-6 * largest


# ---------------------------------------------------------------------------------------------- invariances
def test_replicated_cell_gives_the_tiled_energies(restated, unep):
    s = mp.System(ALCRNI)
    s.calc = unep
    e, f = s.get_energies(), s.get_force()
    pos = s.data.select("x", "y", "z").to_numpy()
    names = np.asarray(s.data["element"].to_numpy())
    cell = s.box.box
    shifts = [i * cell[0] + j * cell[1] + k * cell[2] for i in range(2) for j in range(2) for k in range(2)]
    big = _system(np.vstack([pos + t for t in shifts]), mp.Box(2.0 * cell), np.tile(names, 8), unep)
    assert "_enlarge_data" not in big.__dict__  # 13.9 A wide: no replica
    # the same neighbourhoods, summed in another list's order: to the rounding of sums of ~80 terms
    assert np.abs(big.get_energies() - np.tile(e, 8)).max() < 1e-11 and np.abs(big.get_force() - np.tile(f, (8, 1))).max() < 1e-11


def test_shuffled_frame_gives_the_permuted_results(restated, unep, monkeypatch):
    monkeypatch.setenv("MDAPY_SPATIAL_SORT", "1")
    pos, box, names = _eam_ref.hea(5, ["Al", "Cr", "Ni"], [0.3, 0.3, 0.4], False)  # 18 A: wide enough for a twin
    pos = pos + np.random.default_rng(5).normal(0, 0.1, pos.shape)
    order = np.random.default_rng(6).permutation(len(pos))
    s = _system(pos[order], box, names[order], unep)
    e, f, v, stress = s.get_energies(), s.get_force(), s.get_virials(), s.get_stress()
    assert s._spatial() is not None and s._twin.shown.mirror is s.verlet_list
    want = _nep_ref.on_system_list(s, unep)  # on the translated rows, in the shuffled numbering
    # (numpy's matrix products round a row's sums differently at another place of the batch: equal to rounding, not to the bit)
    for got, name in ((e, "energy"), (f, "force"), (v, "virial")):
        assert np.abs(got - want[name]).max() <= 1e-12 * np.abs(want[name]).max(), name
    q = unep.get_descriptor(s.data, s.box)
    monkeypatch.setenv("MDAPY_SPATIAL_SORT", "0")
    plain = _system(pos, box, names, unep)
    assert np.abs(e - plain.get_energies()[order]).max() < 1e-11 and np.abs(f - plain.get_force()[order]).max() < 1e-11
    assert np.allclose(stress, plain.get_stress(), rtol=1e-10, atol=1e-13)
    assert np.abs(q - unep.get_descriptor(plain.data, plain.box)[order]).max() < 1e-12


def test_isolated_atom(restated, unep, variants):
    for calc, element in ((unep, "Ni"), (variants["nep5_zbl"][0], "Cr")):
        pos = np.array([[10.0, 10.0, 10.0], [30.0, 30.0, 30.0]])
        s = _system(pos, np.eye(3) * 40.0, [element, "Al"], calc, boundary=[0, 0, 0])
        t = calc.element_list.index(element)
        at_zero = float((calc.w1[t] * np.tanh(-calc.b0[t])).sum() - calc.b1 - calc.bias[t])  # the network at q = 0
        assert abs(s.get_energies()[0] - at_zero) < 1e-13 and not s.get_force().any() and not s.get_virials().any()
        assert not calc.get_descriptor(s.data, s.box).any()


def test_host_layer_paths(restated, unep):
    pos, box, names = _cell32(40)
    s = _system(pos, box, names, unep)
    first = s.get_energies()
    for getter in (s.get_energy, s.get_force, s.get_stress, s.get_virials, s.get_energies):
        getter()
    assert restated.calls["calculate"] == 1 and s.get_energies() is first and s.rc == 6.0
    assert sorted(unep.results) == ["energies", "forces", "stress", "virials"]
    want = _nep_ref.on_system_list(s, unep)
    assert np.array_equal(first, want["energy"]) and np.array_equal(s.get_force(), want["force"]) and first.shape == (32,)
    alone = mp.NEP(_nep_ref.UNEP)
    assert np.array_equal(alone.get_forces(s.data, s.box), s.get_force()) and alone.get_energy(s.data, s.box) == s.get_energy()
    bare = mp.System(pos=pos, box=box)
    bare.calc = unep
    with pytest.raises(AssertionError, match="data must contain element property."):
        bare.get_energies()
    odd = names.copy()
    odd[3] = "Fe"
    with pytest.raises(AssertionError, match="NEP model did not include Fe."):
        _system(pos, box, odd, unep).get_force()


# ---------------------------------------------------------------------------------------------- FIRE
MODES = [(False, False, None, False, False, 0), (True, False, None, False, False, 0), (False, True, None, False, False, 0),
         (True, True, None, False, False, 0), (False, True, [1, 0, 0, 0, 0, 0], False, False, 0), (False, True, None, True, False, 0),
         (False, True, None, False, True, 0), (False, True, None, False, False, 1)]


@pytest.mark.parametrize("mode", range(8))
def test_fire_against_ase(restated, unep, mode):
    """tests/test_minimize.py: ASE's FIRE2 (UnitCellFilter with optimize_cell) under UNEP-v1 for 5 steps, np.allclose at its defaults"""
    use_abc, optimize_cell, mask, hydro, const_v, p = MODES[mode]
    want = np.load(os.path.join(GOLDEN, "minimize.npz"))
    s = mp.System(ALCRNI)
    s.calc = unep
    fire = mp.FIRE(s, use_abc=use_abc, optimize_cell=optimize_cell, mask=mask, hydrostatic_strain=hydro, constant_volume=const_v,
                   scalar_pressure=p, device=False)
    fire.run(steps=int(want["steps"]), show_process=False)
    got = {"stress": s.get_stress(), "forces": s.get_force(), "energies": s.get_energies()}
    for name in got:
        print(f"mode {mode} {name}: max abs difference {np.abs(got[name] - want[f'mode_{mode}__{name}']).max():.3e}")
    for name in got:
        assert np.allclose(got[name], want[f"mode_{mode}__{name}"]), name


# ---------------------------------------------------------------------------------------------- the C entry's argument errors
def test_argument_errors_need_no_device():
    """the C entry refuses bad arguments before any device work (the same calls are made on the GPU in test_gpu_nep.py)"""
    from mdapy_amd import _lib

    tried = 0
    for bad, code in _nep_ref.argument_error_calls(_lib.lib()):
        assert code == _lib.ERR_ARG, bad
        with pytest.raises(ValueError):
            _lib.check(code)
        tried += 1
    assert tried >= 20
