"""SQS without a GPU: cluster enumeration, tables and the ``SQS`` class with the restatement of tests/_sqs_ref.py installed as
``kernels.sqs``; the host side of the real engine (``mdapy_amd._sqs``: channels, targets, tables) against that restatement; and
the argument checks of the real shim and of the C ABI, which come before any device work."""
import math
from collections import Counter

import numpy as np
import pytest

import _sqs_ref as ref
import mdapy_amd as mp
from mdapy_amd import _sqs
from mdapy_amd.sqs import enumerate_clusters, image_neighbors

EPS = 2.0 ** -53


@pytest.fixture
def restated(monkeypatch):
    import mdapy_amd.kernels as K

    monkeypatch.setattr(K, "sqs", ref)
    return ref


def _system(pos, box, names):
    return mp.System(data={"x": pos[:, 0], "y": pos[:, 1], "z": pos[:, 2], "element": np.array(names, dtype=object)}, box=box)


def _alloy(structure, a, n, elements, ratios, seed):
    """what build_hea gives, without the replication kernel: numpy positions, then build_hea_fromsystem"""
    from mdapy_amd.build_lattice import lattice_positions

    pos, box = lattice_positions(structure, a, *n)
    return mp.build_hea_fromsystem(mp.System(pos=pos, box=box), elements, ratios, seed)


@pytest.fixture(scope="module")
def enumerated():
    return {name: enumerate_clusters(*ref.case(name)[:2], ref.case(name)[4]) for name in ref.CASES}


# ---- ATAT's own cell
def test_atat_structure_and_pairs(restated):
    pos, box, names = ref.atat_cell()
    assert [len(j) for j, _, _ in image_neighbors(pos, box, 1.05)] == [18] * 20
    sqs = mp.SQS(_system(pos, box, names), cutoffs={2: 1.05}, n_replicas=1, max_steps=0, seed=0).compute()
    assert [(c["n_pts"], c["shell"], c["n_instances"]) for c in sqs.channel_info] == [(2, 0, 240)] * 10 + [(2, 1, 120)] * 10
    assert all(c["target"] == 0.0 or abs(c["target"]) < 1e-30 for c in sqs.channel_info)
    ours_mean, ours_max = float(np.abs(sqs.correlations).mean()), float(np.abs(sqs.correlations).max())
    atat_mean, atat_max = ref.atat_summary(2)
    print(f"pairs: mean |corr| {ours_mean:.5f} (ATAT {atat_mean:.5f}), max {ours_max:.4f} (ATAT {atat_max:.4f})")
    assert abs(ours_mean - atat_mean) < 0.005
    assert ours_max < atat_max + 0.02


def test_atat_triplets(restated):
    pos, box, names = ref.atat_cell()
    sqs = mp.SQS(_system(pos, box, names), cutoffs={2: 1.05, 3: 1.05}, n_replicas=1, max_steps=0, seed=0).compute()
    bodies = Counter(c["n_pts"] for c in sqs.channel_info)
    assert bodies[2] == 20 and bodies[3] > 0
    ours = float(np.abs([c["corr"] for c in sqs.channel_info if c["n_pts"] == 3]).mean())
    atat_mean, _ = ref.atat_summary(3)
    print(f"triplets: mean |corr| {ours:.5f} (ATAT {atat_mean:.5f})")
    assert abs(ours - atat_mean) < 0.005


# ---- enumeration and tables: the package's vectorised code against the restatement's loops
@pytest.mark.parametrize("name", sorted(ref.CASES))
def test_enumeration_order(name, enumerated):
    pos, box, _, _, cutoffs = ref.case(name)
    want_body, want_diams, want_map = ref.clusters(pos, box, cutoffs)
    got_body, got_diams, got_map = enumerated[name]
    assert got_diams == want_diams and got_map == want_map
    assert [b[0] for b in got_body] == [b[0] for b in want_body]
    for (_, got, got_d), (_, want, want_d) in zip(got_body, want_body):
        assert got_d == want_d and list(got) == list(want)
        for shell in want:
            assert np.array_equal(got[shell], want[shell]), "instances, in the order they are found"


@pytest.mark.parametrize("name", sorted(ref.CASES))
def test_engine_tables(name, enumerated):
    """the real engine's host side: channels, targets, symmetrised products, multiset lookup, atom -> instance lists"""
    pos, _, types, m, _ = ref.case(name)
    want = ref.restated_engine(name)
    got = ref.build_engine(_sqs.SQSEngine, enumerated[name], len(pos), types, m)
    assert got.num_channels() == want.num_channels() and got.num_instances() == want.num_instances()
    assert [tuple(got.channel_info(c)) for c in range(got.num_channels())] == [tuple(c) for c in want.channels]
    assert got.point_corr == want.point_corr and got.n_func == m - 1
    M = got._model
    N, _, I, G, C, H = (int(v) for v in M["dims"][:6])
    assert (N, C, H) == (len(pos), want.num_channels(), want.n_bins)
    for c in range(C):
        g, body, off = M["chan_i"][c]
        n, first, K = M["group_i"][g][0], M["group_i"][g][2], M["group_i"][g][5]
        assert body == n - 2 and np.array_equal(M["tab"][off:off + K], want.tables[n][2][c - first]), "tab, bit for bit"
    # histograms counted with the package's tables, in numpy
    rng = np.random.default_rng(5)
    for _ in range(3):
        t = rng.permutation(types)
        hist = np.zeros(H, np.int64)
        for e in range(I):
            n, off = M["group_i"][M["inst_group"][e]][:2]
            code = 0
            for a in M["inst_atoms"][e][:n]:
                code = code * m + t[a]
            hist[off + M["msidx"][{2: 0, 3: m * m, 4: m * m + m ** 3}[n] + code]] += 1
        assert np.array_equal(hist, want.histograms(t))
    assert np.all((M["inst_atoms"] >= 0) == (np.arange(4)[None, :] < M["group_i"][M["inst_group"], 0][:, None])), "unused slots, and only those, hold -1"
    for a in range(N):
        mine = M["a2i"][M["a2i_off"][a]:M["a2i_off"][a + 1]]
        assert np.array_equal(mine, np.nonzero((M["inst_atoms"] == a).any(axis=1))[0]), "every instance of an atom, once"


@pytest.mark.parametrize("name", sorted(ref.CASES))
def test_multiset_form_against_per_instance_form(name):
    _, _, types, _, _ = ref.case(name)
    engine = ref.restated_engine(name)
    rng = np.random.default_rng(9)
    bound = np.array([4.0 * (c[3] + math.factorial(c[0])) * EPS for c in engine.channels])
    for k in range(4):
        t = types if k == 0 else rng.permutation(types)
        ours, theirs = engine.corr_from(engine.histograms(t)), ref.per_instance_correlations(engine, t)
        err = np.abs(ours - theirs)
        print(f"{name}: worst |multiset - per instance| {err.max():.2e} (allowed {bound[np.argmax(err)]:.2e})")
        assert np.all(err <= bound)


@pytest.mark.parametrize("mode", [0, 1])
def test_objective_passes_on_arrays_equal_the_plain_loop(mode):
    for name in sorted(ref.CASES):
        engine = ref.restated_engine(name, mode)
        rng = np.random.default_rng(3)
        for scale in (1e-4, 2e-3, 0.05):  # around atat_tol: every d1 branch
            for _ in range(20):
                dc = np.abs(rng.normal(0.0, scale, engine.num_channels()))
                assert engine.objective_fast(dc) == engine.objective_loop(dc)


def test_binary_targets_and_channel_order():
    pos, _, types, m, _ = ref.case("bcc333")
    engine = ref.restated_engine("bcc333")
    assert m == 2 and Counter(types.tolist()) == {0: 13, 1: 41}
    point = -13 / 54 + 41 / 54
    assert engine.point_corr == [pytest.approx(point, abs=1e-15)]
    assert [(c[0], c[1], c[2], c[3]) for c in engine.channels] == [(2, 0, [0, 0], 54 * 8), (2, 1, [0, 0], 54 * 6)]
    assert all(c[4] == engine.point_corr[0] * engine.point_corr[0] and c[4] > 0.26 for c in engine.channels)
    assert engine.shell_diameter[0] < engine.shell_diameter[1]


def test_generator_is_a_pure_function_of_its_arguments():
    seen = {ref.draw(ref.key(s, r, p), n) for s in (0, 1) for r in (0, 1, 7) for p in range(4) for n in (0, 1, 2 ** 40)}
    assert len(seen) == 2 * 3 * 4 * 3
    assert ref.mix(0) == 0 and ref.mix(1) == 0x5692161D100B05E5  # splitmix64's finaliser
    assert all(0 <= ref.index(ref.draw(5, n), 7) < 7 and 0.0 <= ref.uniform(ref.draw(5, n)) < 1.0 for n in range(200))
    t = ref.shuffled(np.arange(50), 3, 2)
    assert sorted(t.tolist()) == list(range(50)) and not np.array_equal(t, np.arange(50))
    assert np.array_equal(t, ref.shuffled(np.arange(50), 3, 2)) and not np.array_equal(t, ref.shuffled(np.arange(50), 3, 1))


# ---- build_hea
def test_build_hea_fromsystem_gives_the_reference_alloy():
    import _eam_ref

    elements, ratios = ["Al", "Cr", "Ni"], [1 / 3, 1 / 3, 1 / 3]
    pos, box, names = _eam_ref.hea(3, elements, ratios, False)
    alloy = _alloy("fcc", 3.6, (3, 3, 3), elements, ratios, 1)
    assert alloy.N == 108 and np.array_equal(alloy.data["element"].to_numpy(), names)
    assert np.array_equal(np.column_stack([alloy.data[c].to_numpy() for c in "xyz"]), pos)
    assert "build_hea" in mp.__all__ and "build_hea_fromsystem" in mp.__all__ and "SQS" in mp.__all__


def test_build_hea_count_rule():
    count = lambda alloy: Counter(alloy.data["element"].to_numpy().tolist())
    assert count(_alloy("fcc", 3.6, (2, 2, 2), ("A", "B", "C"), (1 / 3,) * 3, 0)) == {"A": 10, "B": 10, "C": 12}  # floor, the last takes the rest
    assert count(_alloy("bcc", 2.87, (3, 3, 3), ("A", "B"), (0.25, 0.75), 0)) == {"A": 13, "B": 41}
    assert count(_alloy("fcc", 3.6, (1, 1, 1), ("A", "B", "C"), (0.01, 0.49, 0.5), 0)) == {"A": 1, "B": 1, "C": 2}  # at least one of each
    with pytest.raises(AssertionError, match="sum to 1"):
        _alloy("fcc", 3.6, (1, 1, 1), ("A", "B"), (0.5, 0.6), 0)
    with pytest.raises(AssertionError, match="unique"):
        _alloy("fcc", 3.6, (1, 1, 1), ("A", "A"), (0.5, 0.5), 0)


def test_build_hea_through_build_crystal(oracle_backend):
    alloy = mp.build_hea(("Al", "Cr", "Ni"), (1 / 3,) * 3, "fcc", 3.6, nx=3, ny=3, nz=3, random_seed=1)
    same = _alloy("fcc", 3.6, (3, 3, 3), ("Al", "Cr", "Ni"), (1 / 3,) * 3, 1)
    assert np.array_equal(alloy.data["element"].to_numpy(), same.data["element"].to_numpy())
    assert np.array_equal(alloy.data["x"].to_numpy(), same.data["x"].to_numpy())
    with pytest.raises(ValueError, match="standard orientation"):
        mp.build_hea(("A", "B"), (0.5, 0.5), "fcc", 3.6, miller1=(1, 1, 0))


# ---- the class
def test_class_preserves_cell_positions_and_composition(restated):
    alloy = _alloy("bcc", 2.87, (3, 3, 3), ("A", "B", "C"), (1 / 3,) * 3, 42)
    sqs = mp.SQS(alloy, cutoffs={2: 3.5}, n_replicas=2, max_steps=1500, T=0.05, seed=0)
    assert sqs.system is None and sqs.objective is None and sqs.correlations is None and sqs.channel_info is None
    assert sqs.compute() is sqs
    assert sqs.system.N == alloy.N and np.array_equal(sqs.system.box.box, alloy.box.box)
    for col in ("x", "y", "z"):
        assert np.array_equal(sqs.system.data[col].to_numpy(), alloy.data[col].to_numpy())
    before, after = alloy.data["element"].to_numpy(), sqs.system.data["element"].to_numpy()
    assert Counter(before.tolist()) == Counter(after.tolist()) and not np.array_equal(before, after)
    assert np.array_equal(sqs.system.data["type"].to_numpy(), np.array([" ABC".index(e) for e in after]))
    assert isinstance(sqs.objective, float) and sqs.correlations.shape == (len(sqs.channel_info),) == (6,)
    assert sqs.replica_objectives.shape == (2,) and sqs.replica_objectives.dtype == np.float64 and sqs.objective == sqs.replica_objectives.min()
    assert set(sqs.channel_info[0]) == {"n_pts", "shell", "diameter", "funcs", "n_instances", "target", "corr"}
    assert [c["corr"] for c in sqs.channel_info] == sqs.correlations.tolist()
    # a type column alone serves as well; max_steps <= 0 evaluates the input as it stands
    typed = mp.System(data=sqs.system.data.drop("element"), box=alloy.box)
    again = mp.SQS(typed, cutoffs={2: 3.5}, max_steps=0).compute()
    assert np.array_equal(again.correlations, sqs.correlations) and again.objective == sqs.objective
    assert np.array_equal(again.system.data["type"].to_numpy(), sqs.system.data["type"].to_numpy())


def test_class_drives_correlations_down(restated):
    alloy = _alloy("fcc", 3.55, (3, 3, 3), ("Fe", "Ni", "Co", "Mn", "Cr"), (0.2,) * 5, 1)
    init = float(np.abs(mp.SQS(alloy, cutoffs={2: 2.7}, n_replicas=1, max_steps=0).compute().correlations).mean())
    sqs = mp.SQS(alloy, cutoffs={2: 2.7}, n_replicas=2, max_steps=5000, T=0.02, seed=2).compute()
    after = float(np.abs(sqs.correlations).mean())
    print(f"108 atoms, five elements: mean |corr| {init:.4f} -> {after:.4f}")
    assert after < 0.75 * init
    assert Counter(sqs.system.data["element"].to_numpy().tolist()) == Counter(alloy.data["element"].to_numpy().tolist())


def test_is_sqs_false_on_the_unoptimised_alloy(restated, oracle_backend, capsys):
    alloy = _alloy("fcc", 3.55, (2, 2, 2), ("Fe", "Ni", "Co", "Mn", "Cr"), (0.2,) * 5, 1)
    sqs = mp.SQS(alloy, cutoffs={2: 4.0}, max_steps=0, n_replicas=1)
    with pytest.raises(RuntimeError, match="compute"):
        sqs.is_sqs()
    verdict, info = sqs.compute().is_sqs(tol=0.02, verbose=False)
    assert verdict is False and capsys.readouterr().out == ""
    assert set(info) == {"verdict", "absolute", "warren_cowley"} and info["verdict"] is False
    assert set(info["absolute"]) == {"pass", "max_delta", "tol"} and info["absolute"]["tol"] == 0.02
    assert info["absolute"]["max_delta"] == max(abs(c["corr"] - c["target"]) for c in sqs.channel_info) >= 0.02
    shells = info["warren_cowley"]["per_shell"]
    assert info["warren_cowley"]["tol"] == 0.02 and [s["shell"] for s in shells] == ["NN1", "NN2"]
    for s in shells:
        assert set(s) == {"shell", "diameter", "rc", "max_abs", "max_off_diag", "matrix"}
        assert s["rc"] == s["diameter"] + 0.05 and s["matrix"].shape == (5, 5) and s["max_abs"] >= s["max_off_diag"] > 0
    sqs.is_sqs(tol=0.02)
    out = capsys.readouterr().out
    assert out.startswith("SQS verification (32 atoms; species: Co(6), Cr(8), Fe(6), Mn(6), Ni(6))")
    assert "correlations    : 20 channels  (pair=20)" in out and "FAIL    <- decides verdict" in out and out.rstrip().endswith("Verdict: NOT YET")


def test_class_refuses_other_cutoffs():
    alloy = _alloy("fcc", 3.6, (1, 1, 1), ("A", "B"), (0.5, 0.5), 0)
    with pytest.raises(ValueError, match="must include key 2"):
        mp.SQS(alloy, cutoffs={3: 3.0})
    with pytest.raises(ValueError, match=r"only 2-, 3- and 4-body cutoffs are supported \(got 5\)"):
        mp.SQS(alloy, cutoffs={2: 3.0, 5: 3.0})
    with pytest.raises(ValueError, match="element"):
        mp.SQS(mp.System(pos=np.zeros((2, 3)), box=np.eye(3)), cutoffs={2: 3.0}).compute()


# ---- the real shim and the C ABI
def test_shim_and_library_check_arguments_before_any_device_work(enumerated):
    from mdapy_amd import _lib, kernels

    assert kernels.sqs.__name__ == "mdapy_amd._sqs" and "sqs" not in kernels.NAMES
    e = _sqs.SQSEngine()
    with pytest.raises(ValueError, match="n_species must be >= 2"):
        e.set_species(1, [1.0])
    with pytest.raises(ValueError, match="n_species must be <= 8"):
        e.set_species(9, [1 / 9] * 9)
    with pytest.raises(RuntimeError, match="set_species"):
        e.add_cluster_body(2, [0, 1], [0])
    e.set_species(2, [0.5, 0.5])
    with pytest.raises(ValueError, match="n_pts must be 2..4"):
        e.add_cluster_body(5, [0, 1, 2, 3, 4], [0])
    with pytest.raises(ValueError, match="size mismatch"):
        e.add_cluster_body(2, [0, 1, 2], [0])
    e.add_cluster_body(2, [0, 1, 1, 0], [0, 0])
    with pytest.raises(RuntimeError, match="n_atoms"):
        e.finalize()
    e.n_atoms = 5000
    with pytest.raises(RuntimeError, match="shell_diameter"):
        e.finalize()
    e.shell_diameter, e.shell_weight = [1.0], [1.0]
    with pytest.raises(ValueError, match="4096"):
        e.finalize()
    e.n_atoms = 2
    with pytest.raises(RuntimeError, match="finalize"):
        e.objective([0, 1])
    e.finalize()

    pos, _, types, m, _ = ref.case("thin")
    engine = ref.build_engine(_sqs.SQSEngine, enumerated["thin"], len(pos), types, m)
    with pytest.raises(ValueError, match="n_atoms"):
        engine.objective(types[:-1])
    with pytest.raises(ValueError, match="species"):
        engine.objective(np.full(len(pos), m))
    with pytest.raises(RuntimeError, match="init_types"):
        engine.run_mc(types[:-1].tolist(), 10, 0.05, 2, 0)
    for bad in (dict(T=0.0), dict(T=-1.0), dict(T=float("nan")), dict(n_replicas=0), dict(max_steps=-1), dict(launch_steps=-1)):
        args = dict(init_types=types.tolist(), max_steps=10, T=0.05, n_replicas=2, seed=0)
        args.update(bad)
        with pytest.raises(ValueError):
            engine.run_mc(**args)

    # the C ABI itself: MDH_ERR_ARG, whatever the machine
    L = _lib.lib()
    keep, ptrs = engine._tables()
    t = np.ascontiguousarray(types, np.int32)
    out = np.zeros(1)
    count = lambda p, space=_lib.HOST: L.mdh_sqs_count(*p, t.ctypes.data, 1, None, None, None, out.ctypes.data, space, None)
    assert count(ptrs, _lib.DEVICE) == _lib.ERR_ARG and b"host memory" in L.mdh_last_error()
    assert count([None] + ptrs[1:]) == _lib.ERR_ARG
    for slot, value, said in ((0, 5000, b"4096"), (1, 9, b"species"), (1, 1, b"species")):
        dims = keep[0].copy()
        dims[slot] = value
        assert count([dims.ctypes.data] + ptrs[1:]) == _lib.ERR_ARG and said in L.mdh_last_error()
    atoms = keep[1].copy()
    atoms[3, 1] = len(pos)  # an instance that names an atom past the end never reaches a kernel
    assert count(ptrs[:1] + [atoms.ctypes.data] + ptrs[2:]) == _lib.ERR_ARG and b"out of range" in L.mdh_last_error()
    lists = keep[4].copy()
    lists[0] = int(keep[0][2])
    assert count(ptrs[:4] + [lists.ctypes.data] + ptrs[5:]) == _lib.ERR_ARG
    wide = t.copy()
    wide[0] = m
    assert L.mdh_sqs_count(*ptrs, wide.ctypes.data, 1, None, None, None, out.ctypes.data, _lib.HOST, None) == _lib.ERR_ARG
    res = [np.zeros(1, np.int32), np.zeros(len(pos), np.int32), np.zeros(engine.num_channels()), np.zeros(2)]
    run = lambda steps, T, R, cut: L.mdh_sqs_run(*ptrs, t.ctypes.data, steps, T, R, 0, cut, *[a.ctypes.data for a in res], None, _lib.HOST, None)
    assert run(10, 0.0, 2, 0) == _lib.ERR_ARG and b"T > 0" in L.mdh_last_error()
    assert run(10, 0.05, 0, 0) == _lib.ERR_ARG and run(-1, 0.05, 2, 0) == _lib.ERR_ARG and run(10, 0.05, 2, -1) == _lib.ERR_ARG
    if _lib.device_count() > 0:
        return  # (with a device the valid calls compute: test_gpu_sqs.py)
    with pytest.raises(RuntimeError, match="HIP error"):
        engine.objective(types)
    with pytest.raises(RuntimeError, match="HIP error"):
        engine.run_mc(types.tolist(), 10, 0.05, 2, 0)
    with pytest.raises(RuntimeError, match="HIP error"):
        mp.SQS(_alloy("fcc", 3.6, (2, 2, 2), ("A", "B"), (0.5, 0.5), 0), cutoffs={2: 3.0}, max_steps=10).compute()
