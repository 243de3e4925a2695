"""SQS on the GPU: the raw ``_sqs.SQSEngine`` and the ``SQS`` class against the numpy restatement of tests/_sqs_ref.py.

Everything is compared with ``np.array_equal``: histograms are integers, and correlations, objectives and the chains' decisions
are formed from them in the order pinned in the header of csrc/sqs.hip, which the restatement follows.  The one place where bits
may differ is ``exp`` in the Metropolis test; a step where that could matter is *knife-edge* (_sqs_ref.chain), the seeds used here
have none, and that is asserted.  With seed 11 the restatement's counters over 5 replicas x 3000 steps are (skipped / downhill /
uphill / rejected / knife-edge):

    atat    T=0.0005  2983 / 1650 / 1641 / 8726 / 0      T=0.02  3024 / 5794 / 5839 /  343 / 0
    thin              5009 /   88 /    8 / 9895 / 0              5120 / 4285 / 4137 / 1458 / 0
    fcc222            3029 / 1339 / 1321 / 9311 / 0              3017 / 5837 / 5770 /  376 / 0
    bcc333            9519 /  604 /  130 / 4747 / 0              9451 / 2140 / 1729 / 1680 / 0
    fcc444            4949 /  460 /  404 / 9187 / 0              4956 / 4307 / 4276 / 1461 / 0

The multiset form is held against the reference's per-instance arithmetic within ``4 (n_inst + n!) 2^-53`` per channel: a channel
is a sum of n_inst terms of magnitude <= 1, each the rounded mean of at most n! rounded products."""
import functools
import math
from collections import Counter

import numpy as np
import pytest

import _sqs_ref as ref
import mdapy_amd as mp

pytestmark = pytest.mark.gpu

EPS = 2.0 ** -53
SEED, R, STEPS, TEMPERATURES = 11, 5, (0, 1, 257, 3000), (0.0005, 0.02)
NAMES = sorted(ref.CASES)


@pytest.fixture(autouse=True)
def _need_gpu():
    from mdapy_amd import _lib

    if _lib.device_count() < 1:
        pytest.fail("test_gpu_sqs needs a HIP device")


@functools.lru_cache(maxsize=None)
def _engine(name, mode=1):
    """the real engine of a named cell, filled from the package's own enumeration"""
    from mdapy_amd import _sqs
    from mdapy_amd.sqs import enumerate_clusters

    pos, box, types, m, cutoffs = ref.case(name)
    return ref.build_engine(_sqs.SQSEngine, enumerate_clusters(pos, box, cutoffs), len(pos), types, m, mode)


@functools.lru_cache(maxsize=None)
def _vectors(name):
    """70 type vectors: the cell's own, 49 shuffles of it, 20 of any composition"""
    _, _, types, m, _ = ref.case(name)
    rng = np.random.default_rng(17)
    rows = [types] + [rng.permutation(types) for _ in range(49)] + [rng.integers(0, m, len(types)) for _ in range(20)]
    rows = np.array(rows, np.int64)
    rows.setflags(write=False)
    return rows


@functools.lru_cache(maxsize=None)
def _restated_chain(name, T):
    return ref.chain(ref.restated_engine(name), ref.case(name)[2], STEPS, T, R, SEED)


# ---- 1. count
@pytest.mark.parametrize("name", NAMES)
def test_count(name):
    vectors, want = _vectors(name), ref.restated_engine(name)
    hist, corr, delta, obj = _engine(name).evaluate(vectors)
    want_hist, want_corr, want_delta, want_obj = want.evaluate(vectors)
    assert hist.dtype == np.int32 and np.array_equal(hist, want_hist), "histograms"
    assert np.array_equal(corr, want_corr), f"correlations: {int((corr != want_corr).sum())} differ"
    assert np.array_equal(delta, want_delta) and np.array_equal(obj, want_obj), "per-channel deltas and the atat objective"
    _, _, _, obj_abs = _engine(name, 0).evaluate(vectors)
    assert np.array_equal(obj_abs, ref.restated_engine(name, 0).evaluate(vectors)[3]), "the abs objective"
    assert len(set(obj.tolist())) > 3
    # the reference's own call surface, one vector at a time
    engine = _engine(name)
    first = vectors[0].tolist()
    assert engine.correlations(first) == want_corr[0].tolist() and engine.per_channel_delta(first) == want_delta[0].tolist()
    assert type(engine.objective(first)) is float and engine.objective(first) == want_obj[0]
    # against the reference's arithmetic
    bound = np.array([4.0 * (c[3] + math.factorial(c[0])) * EPS for c in want.channels])
    for k in (0, 1, 50, 69):
        err = np.abs(corr[k] - ref.per_instance_correlations(want, vectors[k]))
        print(f"{name}[{k}]: worst |multiset - per instance| {err.max():.2e} (allowed {bound[np.argmax(err)]:.2e})")
        assert np.all(err <= bound)


# ---- 2. chains against the restatement
@pytest.mark.parametrize("T", TEMPERATURES)
@pytest.mark.parametrize("name", NAMES)
def test_chains_equal_the_restatement(name, T):
    want = _restated_chain(name, T)
    counters = want["counters"]
    print(f"{name}, T={T}: {counters}")
    assert counters["knife_edge"] == 0, "pick another seed: exp() could decide a step of this chain either way"
    assert all(counters[k] >= 1 for k in ("skipped", "downhill", "uphill", "rejected")), "a step of every kind"
    engine, types = _engine(name), ref.case(name)[2]
    for steps in STEPS:
        best_types, best_obj, best_corr = engine.run_mc(types.tolist(), steps, T, R, SEED, return_replicas=True)
        at = want["at"][steps]
        assert np.array_equal(engine.replica_objectives, at["objectives"]), f"{steps} steps: every replica's best objective"
        assert np.array_equal(engine.replica_best_types, at["types"]), f"{steps} steps: every replica's best types"
        assert engine.winner == at["winner"] and best_types == at["types"][at["winner"]].tolist()
        assert best_obj == at["objectives"][at["winner"]] and best_corr == at["corr"].tolist()
    assert not np.array_equal(want["at"][0]["objectives"], want["at"][3000]["objectives"])


# ---- 3. many replicas, without the restatement
@pytest.mark.parametrize("name", NAMES)
def test_three_hundred_replicas(name):
    engine, types, T = _engine(name), ref.case(name)[2], 0.02
    many = 300

    def run(steps, replicas=many, cut=0):
        engine.run_mc(types.tolist(), steps, T, replicas, SEED, launch_steps=cut, return_replicas=True)
        return engine.replica_objectives.copy(), engine.replica_best_types.copy(), engine.winner

    obj, best, winner = run(2000)
    # the incremental state against a count from scratch
    assert np.array_equal(engine.evaluate(best)[3], obj), "a replica's best objective is the objective of its best types"
    composition = np.bincount(types, minlength=engine.n_species)
    assert all(np.array_equal(np.bincount(row, minlength=engine.n_species), composition) for row in best)
    assert winner == int(np.argmin(obj)) and obj[winner] == obj.min(), "np.argmin: the first of equal minima"
    few_obj, few_best, _ = run(2000, R)
    assert np.array_equal(few_obj, obj[:R]) and np.array_equal(few_best, best[:R]), "a replica does not depend on how many there are"
    again = run(2000)
    assert np.array_equal(again[0], obj) and np.array_equal(again[1], best) and again[2] == winner, "two runs, the same bits"
    longer, _, _ = run(4000)
    assert np.all(longer <= obj), "the best of 4 000 steps is no worse than the best of their first 2 000"
    for cut in (1, 7, 1000):
        cut_obj, cut_best, cut_winner = run(2000, cut=cut)
        assert np.array_equal(cut_obj, obj) and np.array_equal(cut_best, best) and cut_winner == winner, f"launches of {cut} steps"


def test_ties_go_to_the_lowest_replica():
    """54 atoms of two species: every chain finds the same best objective"""
    engine, types = _engine("bcc333"), ref.case("bcc333")[2]
    engine.run_mc(types.tolist(), 3000, 0.02, 300, SEED)
    assert (engine.replica_objectives == engine.replica_objectives.min()).sum() > 1 and engine.winner == 0


# ---- 4. the class, through System
def _count(system):
    return Counter(system.data["element"].to_numpy().tolist())


def test_class_on_the_device():
    alloy = mp.build_hea(("A", "B", "C"), (1 / 3,) * 3, "bcc", 2.87, nx=3, ny=3, nz=3, random_seed=42)
    sqs = mp.SQS(alloy, cutoffs={2: 3.5}, n_replicas=2, max_steps=20000, T=0.05, seed=0).compute()
    assert sqs.system.N == alloy.N and np.array_equal(sqs.system.box.box, alloy.box.box)
    for col in ("x", "y", "z"):
        assert np.array_equal(sqs.system.data[col].to_numpy(), alloy.data[col].to_numpy())
    assert _count(sqs.system) == _count(alloy) and sqs.replica_objectives.shape == (2,) and sqs.objective == sqs.replica_objectives.min()
    assert [c["corr"] for c in sqs.channel_info] == sqs.correlations.tolist()
    as_it_stands = mp.SQS(sqs.system, cutoffs={2: 3.5}, max_steps=0).compute()
    assert as_it_stands.objective == sqs.objective and np.array_equal(as_it_stands.correlations, sqs.correlations)
    assert np.array_equal(as_it_stands.system.data["element"].to_numpy(), sqs.system.data["element"].to_numpy())


def test_class_drives_correlations_down():
    alloy = mp.build_hea(("Fe", "Ni", "Co", "Mn", "Cr"), (0.2,) * 5, "fcc", 3.55, nx=3, ny=3, nz=3, random_seed=1)
    init = float(np.abs(mp.SQS(alloy, cutoffs={2: 2.7}, n_replicas=1, max_steps=0).compute().correlations).mean())
    sqs = mp.SQS(alloy, cutoffs={2: 2.7}, n_replicas=64, max_steps=20000, T=0.02, seed=2).compute()
    after = float(np.abs(sqs.correlations).mean())
    print(f"108 atoms, five elements, 64 chains of 20 000 steps: mean |corr| {init:.4f} -> {after:.4f}, objective {sqs.objective:.5f}")
    assert after < 0.75 * init and sqs.objective < 0.0
    assert _count(sqs.system) == _count(alloy)


def test_is_sqs_false_on_the_unoptimised_alloy():
    alloy = mp.build_hea(("Fe", "Ni", "Co", "Mn", "Cr"), (0.2,) * 5, "fcc", 3.55, nx=2, ny=2, nz=2, random_seed=1)
    sqs = mp.SQS(alloy, cutoffs={2: 4.0}, max_steps=0, n_replicas=1).compute()
    verdict, info = sqs.is_sqs(tol=0.02, verbose=False)
    assert verdict is False and info["absolute"]["pass"] is False and info["absolute"]["max_delta"] >= 0.02
    assert [s["shell"] for s in info["warren_cowley"]["per_shell"]] == ["NN1", "NN2"]
    assert all(s["matrix"].shape == (5, 5) for s in info["warren_cowley"]["per_shell"])


CONVERGED_STEPS = 20000  # per chain, 256 chains


def test_is_sqs_true_on_converged_cubic():
    alloy = mp.build_hea(("A", "B", "C"), (1 / 3,) * 3, "fcc", 3.6, nx=4, ny=4, nz=4, random_seed=0)
    sqs = mp.SQS(alloy, cutoffs={2: 4.0, 3: 3.0, 4: 3.0}, n_replicas=256, max_steps=CONVERGED_STEPS, T=0.02, seed=1).compute()
    verdict, info = sqs.is_sqs(tol=0.05, verbose=False)
    print(f"256 atoms, 256 chains of {CONVERGED_STEPS} steps: objective {sqs.objective:.5f}, max |pi - target| {info['absolute']['max_delta']:.4f}")
    assert verdict, f"expected SQS verdict True; info={info}"
    assert info["absolute"]["pass"]
    assert len(info["warren_cowley"]["per_shell"]) >= 1 and info["warren_cowley"]["per_shell"][0]["shell"] == "NN1"
    assert sqs.replica_objectives.shape == (256,) and sqs.objective == sqs.replica_objectives.min()
