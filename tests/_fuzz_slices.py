"""The fixed-seed slices of the extended sweeps (tests/fuzz_system.py with ``extended=True``, the consumer entries of
tests/fuzz_parity.py) that tests/test_gpu_fuzz_consumers.py runs against the HIP library and tests/test_fuzz_plans.py runs on
the host, and what both assert about them: no failures, and that the slice was not vacuous — judged on the yardsticks' side
(the figures fuzz_parity.STATS collects), so the host run proves it for the GPU run.  TEST INFRASTRUCTURE."""
import _chill_ref
import fuzz_parity as FP

# fresh seeds: none of them is in a range tests/test_gpu_fuzz.py pins
C_ABI = dict(draw=range(41000, 41040), water=range(41500, 41520))
# (a run of consecutive seeds, and a few small systems picked from 46000 ... and 47000 ... for what a short run may miss: a thin
# box whose plan holds the strain entry — the replica — the ADF tables of more than 32 patterns or more than 8192 bins,
# an entry that ran fewer than MIN_RUNS times)
SYSTEM = dict(draw=list(range(42010, 42030)) + [46010, 46018, 46026, 46050, 46086, 46092, 46146],
              water=list(range(43000, 43026)) + [47013, 47017, 47020, 47050, 47051])
TWIN = dict(draw=list(range(44300, 44320)) + [46020, 46037, 46042, 46055, 46071, 46092], water=list(range(45000, 45026)) + [47117, 47125])
NEW = ("bond", "adf", "chill", "strain", "ws")
MIN_RUNS = 3  # of every new entry, in every System slice
C_ABI_MIN_RUNS = 40  # and in the C-ABI slice (60 systems; CHILL+ skips the unrattled metal crystals among them)


def system_sweep(seeds, water, monkeypatch, twin=False, host_only=False):
    """-> (failures, calls that agreed, the yardsticks' figures)"""
    import fuzz_system as F

    if twin:
        monkeypatch.setenv("FUZZ_TWIN", "1")
    else:
        monkeypatch.delenv("FUZZ_TWIN", raising=False)
    monkeypatch.setattr(FP, "STATS", {})
    fails, ran = [], 0
    for seed in seeds:
        ran += F.run_seed(seed, fails, extended=True, water=water, host_only=host_only)
    return fails, ran, dict(FP.STATS)


def c_abi_sweep(monkeypatch):
    monkeypatch.setattr(FP, "STATS", {})
    fails = []
    for seeds, draw in ((C_ABI["draw"], FP.draw), (C_ABI["water"], FP.draw_water)):
        for seed in seeds:
            for name, fn in FP.consumer_checks(draw(seed)):
                FP._note("ran " + name)
                try:
                    fn()
                except Exception as e:  # noqa: BLE001 - every kind of failure is a finding
                    fails.append((seed, name, type(e).__name__, str(e)[:200]))
    return fails, dict(FP.STATS)


def chill_share(stats):
    """over a whole slice at most MAX_AMBIGUOUS of all atoms sit on a threshold (per system: fuzz_parity.chill_rule)"""
    assert stats.get("chill atoms", 0) > 0
    assert stats["chill ambiguous"] <= _chill_ref.MAX_AMBIGUOUS * stats["chill atoms"], stats


def chill_classes(stats):
    """CHILL+ had something to classify: at least four of its six classes, labels other than 0 among them"""
    seen = [code for code in range(6) if stats.get(f"chill class {code}", 0) > 0]
    assert len(seen) >= 4 and any(code > 0 for code in seen), stats


def adf_kinds(stats, kinds=("same", "mixed", "lower", "many", "wide")):
    """every kind of pattern set counted something at least once"""
    empty = [kind for kind in kinds if stats.get("adf nonempty " + kind, 0) < 1]
    assert not empty, (empty, stats)


def not_vacuous(stats, water, twin=False):
    print(stats)
    short = [name for name in NEW if stats.get("ran " + name, 0) < MIN_RUNS]
    assert not short, (short, stats)
    chill_share(stats)
    if water:  # (the metals and gases of ``draw`` have next to no four-coordinated site: there the entry is swept, not judged)
        chill_classes(stats)
    adf_kinds(stats)
    assert stats.get("bond lengths", 0) > 0
    assert stats.get("ws vacancies", 0) > 0 and stats.get("ws interstitials", 0) > 0, stats
    assert stats.get("strain affine", 0) > 0 and stats.get("strain plain", 0) > 0 and stats.get("strain replica", 0) > 0, stats
    if twin:
        unused = [name for name in ("bond", "chill", "strain") if stats.get("twin " + name, 0) < 1]
        assert not unused, (unused, stats)


def c_abi_not_vacuous(stats):
    print(stats)
    short = [name for name in NEW if stats.get("ran " + name, 0) < C_ABI_MIN_RUNS]
    assert not short, (short, stats)
    assert stats.get("ws ties", 0) >= 100, stats  # queries at exactly equal distance from several sites (fuzz_parity.ws_ties)
    chill_share(stats)
    chill_classes(stats)
    adf_kinds(stats)
    assert stats.get("bond lengths", 0) > 0 and stats.get("bond angles", 0) > 0 and stats.get("strain finite", 0) > 0
    assert stats.get("ws vacancies", 0) > 0 and stats.get("ws interstitials", 0) > 0
    unseen = [how for how in ("exact", "padded", "truncated", "nearest", "lowered", "beyond") if stats.get("list " + how, 0) < 1]
    assert not unseen, (unseen, stats)
