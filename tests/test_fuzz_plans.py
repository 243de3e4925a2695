"""The randomised System sweep (tests/fuzz_system.py) without a GPU: that ``plan`` still gives the sequences the pinned ranges of
tests/test_gpu_fuzz.py have always run, and the extended plans of tests/test_gpu_fuzz_consumers.py — the same seeds — with the
oracle backend and the numpy restatements on BOTH sides, one of them forced onto the cell-sorted twin.  That proves that the
plans execute, that the policy layer gives the twin's answers in the system's numbering, and — the figures being the
yardsticks' — that the GPU slices are not vacuous and stay inside the ambiguous share of CHILL+."""
import json
import os

import pytest

import _fuzz_slices as S

HERE = os.path.dirname(os.path.abspath(__file__))


@pytest.mark.parametrize("voronoi", ["with_voronoi_reference", "without_voronoi_reference"])
def test_default_plan_gives_the_recorded_sequences(voronoi, monkeypatch):
    """tests/golden/fuzz/plan_labels.json: the labels ``plan(draw(seed))`` gave for seeds 32000-32039 and 33000-33039 before the
    extended entries existed (the Voronoi entries depend on whether the reference library was built: both recorded)"""
    import fuzz_system as F

    with open(os.path.join(HERE, "golden", "fuzz", "plan_labels.json")) as f:
        recorded = json.load(f)[voronoi]
    monkeypatch.setattr(F.O, "have_voro_ref", lambda: voronoi == "with_voronoi_reference")
    assert sorted(recorded) == [str(seed) for seed in list(range(32000, 32040)) + list(range(33000, 33040))]
    for seed, labels in recorded.items():
        assert [label for label, _ in F.plan(F.draw(int(seed)))] == labels, seed
        extended = [label for label, _ in F.plan(F.draw(int(seed)), extended=True)]
        assert len(extended) >= 4 and set(extended) <= set(labels) | set(S.NEW) | {lab for seq in recorded.values() for lab in seq}


@pytest.mark.parametrize("twin", [False, True], ids=["plain", "twin"])
@pytest.mark.parametrize("water", [False, True], ids=["draw", "water"])
def test_extended_plans_on_the_host(water, twin, monkeypatch):
    seeds = (S.TWIN if twin else S.SYSTEM)["water" if water else "draw"]
    fails, ran, stats = S.system_sweep(seeds, water, monkeypatch, twin=twin, host_only=True)
    assert not fails, fails
    assert ran > 100
    S.not_vacuous(stats, water, twin)
