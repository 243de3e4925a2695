"""GPU suite: fixed-seed slices of the randomised sweeps for the consumers the oracle does not have — bond / angular
distribution, CHILL+, atomic strain, Wigner-Seitz — against the numpy restatements of tests/_bond_ref.py, _chill_ref.py,
_strain_ref.py and _ws_ref.py: at the C ABI on altered lists (tests/fuzz_parity.py: ``consumer_checks``), and through System in
random call sequences (tests/fuzz_system.py: ``plan(s, extended=True)``) on the systems of ``draw`` and of ``draw_water``, as
they are and on the cell-sorted twin.  Every test also asserts that its slice was not vacuous (tests/_fuzz_slices.py)."""
import os
import sys

import pytest

pytestmark = pytest.mark.gpu
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import _fuzz_slices as S  # noqa: E402


@pytest.fixture(autouse=True)
def _need_gpu():
    from mdapy_amd import _lib

    if _lib.device_count() < 1:
        pytest.fail("test_gpu_fuzz_consumers needs a HIP device")


def test_c_abi_consumers_fixed_seeds(monkeypatch):
    fails, stats = S.c_abi_sweep(monkeypatch)
    assert not fails, fails
    S.c_abi_not_vacuous(stats)


@pytest.mark.parametrize("water", [False, True], ids=["draw", "water"])
def test_extended_system_sweep_fixed_seeds(water, monkeypatch):
    fails, ran, stats = S.system_sweep(S.SYSTEM["water" if water else "draw"], water, monkeypatch)
    assert not fails, fails
    assert ran > 100
    S.not_vacuous(stats, water)


@pytest.mark.parametrize("water", [False, True], ids=["draw", "water"])
def test_extended_system_sweep_on_the_cell_sorted_twin(water, monkeypatch):
    fails, ran, stats = S.system_sweep(S.TWIN["water" if water else "draw"], water, monkeypatch, twin=True)
    assert not fails, fails
    assert ran > 100
    S.not_vacuous(stats, water, twin=True)
