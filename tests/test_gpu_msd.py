"""The mean squared displacement on the GPU: the raw ``_msd`` shim and ``MeanSquaredDisplacement`` against the numpy
restatement of tests/_msd_ref.py.

Bounds, with u = 2^-53, n = F - m the number of terms of a window entry and ``want`` the restatement's value:

* window ``particle_msd``: ``|got - want| <= 2 (n + 2) u want``.  Derived, not measured: the sum has n non-negative terms with the
  restatement's bits, added in any order ((n - 1) u), it is divided once on each side, the yardstick's fsum rounds once, and the
  whole is doubled for higher-order terms.  Where ``want == 0`` (every lag-0 entry, an atom that never moves) the bound is 0.
* direct ``particle_msd``: one term, no sum: ``np.array_equal``.
* ``msd``, either mode: ``|got - fsum(want_row) / N| <= (2 (n + 2) + 2 (N + 2)) u want``, n = 1 in direct mode.
* on a lattice walk every term and partial sum is an integer below 2^53: window ``particle_msd`` is ``np.array_equal``; and the
  walk shifted by 2^30 gives the bits of the plain walk, which no float32 path and no S1 - 2 S2 formulation can."""
import functools
import math

import numpy as np
import pytest

import _msd_ref
import mdapy_amd as mp

pytestmark = pytest.mark.gpu

AB = 64  # atoms per workgroup (csrc/msd.hip MSD_AB)
LB = 32  # lags per workgroup (MSD_LB: four waves of MSD_LW = 8)
C = 8    # time origins per chunk = frames per LDS slab (MSD_C)
EPS = 2.0 ** -53

EDGE_F = (1, 2, LB - 1, LB, LB + 1, 2 * LB + 3, C + 1)
EDGE_N = (1, AB - 1, AB, AB + 1, 2 * AB + 2)
BIG = (2 * LB + 3, 2 * AB + 2)


@pytest.fixture(autouse=True)
def _need_gpu():
    from mdapy_amd import _lib

    if _lib.device_count() < 1:
        pytest.fail("test_gpu_msd needs a HIP device")


# ---- inputs
def walk(F, N):
    """a random walk on the integer lattice"""
    rng = np.random.default_rng(1000 * F + N)
    return np.cumsum(rng.choice([-1.0, 0.0, 1.0], size=(F, N, 3)), axis=0)


def real(F, N):
    """N(0, 2) starting points plus a cumulative N(0, 0.3) walk; atom 0 stands still in every frame"""
    rng = np.random.default_rng(7000 * F + N)
    pos = rng.normal(0.0, 2.0, (1, N, 3)) + np.cumsum(rng.normal(0.0, 0.3, (F, N, 3)), axis=0)
    pos[:, 0] = pos[0, 0]
    return pos


@functools.lru_cache(maxsize=None)
def _case(kind, F, N):
    """(positions, restatement) of a named input, made once; both read-only"""
    pos = {"walk": walk, "real": real, "offset": lambda F, N: walk(F, N) + 2.0 ** 30}[kind](F, N)
    pos.setflags(write=False)
    return pos, _msd_ref.restate(pos)


# ---- the device side, through the shim; outputs start as NaN
def _run(mode, pos, lags=None, table=True, mean=True):
    from mdapy_amd import kernels

    F, N = pos.shape[:2]
    rows = F if lags is None else lags
    particle = np.full((rows, N), np.nan) if table else None
    msd = np.full(rows, np.nan) if mean else None
    getattr(kernels.msd, mode)(pos, particle, msd)
    return particle, msd


def _terms(mode, F, rows):
    return (F - np.arange(rows)).astype(np.float64) if mode == "window" else np.ones(rows)


def _check(mode, pos, want_table, particle, msd, what):
    """the bounds of the module docstring; prints each figure before it asserts"""
    F, N = pos.shape[:2]
    rows = want_table.shape[0]
    n = _terms(mode, F, rows)
    assert particle.shape == (rows, N) and msd.shape == (rows,)
    assert not np.isnan(particle).any() and not np.isnan(msd).any(), f"{what}: an output entry was not written"
    err = np.abs(particle - want_table)
    if mode == "direct":
        print(f"{what}: direct particle_msd, {int((particle != want_table).sum())} entries differ")
        assert np.array_equal(particle, want_table)
    else:
        bound = 2.0 * (n[:, None] + 2.0) * EPS * want_table
        rel = np.where(want_table > 0, err / np.where(want_table > 0, want_table, 1.0), 0.0) / ((n[:, None] + 2.0) * EPS)
        print(f"{what}: window particle_msd, worst error {float(rel.max()):.3f} x (n + 2) 2^-53 want (allowed 2), "
              f"{int((want_table == 0).sum())} exact zeros wanted")
        assert np.all(err <= bound), f"{what}: {int((err > bound).sum())} entries outside 2 (n + 2) 2^-53 want"
    assert np.all(particle[want_table == 0] == 0), f"{what}: an entry that must be an exact 0 is not"
    want_msd = np.array([math.fsum(row) / float(N) for row in want_table])
    allowed = (2.0 * (n + 2.0) + 2.0 * (N + 2.0)) * EPS * want_msd
    off = np.abs(msd - want_msd)
    worst = float(np.max(np.where(want_msd > 0, off / np.where(want_msd > 0, want_msd, 1.0), 0.0))) / EPS
    print(f"{what}: msd, worst error {worst:.2f} x 2^-53 want (allowed from {float(np.min(2 * (n + 2) + 2 * (N + 2))):.0f})")
    assert np.all(off <= allowed), f"{what}: msd outside (2 (n + 2) + 2 (N + 2)) 2^-53 want"


# ---- what the inputs contain (no device work)
def test_inputs_hold_what_they_are_said_to():
    F, N = BIG
    plain, want = _case("walk", F, N)
    shifted, want_shifted = _case("offset", F, N)
    assert np.array_equal(shifted - 2.0 ** 30, plain) and np.array_equal(want_shifted.window, want.window)
    # rounded to float32 the shifted walk loses its steps: what a single-precision path would compute
    single = _msd_ref.restate(shifted.astype(np.float32).astype(np.float64))
    assert not np.array_equal(single.window, want.window) and not np.array_equal(single.direct, want.direct)
    assert np.abs(single.window_msd - want.window_msd).max() > 1.0
    pos, want = _case("real", F, N)
    assert not want.window[:, 0].any() and not want.direct[:, 0].any() and np.all(want.window[1:, 1:] > 0)
    assert not want.window[0].any() and want.window_msd[0] == 0


# ---- the raw entry points
@pytest.mark.parametrize("N", EDGE_N)
@pytest.mark.parametrize("F", EDGE_F)
def test_tile_edges(F, N):
    pos, want = _case("walk", F, N)
    for mode, table in (("window", want.window), ("direct", want.direct)):
        particle, msd = _run(mode, pos)
        _check(mode, pos, table, particle, msd, f"walk({F}, {N}) {mode}")
        assert np.array_equal(particle, table), f"{mode}: a lattice walk is exact"
        if F == 1:
            assert not particle.any() and not msd.any(), "one frame: nothing moves"
    assert np.array_equal(_run("window", pos)[0][-1], _run("direct", pos)[0][-1]), "the last lag is the one term of direct mode"


@pytest.mark.parametrize("kind", ["real", "offset"])
def test_within_the_derived_bounds(kind):
    F, N = BIG
    pos, want = _case(kind, F, N)
    for mode, table in (("window", want.window), ("direct", want.direct)):
        particle, msd = _run(mode, pos)
        _check(mode, pos, table, particle, msd, f"{kind}({F}, {N}) {mode}")


def test_a_shift_by_2_to_the_30_changes_no_bit():
    F, N = BIG
    plain, want = _case("walk", F, N)
    shifted, _ = _case("offset", F, N)
    for mode, table in (("window", want.window), ("direct", want.direct)):
        particle, msd = _run(mode, plain)
        moved_particle, moved_msd = _run(mode, shifted)
        assert np.array_equal(particle, table)
        assert np.array_equal(moved_particle, particle) and np.array_equal(moved_msd, msd), mode


@pytest.mark.parametrize("lags", [1, LB, LB + 1])
def test_truncated_lags(lags):
    F, N = BIG
    pos, want = _case("real", F, N)
    full_particle, full_msd = _run("window", pos)
    particle, msd = _run("window", pos, lags=lags)
    assert np.array_equal(particle, full_particle[:lags]) and np.array_equal(msd, full_msd[:lags])
    _check("window", pos, want.window[:lags], particle, msd, f"real, {lags} lags")


@pytest.mark.parametrize("mode", ["window", "direct"])
def test_either_output_alone_and_twice_the_same_bits(mode):
    F, N = BIG
    pos, _ = _case("real", F, N)
    particle, msd = _run(mode, pos)
    again_particle, again_msd = _run(mode, pos)
    assert np.array_equal(particle, again_particle) and np.array_equal(msd, again_msd), "two runs, the same bits"
    none, only_msd = _run(mode, pos, table=False)
    only_particle, nothing = _run(mode, pos, mean=False)
    assert none is None and nothing is None
    assert np.array_equal(only_msd, msd) and np.array_equal(only_particle, particle)
    with pytest.raises(ValueError):
        _run(mode, pos, table=False, mean=False)


# ---- the class
@pytest.mark.parametrize("mode", ["window", "direct"])
def test_class_level(mode):
    from mdapy_amd.devarray import HArray

    F, N = 2 * LB + 3, AB + 1
    pos, want = _case("real", F, N)
    table = want.window if mode == "window" else want.direct
    host = mp.MeanSquaredDisplacement(pos, mode=mode)
    assert host.particle_msd is None and host.msd is None and host.mode == mode
    assert host.compute() is None
    assert isinstance(host.particle_msd, np.ndarray) and host.particle_msd.dtype == np.float64 and host.particle_msd.shape == (F, N)
    assert isinstance(host.msd, np.ndarray) and host.msd.dtype == np.float64 and host.msd.shape == (F,)
    _check(mode, pos, table, host.particle_msd, host.msd, f"MeanSquaredDisplacement({mode})")
    assert host.msd[0] == 0
    resident = HArray.from_numpy(np.array(pos))
    for device_input in (resident, resident.dev()):
        dev = mp.MeanSquaredDisplacement(device_input, mode=mode)
        assert dev.pos_list is device_input
        dev.compute()
        assert isinstance(dev.particle_msd, np.ndarray) and isinstance(dev.msd, np.ndarray)
        assert np.array_equal(dev.particle_msd, host.particle_msd) and np.array_equal(dev.msd, host.msd)
