"""The Lindemann index on the GPU: the raw ``_lindemann`` shim and ``LindemannParameter`` against the numpy restatement of
tests/_lindemann_ref.py.

Pair tables are compared with ``np.array_equal``: both sides do the reference's per-pair arithmetic in IEEE binary64.  Results
are sums of identical non-negative terms taken in two orders, so they are compared within ``4 n 2^-53 want``, n the number of
terms a result can hold (N - 1 for an atom, N (N - 1) for a frame, N (N - 1) / 2 for the global value): the yardstick rounds the
exact sum once and divides (2 roundings), the device adds in a tree of far fewer than n levels and divides once; where every term
is skipped — every entry of frame 0, a row whose pairs never move — the bound is 0 and the result must be an exact 0.

What each seeded input is said to contain was checked on the CPU beforehand and is asserted here."""
import functools

import numpy as np
import pytest

import _lindemann_ref
import mdapy_amd as mp

pytestmark = pytest.mark.gpu

T = 64  # the kernels' tile edge (csrc/lindemann.hip LD_T)
EPS = 2.0 ** -53


@pytest.fixture(autouse=True)
def _need_gpu():
    from mdapy_amd import _lib

    if _lib.device_count() < 1:
        pytest.fail("test_gpu_lindemann needs a HIP device")


# ---- inputs
def walk(F, N, seed):
    """the reference's own test input: a random walk on the integer lattice; in frame 0 many atoms coincide"""
    rng = np.random.default_rng(seed)
    return np.cumsum(rng.choice([-1.0, 0.0, 1.0], size=(F, N, 3)), axis=0)


def solid(F, seed):
    """a 5 x 5 x 5 cubic lattice, spacing 2.5, rattled by N(0, 0.08) in every frame: var / mean^2 goes down to 5e-5, where the
    global mode's S2 / F - (S1 / F)^2 cancels"""
    rng = np.random.default_rng(seed)
    g = np.arange(5) * 2.5
    lattice = np.stack(np.meshgrid(g, g, g, indexing="ij"), axis=-1).reshape(-1, 3)
    return lattice[None] + rng.normal(0.0, 0.08, (F, len(lattice), 3))


RIGID = 12


def rigid(F=11, N=70, seed=0):
    """a walk whose atoms 0 .. 11 are a rigid body (N(0, 3) coordinates) shifted by an integer vector per frame — their distances
    change by rounding alone, so var and delta are zero or a few ulps either side of it — and whose atom 13 lies on atom 12 in
    every frame"""
    rng = np.random.default_rng(seed)
    pos = np.cumsum(rng.choice([-1.0, 0.0, 1.0], size=(F, N, 3)), axis=0)
    body = rng.normal(0.0, 3.0, (RIGID, 3))
    shift = rng.integers(-8, 9, (F, 3)).astype(np.float64)
    pos[:, :RIGID] = body[None] + shift[:, None]
    pos[:, 13] = pos[:, 12]
    return pos


CASES = {
    "rigid0": lambda: rigid(seed=0),
    "rigid1": lambda: rigid(seed=1),
    "rigid2": lambda: rigid(seed=2),
    "solid": lambda: solid(9, 5),
    "walk": lambda: walk(12, 130, 7),
}


@functools.lru_cache(maxsize=None)
def _case(name):
    """(positions, restatement) of a named input, made once; both read-only"""
    pos = CASES[name]()
    pos.setflags(write=False)
    return pos, _lindemann_ref.restate(pos)


@functools.lru_cache(maxsize=None)
def _walk_case(F, N):
    pos = walk(F, N, 100 * F + N)
    pos.setflags(write=False)
    return pos, _lindemann_ref.restate(pos)


# ---- the device side, through the shim
MARK = -7.25  # what the global mode's tables hold beforehand: everything outside the strict upper triangle keeps it


def _all(pos, segments=None, tables=True):
    from mdapy_amd import kernels

    F, N = pos.shape[:2]
    mean = np.full((N, N), np.nan) if tables else None
    var = np.full((N, N), np.nan) if tables else None
    frame, atom = np.full(F, np.nan), np.full((F, N), np.nan)
    kernels.lindemann.compute_all(pos, mean, var, frame, atom, segments=segments)
    return frame, atom, mean, var


def _global(pos, tables=True):
    from mdapy_amd import kernels

    N = pos.shape[1]
    s1 = np.full((N, N), MARK) if tables else None
    s2 = np.full((N, N), MARK) if tables else None
    value = kernels.lindemann.compute_global(pos, s1, s2, 1)
    assert type(value) is float
    return value, s1, s2


def _within(got, want, n, what):
    got, want = np.asarray(got, dtype=np.float64), np.asarray(want, dtype=np.float64)
    assert got.shape == want.shape, what
    bound = 4.0 * n * EPS * want
    err = np.abs(got - want)
    worst = float(np.max(np.where(want > 0, err / np.where(want > 0, want, 1.0), 0.0))) / EPS if got.size else 0.0
    print(f"{what}: worst error {worst:.2f} x 2^-53 want (allowed {4 * n}), {int((want == 0).sum())} exact zeros wanted")
    assert np.all(err <= bound), f"{what}: {int((err > bound).sum())} entries outside 4 n 2^-53 want, worst {worst:.1f} x 2^-53"


def _check_results(pos, want, frame, atom, value):
    N = pos.shape[1]
    _within(atom, want.atom, N - 1, "lindemann_atom")
    _within(frame, want.frame, N * (N - 1), "lindemann_frame")
    _within(value, want.trj, N * (N - 1) // 2, "global value")


def _check_tables(want, mean, var, s1, s2):
    assert np.array_equal(mean, want.mean), f"pair_mean: {int((mean != want.mean).sum())} entries differ"
    assert np.array_equal(var, want.var), f"pair_var: {int((var != want.var).sum())} entries differ"
    up = want.upper
    assert np.array_equal(s1[up], want.sum[up]), f"pair_sum: {int((s1[up] != want.sum[up]).sum())} entries differ"
    assert np.array_equal(s2[up], want.sumsq[up]), f"pair_sumsq: {int((s2[up] != want.sumsq[up]).sum())} entries differ"
    assert np.all(s1[~up] == MARK) and np.all(s2[~up] == MARK), "the global mode wrote outside the strict upper triangle"


# ---- what the inputs contain
def test_inputs_hold_what_they_are_said_to():
    pos, want = _case("walk")
    assert not want.var_positive[0].any() and not want.frame[0] and not want.atom[0].any()
    first = pos[0]
    coincide = (np.abs(first[:, None] - first[None]).sum(-1) == 0).sum() - len(first)
    assert coincide > 100, "many atoms of the walk's frame 0 lie on each other"

    pos, want = _case("solid")
    assert pos.shape == (9, 125, 3)
    off = ~np.eye(125, dtype=bool)
    with np.errstate(invalid="ignore"):
        rel = (want.var / want.mean ** 2)[off]
    assert 3e-5 < rel.min() < 5e-5, "the cancellation regime of the naive sums"
    assert abs(want.trj - want.frame[-1]) <= 5e-15 * want.trj and want.delta_positive.sum() == 125 * 124 // 2

    for seed in range(3):
        pos, want = _case(f"rigid{seed}")
        assert pos.shape == (11, 70, 3)
        body = np.zeros((70, 70), dtype=bool)
        body[:RIGID, :RIGID] = True
        ordered = body & ~np.eye(70, dtype=bool)
        var = want.var[ordered]
        assert ordered.sum() == 132 and np.all(var >= 0)
        assert 48 <= (var == 0).sum() <= 54 and 78 <= (var > 0).sum() <= 84, "rigid pairs on both sides of var > 0"
        assert np.sqrt(var.max()) < 64 * EPS * want.mean[ordered].max(), "sqrt(var) of a rigid pair is a few ulps of its distance"
        pairs = body & want.upper
        delta = want.delta[pairs]
        assert pairs.sum() == 66
        assert 27 <= (delta > 0).sum() <= 30 and 9 <= (delta == 0).sum() <= 15 and 22 <= (delta < 0).sum() <= 30, "delta on both sides of 0, and on it"
        assert want.mean[12, 13] == 0 and want.var[12, 13] == 0 and want.sum[12, 13] == 0, "the coincident pair"
        assert not want.var_positive[:, 12, 13].any() and not want.delta_positive[12, 13]


# ---- the raw entry points
@pytest.mark.parametrize("name", sorted(CASES))
def test_pair_tables_are_exact(name):
    pos, want = _case(name)
    _, _, mean, var = _all(pos)
    _, s1, s2 = _global(pos)
    _check_tables(want, mean, var, s1, s2)


@pytest.mark.parametrize("name", sorted(CASES))
def test_results_within_the_derived_bound(name):
    pos, want = _case(name)
    frame, atom, _, _ = _all(pos, tables=False)
    value, _, _ = _global(pos, tables=False)
    _check_results(pos, want, frame, atom, value)
    assert not frame[0] and not atom[0].any(), "frame 0 has no term: exact zeros"


@pytest.mark.parametrize("F", [1, 2, 12])
@pytest.mark.parametrize("N", [2, T - 1, T, T + 1, 2 * T + 2, 4 * T + 1])
def test_tile_edges(N, F):
    pos, want = _walk_case(F, N)
    frame, atom, mean, var = _all(pos)
    value, s1, s2 = _global(pos)
    _check_tables(want, mean, var, s1, s2)
    _check_results(pos, want, frame, atom, value)
    if F == 1:
        assert value == 0.0 and not frame.any() and not atom.any() and not var.any(), "one frame: nothing fluctuates"


def test_segments():
    pos, want = _walk_case(12, 4 * T + 1)
    N = pos.shape[1]
    seen = {}
    for segments in (1, 2, 3, 9):  # five j blocks: 9 is clamped
        frame, atom, _, _ = _all(pos, segments=segments, tables=False)
        _within(atom, want.atom, N - 1, f"lindemann_atom, segments={segments}")
        _within(frame, want.frame, N * (N - 1), f"lindemann_frame, segments={segments}")
        again_frame, again_atom, _, _ = _all(pos, segments=segments, tables=False)
        assert np.array_equal(frame, again_frame) and np.array_equal(atom, again_atom), "two runs, the same bits"
        seen[segments] = atom
    default_frame, default_atom, _, _ = _all(pos, tables=False)
    assert np.array_equal(default_atom, seen[9]), "the library's choice at five blocks is one block per workgroup, as the clamp's"
    with pytest.raises(ValueError):
        _all(pos, segments=-1, tables=False)


# ---- the class
def test_class_level():
    from mdapy_amd.devarray import HArray

    pos, want = _case("solid")
    N = pos.shape[1]
    only = mp.LindemannParameter(pos, only_global=True)
    only.compute()
    assert only.lindemann_frame is None and only.lindemann_atom is None and type(only.lindemann_trj) is float
    _within(only.lindemann_trj, want.trj, N * (N - 1) // 2, "LindemannParameter(only_global=True)")

    full = mp.LindemannParameter(pos)
    assert full.lindemann_frame is None and full.lindemann_atom is None
    full.compute()
    assert isinstance(full.lindemann_frame, np.ndarray) and full.lindemann_frame.shape == (9,)
    assert isinstance(full.lindemann_atom, np.ndarray) and full.lindemann_atom.shape == (9, N)
    assert type(full.lindemann_trj) is float and full.lindemann_trj == full.lindemann_frame[-1]
    _within(full.lindemann_atom, want.atom, N - 1, "LindemannParameter.lindemann_atom")
    _within(full.lindemann_frame, want.frame, N * (N - 1), "LindemannParameter.lindemann_frame")
    assert np.isclose(full.lindemann_trj, only.lindemann_trj)  # the reference's own test

    resident = HArray.from_numpy(pos)
    for device_input in (resident, resident.dev()):
        dev_full = mp.LindemannParameter(device_input)
        dev_full.compute()
        assert np.array_equal(dev_full.lindemann_atom, full.lindemann_atom) and np.array_equal(dev_full.lindemann_frame, full.lindemann_frame)
        dev_only = mp.LindemannParameter(device_input, only_global=True)
        dev_only.compute()
        assert dev_only.lindemann_trj == only.lindemann_trj and dev_only.lindemann_frame is None


def test_outputs_in_hbm():
    """the shim with every array resident: the same bits as with numpy arrays"""
    from mdapy_amd import kernels
    from mdapy_amd.devarray import HArray

    pos, want = _case("rigid0")
    F, N = pos.shape[:2]
    frame, atom, mean, var = _all(pos)
    dpos = HArray.from_numpy(pos)
    dframe, datom = HArray.empty(F, np.float64), HArray.empty((F, N), np.float64)
    dmean, dvar = HArray.empty((N, N), np.float64), HArray.empty((N, N), np.float64)
    kernels.lindemann.compute_all(dpos, dmean, dvar, dframe, datom)
    assert np.array_equal(np.asarray(dframe), frame) and np.array_equal(np.asarray(datom), atom)
    assert np.array_equal(np.asarray(dmean), want.mean) and np.array_equal(np.asarray(dvar), want.var)
    s1 = HArray.full((N, N), MARK, np.float64)
    value = kernels.lindemann.compute_global(dpos, s1, None, 1)
    assert value == _global(pos, tables=False)[0]
    s1 = np.asarray(s1)
    assert np.array_equal(s1[want.upper], want.sum[want.upper]) and np.all(s1[~want.upper] == MARK)
