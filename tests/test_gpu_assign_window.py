"""-m gpu: the cell binning after k_assign groups atoms of one cell up to three lanes apart (assign_groups.hpp), writes (cell, slot)
as one entry, and the tile kernel leaves its slice pass out when the last build of the same (N, grid) listed nothing.  Rows,
counts and distances of build_neighbor are bitwise the oracle's build_neighbor, the labels of mdh_build_neighbor_fcna the oracle's
fcna, on inputs that reach every branch of the grouping and of the mop-up."""
import ctypes

import numpy as np
import pytest

from mdapy_amd import _lib, _neighbor
from mdapy_amd.build_lattice import lattice_positions
from oracle import oracle as O

pytestmark = pytest.mark.gpu

PBC = np.array([1, 1, 1], np.int32)
ORG0 = np.zeros(3)
A_CU = 3.615
RC = 0.854 * A_CU
M = 16


def _xyz(pos):
    return tuple(np.ascontiguousarray(pos[:, k]) for k in range(3))


def _oracle(pos, box, key=None):
    """rows (caller's pads, M slots, counts running past M), distances, counts and fixed-cutoff labels of the oracle.  Atoms with
    x = NaN are absent: left out of the search, in nobody's row (their own rows are not defined: `ok` says which count).  key: the
    atoms of a cell in descending key instead of descending id — the oracle on the atoms renumbered by rising key, ids mapped back."""
    ok = np.isfinite(pos[:, 0])
    ids = np.nonzero(ok)[0]
    if key is not None:
        ids = ids[np.argsort(key[ids], kind="stable")]
    sub = np.ascontiguousarray(pos[ids])
    x, y, z = _xyz(sub)
    n = len(ids)
    v = np.full((n, M), -1, np.int32); d = np.full((n, M), RC + 1.0); c = np.zeros(n, np.int32)
    O.build_neighbor(x, y, z, box, ORG0, PBC, RC, v, d, c, 4)
    p = np.zeros(n, np.int32)
    O.fcna(x, y, z, box, ORG0, PBC, v, c, p, RC, 4)
    N = len(pos)
    rows = np.full((N, M), -1, np.int32); dist = np.full((N, M), RC + 1.0)
    counts = np.zeros(N, np.int32); labels = np.zeros(N, np.int32)
    rows[ids] = np.where(v >= 0, ids[np.clip(v, 0, None)], -1)
    dist[ids], counts[ids], labels[ids] = d, c, p
    return ok, rows, dist, counts, labels


def _gpu(pos, box, key=None, window=None, fused_first=False):
    """(rows, distances, counts) of build_neighbor and (rows, distances, counts, labels) of build_neighbor_fcna"""
    x, y, z = _xyz(pos)
    n = len(x)
    v = np.empty((n, M), np.int32); d = np.empty((n, M)); c = np.empty(n, np.int32)
    vf = np.empty((n, M), np.int32); df = np.empty((n, M)); cf = np.empty(n, np.int32); pf = np.zeros(n, np.int32)

    def plain():
        if window is not None:
            _neighbor.hint_cell_window(0, *window)
        _neighbor.build_neighbor(x, y, z, box, ORG0, PBC, RC, v, d, c, 1, fill_pads=True, key=key)

    def fused():
        if window is not None:
            _neighbor.hint_cell_window(0, *window)
        _neighbor.build_neighbor_fcna(x, y, z, box, ORG0, PBC, RC, vf, df, cf, pf, 1, fill_pads=True, key=key)

    for call in ((fused, plain) if fused_first else (plain, fused)):
        call()
    return (v, d, c), (vf, df, cf, pf)


def _compare(tag, pos, box, key=None, window=None, fused_first=False):
    ok, rows, dist, counts, labels = _oracle(pos, box, key)
    plain, fused = _gpu(pos, box, key, window, fused_first)
    for name, got in (("build_neighbor", plain), ("build_neighbor_fcna", fused)):
        assert np.array_equal(got[2][ok], counts[ok]), (tag, name, "counts")
        assert np.array_equal(got[0][ok], rows[ok]), (tag, name, "rows")
        assert np.array_equal(got[1][ok], dist[ok]), (tag, name, "distances")
    assert np.array_equal(fused[3][ok], labels[ok]), (tag, "labels", int((fused[3][ok] != labels[ok]).sum()))
    return counts, labels, ok


def _tile_kernel_took_it(tag):
    plan = np.zeros(8, np.int32)
    _lib.lib().mdh_debug_neighbor_plan(plan.ctypes.data)
    assert plan[0] > 0, (tag, plan.tolist())


def _listed_at_plan_time():
    out4 = (ctypes.c_int64 * 4)()
    _lib.lib().mdh_debug_counters(out4)
    return int(out4[1])


def test_lattice_in_lattice_order():
    """the four basis atoms of a lattice cell alternate between grid cells: groups of lanes two and three apart"""
    pos, box = lattice_positions("fcc", A_CU, 20, 20, 20)
    counts, labels, _ = _compare("lattice", pos, box)
    _tile_kernel_took_it("lattice")
    assert (counts == 12).all() and (labels == 1).all()


def test_lattice_permuted_inside_blocks_of_eight():
    """atoms of one cell one to seven lanes apart, in no fixed pattern: members, stranded lanes and heads of every kind"""
    pos, box = lattice_positions("fcc", A_CU, 20, 20, 20)
    rng = np.random.default_rng(5)
    pos = pos + rng.normal(0.0, 0.03, pos.shape)
    perm = (np.arange(len(pos)).reshape(-1, 8) + 0)
    perm = np.take_along_axis(perm, np.argsort(rng.random(perm.shape), axis=1), axis=1).reshape(-1)
    assert not np.array_equal(perm, np.arange(len(pos))) and np.array_equal(np.sort(perm), np.arange(len(pos)))
    counts, labels, _ = _compare("blocks of 8", np.ascontiguousarray(pos[perm]), box)
    _tile_kernel_took_it("blocks of 8")
    assert (labels == 1).sum() > 0.9 * len(pos)


def test_more_than_a_million_atoms_four_slices_per_lane():
    """from 2^20 atoms on a lane of k_assign holds four slices of 64 atoms, their atomics in flight together; rattled, so that the
    groups differ from slice to slice"""
    pos, box = lattice_positions("fcc", A_CU, 64, 64, 65)
    assert len(pos) >= 1 << 20
    pos = pos + np.random.default_rng(6).normal(0.0, 0.05, pos.shape)
    counts, labels, _ = _compare("four slices", pos, box)
    assert (labels == 1).sum() > 0.9 * len(pos)


def test_absent_atoms():
    """x = NaN: no cell, no atomic, in nobody's row — singly, in pairs inside a group, and a whole slice of them"""
    pos, box = lattice_positions("fcc", A_CU, 16, 16, 16)
    rng = np.random.default_rng(7)
    pos = pos + rng.normal(0.0, 0.03, pos.shape)
    gone = rng.random(len(pos)) < 0.01
    gone[1000:1003] = True; gone[2001] = True; gone[2003] = True; gone[64 * 50:64 * 51] = True
    pos[gone, 0] = np.nan
    counts, labels, ok = _compare("absent", pos, box)
    assert (~ok).sum() == gone.sum() > 100 and counts[ok].min() < 12 and (labels[ok] == 1).sum() > 0.5 * len(pos)


def test_windowed_build_with_a_key():
    """a slab of a long box behind mdh_hint_cell_window, the atoms of a cell ordered by a key: the passes over the cells run over
    the window's planes, the rows are those of the oracle on the atoms renumbered by key"""
    pos, box = lattice_positions("fcc", A_CU, 40, 8, 8)
    pos = pos + np.random.default_rng(8).normal(0, 0.05, pos.shape)
    L = np.asarray(box, float)[0][0]
    f = (pos[:, 0] / L) % 1.0
    pos = np.ascontiguousarray(pos[(f >= 0.30) & (f < 0.52)])
    key = np.random.default_rng(3).permutation(len(pos)).astype(np.int64) + 7
    for window in (None, (0.28, 0.54)):
        counts, labels, _ = _compare(("slab", window), pos, box, key=key, window=window)
        _tile_kernel_took_it(("slab", window))
    assert counts.max() >= 12 and (labels == 1).any()


@pytest.mark.parametrize("fused_first", [False, True], ids=["rows_first", "labels_first"])
def test_no_slice_pass_after_a_build_that_listed_nothing(fused_first):
    """one (N, grid), frame after frame, every frame through both entries (the first of the two meets the new frame).  A lattice
    lists nothing, so the next build launches no slice pass; that build meets a dense ball whose tiles overflow the tile kernel's
    LDS budget: the mop-up takes the first pass's tiles, rows and labels are the oracle's, and the count it reports makes the
    build after it launch the slice pass again."""
    lattice, box = lattice_positions("fcc", A_CU, 22, 24, 24)  # (a size no other test builds: the count is kept per (N, grid))
    rng = np.random.default_rng(9)
    lattice = lattice + rng.normal(0.0, 0.03, lattice.shape)
    ball = lattice.copy()
    moved = np.arange(0, len(ball), 14)
    u = rng.normal(size=(len(moved), 3))
    centre = 0.5 * np.diag(np.asarray(box, float))
    ball[moved] = centre + u / np.linalg.norm(u, axis=1)[:, None] * (rng.random((len(moved), 1)) ** (1 / 3)) * 9.0
    seen = []
    for name, pos in (("lattice", lattice), ("lattice again", lattice), ("ball", ball), ("ball again", ball), ("lattice at last", lattice),
                      ("and again", lattice)):
        counts, _, _ = _compare(name, pos, box, fused_first=fused_first)
        _tile_kernel_took_it(name)
        seen.append(_listed_at_plan_time())  # what the SECOND build of the frame found when it planned
        assert (counts.max() > 100) == name.startswith("ball"), (name, int(counts.max()))
    # the second build's plan sees what the first build of the same frame listed
    # (an inference, not a trace: out4[1] is the pinned word the mop-up or the slice pass wrote, as the plan read it; the launcher
    # decides `slice_pass = plan.last_listed != 0` from that same word, so a value > 0 here means the slice pass was launched)
    assert seen[0] == 0 and seen[1] == 0, seen      # nothing listed: the builds from "lattice again" on launch no slice pass
    assert seen[2] > 0 and seen[3] > 0, seen        # the ball's first build ran without a slice pass and reported its tiles; slice pass from then on
    assert seen[4] == 0 and seen[5] == 0, seen      # ... until a build lists nothing again
