"""Host checks of the rule by which k_assign groups the atoms of a 64-atom slice under one returning atomic
(mdapy_amd/csrc/assign_groups.hpp, run on the host through mdh_debug_assign_groups): whatever the sequence of cells, every atom
gets a slot of its own inside its cell, and the heads' counts add up to the cell's population; on the headline lattice the rule
issues as few atomics as any merging inside a slice can — one per distinct cell of the slice.  A slice takes the window rule or
the rule of adjacent runs, whichever issues fewer atomics; the contract is the same under both."""
import os
import sys

import numpy as np
import pytest

from mdapy_amd import _lib


def _groups(cells):
    cells = np.ascontiguousarray(cells, np.int32)
    n = len(cells)
    head, count, rank = (np.full(n, -99, np.int32) for _ in range(3))
    atomics = _lib.lib().mdh_debug_assign_groups(cells.ctypes.data, n, head.ctypes.data, count.ctypes.data, rank.ctypes.data)
    return int(atomics), head, count, rank


def _check(cells):
    """the contract, slice by slice, with the atomics replayed in two different orders -> number of atomics"""
    cells = np.asarray(cells, np.int32)
    atomics, head, count, rank = _groups(cells)
    n = len(cells)
    issued = 0
    for s0 in range(0, n, 64):
        c, h, k, r = (a[s0:s0 + 64] for a in (cells, head, count, rank))
        m = len(c)
        lanes = np.arange(m)
        assert ((h >= 0) & (h <= lanes)).all(), (s0, h.tolist())  # a head sits in the same slice, in front of its members
        is_head = h == lanes
        assert (k[is_head] >= 1).all() and (k[~is_head] == 0).all() and (r[is_head] == 0).all(), s0
        assert is_head[c < 0].all() and (k[c < 0] == 1).all()  # (no group around an atom without a cell; it issues no atomic)
        assert (c[h] == c).all(), s0  # a member's head sits in the member's cell
        assert (h[h] == h).all(), s0  # ... and is a head
        for l in lanes[~is_head]:
            assert 1 <= r[l] < k[h[l]], (s0, l)
        pop = {int(v): int((c == v).sum()) for v in np.unique(c[c >= 0])}
        for v, p in pop.items():
            assert int(k[is_head & (c == v)].sum()) == p, (s0, v)
        issued += int((is_head & (c >= 0)).sum())
        for order in (lanes, lanes[::-1]):  # the atomics land in any order
            counter, base = {}, np.zeros(m, np.int64)
            for l in order:
                if is_head[l] and c[l] >= 0:
                    base[l] = counter.get(int(c[l]), 0)
                    counter[int(c[l])] = int(base[l]) + int(k[l])
            slot = base[h] + r
            for v, p in pop.items():
                assert sorted(slot[c == v].tolist()) == list(range(p)), (s0, v, slot[c == v].tolist())
    assert issued == atomics
    return atomics


def _distinct_per_slice(cells):
    """the floor of any merging inside a slice: the distinct cells (>= 0) of every 64-atom slice, by the brute-force definition"""
    cells = np.asarray(cells, np.int64)
    pad = (-len(cells)) % 64
    c = np.concatenate([cells, np.full(pad, -1)]).reshape(-1, 64)
    c = np.sort(c, axis=1)
    new = np.concatenate([np.ones((len(c), 1), bool), c[:, 1:] != c[:, :-1]], axis=1)
    return int((new & (c >= 0)).sum())


def _tile(pattern, n=64):
    return np.resize(np.asarray(pattern, np.int32), n)


ADVERSARIAL = {
    "ABAB": _tile([5, 9]),
    "ABAB_then_CDCD": (np.arange(64) // 4 * 2 + np.arange(64) % 2).astype(np.int32),
    "ABCA": _tile([5, 9, 2, 5]),
    "AABA": _tile([5, 5, 9, 5]),
    "ABCABC": _tile([1, 2, 3]),
    "all_equal": np.full(64, 7, np.int32),
    "all_distinct": np.arange(64, dtype=np.int32),
    "negatives_mixed_in": _tile([4, -1, 4, 4, -3, 4, -1, -1, 6, 6, -2, 6]),
    "all_negative": -1 - np.arange(64, dtype=np.int32),
    "three_apart": _tile([8, 1, 2, 8, 3, 4]),          # the pair is 3 lanes apart: one group; the next 8 is 3 behind the MEMBER: a head
    "exactly_three_apart_once": np.concatenate([[8, 100, 101, 8], 200 + np.arange(60)]).astype(np.int32),
    "exactly_four_apart_once": np.concatenate([[8, 100, 101, 102, 8], 200 + np.arange(59)]).astype(np.int32),
    "four_apart": _tile([8, 1, 2, 3]),                 # just outside the window: every 8 a head of its own
    "chain_of_equal_every_third": _tile([8, 1, 2]),    # 8 . . 8 . . 8: heads and members alternate
    "group_at_lane_0": np.concatenate([[3, 3, 3, 3], 10 + np.arange(60)]).astype(np.int32),
    "group_at_lane_63": np.concatenate([10 + np.arange(60), [3, 3, 3, 3]]).astype(np.int32),
    "pair_across_60_63": np.concatenate([10 + np.arange(60), [3, 90, 91, 3]]).astype(np.int32),
    "member_at_lane_1_2_3": np.concatenate([[3, 4, 3, 3], 10 + np.arange(60)]).astype(np.int32),
    "head_then_member_then_stranded": _tile([7, 1, 2, 7, 3, 7, 4, 5, 6, 9]),  # the third 7 sees only a member 2 back: own head
    "two_slices_same_cell": np.full(128, 11, np.int32),  # groups never cross a slice
    "short_last_slice": np.concatenate([np.full(64, 2), [2, 2, 5, 2, 5]]).astype(np.int32),
}


@pytest.mark.parametrize("name", list(ADVERSARIAL))
def test_adversarial_sequences(name):
    _check(ADVERSARIAL[name])


def test_expected_groups_of_the_simple_patterns():
    assert _check(ADVERSARIAL["all_equal"]) == 1          # one run (the window rule alone: a head, three members, sixty stranded lanes)
    assert _check(ADVERSARIAL["all_distinct"]) == 64
    assert _check(ADVERSARIAL["all_negative"]) == 0
    assert _check(ADVERSARIAL["ABAB"]) == 62              # A B and their members; from lane 4 on every equal lane in reach is a member
    assert _check(ADVERSARIAL["ABAB_then_CDCD"]) == 32    # what a lattice gives: two heads per four lanes, each with one member
    assert _check(ADVERSARIAL["exactly_three_apart_once"]) == 63
    assert _check(ADVERSARIAL["exactly_four_apart_once"]) == 64
    assert _check(ADVERSARIAL["two_slices_same_cell"]) == 2
    assert _check(ADVERSARIAL["four_apart"]) == 64
    assert _check(ADVERSARIAL["ABCABC"]) == 61            # A B C, their members three behind, then 58 lanes on their own
    _, head, count, rank = _groups([5, 5, 9, 5, 7, 7, 9, 7])
    assert head.tolist() == [0, 0, 2, 0, 4, 4, 6, 4] and count.tolist() == [3, 0, 1, 0, 3, 0, 1, 0]
    assert rank.tolist() == [0, 1, 0, 2, 0, 1, 0, 2]


def test_random_sequences():
    rng = np.random.default_rng(20)
    for trial in range(300):
        n = int(rng.integers(1, 400))
        kind = trial % 4
        if kind == 0:    # few cells: long chains of equal lanes at every distance
            cells = rng.integers(0, int(rng.integers(1, 6)), n)
        elif kind == 1:  # many cells: mostly alone
            cells = rng.integers(0, 1000, n)
        elif kind == 2:  # negatives mixed in
            cells = rng.integers(-3, 5, n)
        else:            # a slowly drifting walk, like atoms in a spatial order
            cells = np.cumsum(rng.integers(0, 2, n)) // int(rng.integers(1, 4)) + rng.integers(0, 2, n) * 50
        _check(cells)


def _bench_cells(ncells):
    """grid cell of every atom of the benchmark's own lattice (bench.slab_positions) at --cells ncells, as k_assign computes it"""
    import torch

    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    if root not in sys.path:
        sys.path.insert(0, root)
    import bench

    x, y, z, _ = bench.slab_positions(torch, torch.device("cpu"), ncells, 0, 0.0)
    L = bench.A_CU * ncells
    nc = max(int(np.floor(L / bench.RC)), 3)  # neighbor_grid_dims
    rc_inv = 1.0 / bench.RC
    c = [np.clip(np.floor(v.numpy() * rc_inv), 0, nc - 1).astype(np.int64) for v in (x, y, z)]  # cell_coords (the atoms are inside the box)
    cell = (c[0] * nc + c[1]) * nc + c[2]
    assert cell.max() < 2 ** 31
    return cell.astype(np.int32)


def _brute_force_atomics(cells):
    """the rule written a second time, on whole arrays: per 64-atom slice the smaller of the atomics of the window rule (an atom
    issues one unless a PRIMARY atom — none of its cell among the three before it — of its cell sits one to three lanes before it)
    and of the rule of adjacent runs -> (atomics, atomics of the window rule alone, atomics of the runs alone)"""
    cells = np.asarray(cells, np.int64)
    pad = (-len(cells)) % 64
    c = np.concatenate([cells, -1 - np.arange(pad)])
    lane = np.arange(len(c)) % 64
    eq = []
    for d in (1, 2, 3):
        before = np.concatenate([np.full(d, -1), c[:-d]])
        eq.append((c >= 0) & (lane >= d) & (before == c))
    primary = ~(eq[0] | eq[1] | eq[2])
    member = np.zeros(len(c), bool)
    for d in (1, 2, 3):
        member |= eq[d - 1] & np.concatenate([np.zeros(d, bool), primary[:-d]])
    window = (~member & (c >= 0)).reshape(-1, 64).sum(axis=1)
    runs = (((lane == 0) | (np.concatenate([[-1], c[:-1]]) != c)) & (c >= 0)).reshape(-1, 64).sum(axis=1)
    return int(np.minimum(window, runs).sum()), int(window.sum()), int(runs.sum())


def test_headline_lattice_reaches_the_floor_of_in_slice_merging():
    """The benchmark's 10 061 824 atoms in the lattice builder's order (bench.slab_positions at --cells 136, binned as k_assign bins
    them: 159^3 cells of width rc).  The atomics the twin issues equal the number of distinct cells per 64-atom slice, counted by
    sorting every slice — no merging inside a slice can issue fewer.  The figures: 6 733 067 atomics, 8 232 352 under the rule of
    adjacent runs that this replaces (ratio 0.818).  The issue that asked for this rule quotes 6 850 067 and 8 329 252 (ratio 0.822)
    from a replay of its own; no order of the fcc basis and neither rounding of x / rc reproduces those from the benchmark's
    positions, so the expected value here is the brute-force count, not the quoted one."""
    cells = _bench_cells(136)
    assert len(cells) == 10061824
    atomics, head, count, rank = _groups(cells)
    floor = _distinct_per_slice(cells)
    both, window, runs = _brute_force_atomics(cells)
    print(f"headline lattice: twin {atomics}, distinct cells per slice {floor}, second implementation {both} "
          f"(window rule alone {window}, adjacent runs alone {runs})")
    assert atomics == floor == both == window == 6733067
    assert runs == 8232352
    assert runs > 1.2 * atomics
    lanes = np.arange(len(cells)) % 64
    assert int(((head == lanes) & (cells >= 0)).sum()) == atomics and int(count.sum()) == len(cells)


def test_small_lattice_against_the_second_implementation():
    """--cells 40 (256 000 atoms): the count recomputed from the definition of the rule; the contract checked slot by slot on the first
    600 slices"""
    cells = _bench_cells(40)
    atomics = _groups(cells)[0]
    both, window, runs = _brute_force_atomics(cells)
    floor = _distinct_per_slice(cells)
    print(f"40^3 lattice: twin {atomics}, second implementation {both} (window {window}, runs {runs}), distinct cells per slice {floor}")
    assert atomics == both and floor <= atomics <= min(window, runs)
    assert atomics < 1.03 * floor  # (within 3 % of the floor: the slices cut the lattice's rows at other places than at 136^3)
    sub = cells[:64 * 600]
    assert _check(sub) == _brute_force_atomics(sub)[0]


def test_random_sequences_against_the_second_implementation():
    rng = np.random.default_rng(21)
    for trial in range(200):
        cells = rng.integers(-2, int(rng.integers(1, 40)), int(rng.integers(1, 700)))
        assert _groups(cells)[0] == _brute_force_atomics(cells)[0], trial
