"""-m gpu: sequences of DIFFERENT consecutive frames through every path that keeps state from one call to the next.

Every other parity test builds a fresh object on one frame, and where it calls twice it repeats the frame; a drop-in for trajectory
analysis is used on a sequence of different frames.  The frames come from tests/_trajectory.py, the expected answer of a frame is
the oracle's on that frame alone, and every comparison is bitwise (rattled crystals and gases: no exact ties in distance).

  B1  neighbor_cna_step(..., reuse_buffers=True): the four result arrays kept on the decomposition
  B2  System after System: the permutation of the last sorted System (_twin.py _last)
  B3  the k-nearest searches of one System that share candidate rows (knn.py), and the signature table of knn.hip
  B4  atoms the rows build does not bin (counts of the rows build)"""
import ctypes
import functools
import itertools
import os

import numpy as np
import pytest

import _trajectory as T

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
RC_CNA = 0.854 * 3.615


def _report(fn):
    """run fn with the event ranges on -> (knn_rows_build, knn_rows_select): cutoff builds for candidate rows, searches from rows"""
    from mdapy_amd import _lib

    L = _lib.lib()
    L.mdh_prof_reset(); L.mdh_prof_enable(1)
    try:
        fn()
    finally:
        L.mdh_prof_enable(0)
    buf = ctypes.create_string_buffer(4096)
    L.mdh_prof_report(buf, 4096)
    rec = {ln.split()[0]: int(ln.split()[1]) for ln in buf.value.decode().strip().splitlines() if ln}
    return rec.get("knn_rows_build", 0), rec.get("knn_rows_select", 0)


# ================================================================================================================================
# B1  the decomposed step with kept buffers
# ================================================================================================================================
def _sequence_rank(rank, world, torch, mode="plain"):
    """A -> gap -> A -> drift (re-partitioned) -> A through ONE SlabDecomposition with reuse_buffers=True, on tensors with room behind
    them (the static exchange: a ghost block of fixed size whose unused slots are absent atoms — the only exchange under which the
    signature of the kept buffers survives a change of the ghost count).  mode: "plain", "prefetch" (next_frame given: the next
    exchange starts before this frame's kernels) or "wide" (rows of 132 slots, beyond the tile kernel's 128: every step runs on the
    kernels behind it, which write the rows of ALL ghosts).  -> (names of the checks that failed, owned atoms, ghosts of frame A)"""
    import mdapy_amd as mp
    import mdapy_amd.distributed as D
    from mdapy_amd import _lib

    dev = torch.device("cuda", 0)
    A, rc = T.decomposed_frame()
    faces = [r / max(world, 2) for r in range(max(world, 2))]
    G = T.gap(A, 0, faces, rc)
    Dr = T.drift(A, np.random.default_rng(77), 0.25)  # (of the ~140 atoms within 0.25 A of a face, half cross it)
    frames = [("A", A), ("gap", G), ("A again", A), ("drift", Dr), ("A at last", A)]
    want = {id(f): T.expected_cutoff(f, rc) for f in (A, G, Dr)}
    # rows wide enough for every frame (the oracle's largest count: the atoms `gap` moved land among others) — row overflow, which
    # only a reader of the counts notices, stays out of this test; one width for all frames, or the kept buffers would be dropped
    M = 132 if mode == "wide" else max(int(w["counts"].max()) for w in want.values())
    box = mp.Box(A.box)
    dec = D.SlabDecomposition(box, rank, world, axis=0)
    bad = []

    def check(name, ok):
        if not bool(ok):
            bad.append(name)

    def tensors(d, frame):
        ids = D.partition_atoms(frame.pos, box, world, axis=0)[rank]
        t = lambda a: d.with_room(torch.from_numpy(np.ascontiguousarray(a)).to(dev), 0.6)
        return ids, (t(frame.pos[ids, 0]), t(frame.pos[ids, 1]), t(frame.pos[ids, 2]), t(ids))

    def look(tag, frame, ids, out):
        """owned rows against the oracle's for the whole frame; absent slots against their contract -> what to compare with a fresh run"""
        dom, v, d, nn, pat = out
        e = want[id(frame)]
        own, gid = dom.owned.cpu().numpy(), dom.gid.cpu().numpy()
        v, d, nn, pat = v.cpu().numpy(), d.cpu().numpy(), nn.cpu().numpy(), pat.cpu().numpy()
        g_own = gid[own]
        check(tag + "owned set", own.sum() == len(ids) and np.array_equal(np.sort(g_own), np.sort(ids)) and int(dom.n_owned) == len(ids))
        w = e["rows"].shape[1]
        rows = np.where(v[own] >= 0, gid[np.clip(v[own], 0, None)], -1)
        check(tag + "rows", np.array_equal(rows[:, :w], e["rows"][g_own]) and (rows[:, w:] == -1).all())
        check(tag + "counts", np.array_equal(nn[own], e["counts"][g_own]))
        check(tag + "distances", np.array_equal(d[own][:, :w], e["dist"][g_own]) and (d[own][:, w:] == rc + 1.0).all())
        check(tag + "labels", np.array_equal(pat[own], e["cna"][g_own]))
        gone = gid < 0
        check(tag + "absent slots lie behind the owned atoms and hold x = NaN", not gone[:len(ids)].any()
              and np.array_equal(np.isnan(dom.x.cpu().numpy()), gone))
        check(tag + "absent slots: nn == 0", (nn[gone] == 0).all())
        check(tag + "absent slots: verlet == -1", (v[gone] == -1).all())
        check(tag + "absent slots: dist == rc + 1", (d[gone] == rc + 1.0).all())
        check(tag + "absent slots: pattern == 0", (pat[gone] == 0).all())
        by_id = np.argsort(g_own)  # (a fresh decomposition may hold the owned atoms in another order)
        return {"rows": rows[by_id], "dist": d[own][by_id], "counts": nn[own][by_id], "labels": pat[own][by_id],
                "ghosts": int((gid >= 0).sum()) - len(ids), "absent": int(gone.sum())}

    sets = [tensors(dec, f) for _, f in frames]
    plan = np.zeros(8, np.int32)
    seen, kept_rows = [], []
    for step, (name, frame) in enumerate(frames):
        ids, args = sets[step]
        nxt = sets[step + 1][1] if mode == "prefetch" and step + 1 < len(frames) else None
        out = D.neighbor_cna_step(dec, *args, rc, M, next_frame=nxt, reuse_buffers=True)
        torch.cuda.synchronize()
        _lib.lib().mdh_debug_neighbor_plan(plan.ctypes.data)
        tag = f"step {step} ({name}): "
        if mode == "wide":
            check(tag + f"the tile kernel refused rows of {M} slots (plan {plan.tolist()})", plan[0] == 0 and plan[6] == -1)
        else:
            check(tag + f"the tile kernel took the step (plan {plan.tolist()})", plan[0] > 0)
        got = look(tag, frame, ids, out)
        kept_rows.append(out[1].data_ptr())
        if world > 1:
            check(tag + "static exchange taken", getattr(out[0], "absent_slots", False) and got["absent"] > 0)
            check(tag + "the kept arrays are the ones returned", dec._step_buffers[1][0] is out[1])
            if mode == "prefetch":
                check(tag + "the next exchange is under way", len(dec._pending) == (1 if nxt is not None else 0))
        seen.append(got)
        # the same frame through a FRESH decomposition without kept buffers: owned rows the same, absent slots under the same contract
        fresh_dec = D.SlabDecomposition(box, rank, world, axis=0)
        ids_f, args_f = tensors(fresh_dec, frame)
        fresh = look(tag + "fresh: ", frame, ids_f, D.neighbor_cna_step(fresh_dec, *args_f, rc, M, reuse_buffers=False))
        for key in ("rows", "dist", "counts", "labels", "ghosts"):
            check(tag + "equals the fresh decomposition's " + key, np.array_equal(got[key], fresh[key]))
    dec._drop_pending()
    torch.cuda.synchronize()
    dec.check_halo()
    if world > 1:
        # without these the sequence proves nothing: the gap frame has fewer ghosts (more absent slots) than A on THIS rank, the
        # buffers of A were the gap frame's and the second A's, and the drift frame changed the slab's atoms
        check(f"gap has fewer ghosts than A ({seen[1]['ghosts']} < {seen[0]['ghosts']})", 0 <= seen[1]["ghosts"] < seen[0]["ghosts"])
        check("A has the same ghosts each time", seen[0]["ghosts"] == seen[2]["ghosts"] == seen[4]["ghosts"] > 0)
        check("A, gap and A again share their arrays", kept_rows[0] == kept_rows[1] == kept_rows[2])
        check("the drift frame moved atoms across a face", not np.array_equal(sets[3][0], sets[0][0]))
    return bad, len(sets[0][0]), seen[0]["ghosts"]


MODES = ["plain", "prefetch", "wide"]


@pytest.mark.parametrize("mode", MODES)
def test_kept_buffers_world1(mode):
    """one rank, in process: no ghosts and no absent slots, so the reuse branch (which needs ghosts to skip) is not taken — the
    sequence still has to equal the oracle frame by frame"""
    import torch

    bad, n_own, n_ghost = _sequence_rank(0, 1, torch, mode)
    assert bad == [] and n_ghost == 0 and n_own == 21952


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("world", [2, 4])
def test_kept_buffers_follow_a_sequence_of_different_frames(world, mode):
    """A -> gap -> A -> drift -> A through one decomposition with reuse_buffers=True, as gloo ranks that share the GPU.  After EVERY
    step: owned rows, counts, distances and labels equal the oracle's for the undivided frame; every slot with dom.gid < 0 has
    nn == 0, verlet == -1, dist == rc + 1 and pattern == 0; owned rows equal a fresh decomposition's with reuse_buffers=False.  Ghost
    rows are unspecified (distributed.py) and not compared.  `gap` empties the ghost layers while every slab keeps its atoms: slots
    that held a ghost WITH a row in step t hold an absent atom in step t + 1 — in "wide" every ghost had a row (the kernels behind
    the tile kernel write them all).  The reuse branch needs device tensors (`is_cuda`): there is no CPU twin of this test."""
    from test_gpu_distributed import _spawn

    res = _spawn(world, functools.partial(_sequence_rank, mode=mode))
    for rank, bad, n_own, n_ghost in sorted(res):
        assert bad == [], f"rank {rank}: {bad}"
        assert n_own > 0 and n_ghost > 0
    assert sum(r[2] for r in res) == 21952


# ================================================================================================================================
# B2  System trajectories and the remembered permutation
# ================================================================================================================================
def _bcc_sheared():
    return T.sheared(T.start("bcc", (20, 20, 20), seed=31, a=2.87, rattle=0.05))


def _fcc():
    return T.start("fcc", (16, 16, 16), seed=32, rattle=0.07)


# name -> (first frame, steps, what happens to the permutation frame by frame, memory space of the columns frame by frame)
TRAJECTORIES = {
    "drift_drift": (_bcc_sheared, ["drift", "drift"], ["sort", "reuse", "reuse"], None),
    "jump_drift": (_fcc, ["jump", "drift"], ["sort", "reuse", "reuse"], None),
    "drift_renumber_drift": (_fcc, ["drift", "renumber", "drift"], ["sort", "reuse", "sort", "reuse"], None),
    "resize": (lambda: T.start("gas", (16, 16, 16), seed=33), ["resize"], ["sort", "sort"], None),
    "reshape": (lambda: T.open_along(_fcc(), 2), ["reshape"], ["sort", "reuse"], None),
    "repbc": (lambda: T.start("bcc", (20, 20, 20), seed=34, a=2.87, rattle=0.05), ["repbc"], ["sort", "sort"], None),
    # (the order statistic that decides about a twin reads the columns on the device, so host columns have a device mirror by the
    # time the permutation is looked up: the memory space of a frame's columns does not send it to the sort)
    "host_device_and_back": (_fcc, ["drift"] * 4, ["sort", "reuse", "reuse", "reuse", "reuse"], "hddhh"),
    "drift_nan_drift": (_fcc, ["drift", "nan_atom", "drift"], ["sort", "reuse", "none", "none"], None),
}


def _system(frame, space):
    import mdapy_amd as mp
    from mdapy_amd.devarray import HArray
    from mdapy_amd.frame import Frame

    box = mp.Box(frame.box, boundary=[int(b) for b in frame.boundary], origin=frame.origin)
    if space == "h":
        return mp.System(pos=frame.pos, box=box)
    return mp.System(data=Frame({c: HArray.from_numpy(col) for c, col in zip("xyz", frame.xyz())}), box=box)


def _analyse(frames, spaces, rc, k):
    from mdapy_amd import _twin as twin_mod
    from mdapy_amd.devarray import as_numpy

    twin_mod.forget_order()
    out, last = [], None
    for f, space in zip(frames, spaces):
        s = _system(f, space)
        s.cal_common_neighbor_analysis(rc=rc)
        res = {"cna": s.data["cna"].to_numpy().copy(), "rows": as_numpy(s.verlet_list).copy(), "dist": as_numpy(s.distance_list).copy(),
               "counts": as_numpy(s.neighbor_number).copy()}
        s.build_nearest_neighbor(k)
        res["knn_rows"], res["knn_dist"] = as_numpy(s.verlet_list).copy(), as_numpy(s.distance_list).copy()
        twin = s._spatial()
        if twin is None:
            how = "none"
        else:
            perm = np.asarray(as_numpy(twin._perm))
            assert np.array_equal(np.sort(perm), np.arange(f.n)) and twin.N == f.n
            how = "reuse" if last is not None and twin._perm is last else "sort"
            last = twin._perm
        out.append((how, res))
    return out


@pytest.mark.parametrize("name", list(TRAJECTORIES))
def test_system_after_system_equals_the_oracle_frame_by_frame(monkeypatch, name):
    """one System per frame (fixed-cutoff CNA and a 12-nearest list each), on the path systems of 200 000 atoms and more take: the
    threshold is lowered to 10 000 for the test, so that the oracle's brute-force search stays cheap (NOT MDAPY_SPATIAL_SORT=1,
    which skips the order statistic in front of the twin — with it, fresh host columns have no device mirror yet when the
    permutation is looked up and every frame is sorted).  Every frame's lists, counts, distances and
    labels equal the oracle on that frame alone and a run of the same sequence with MDAPY_REUSE_ORDER=0.  WHICH frames were read
    through the previous frame's permutation is asserted through twin._perm — a run that sorts every frame fails.  A frame with an
    absent atom (x = NaN) gets no twin whether a permutation is remembered or not (tests/test_gpu_order.py
    test_absent_atoms_make_the_sort_stand_down is the first frame's contract); its finite atoms' results equal the oracle's over the
    finite atoms, its own k-nearest row is not compared here (B4 pins it)."""
    from mdapy_amd import _twin as twin_mod

    monkeypatch.delenv("MDAPY_SPATIAL_SORT", raising=False)
    monkeypatch.setattr(twin_mod, "SORT_MIN_ATOMS", 10000)
    first, steps, want, spaces = TRAJECTORIES[name]
    f0 = first()
    rc = RC_CNA if f0.n != 16000 else 1.2 * 2.87  # (bcc: first and second shell)
    frames = T.sequence(f0, steps, seed=35)
    spaces = spaces or "h" * len(frames)
    got = _analyse(frames, spaces, rc, 12)
    assert [g[0] for g in got] == want
    monkeypatch.setenv("MDAPY_REUSE_ORDER", "0")
    plain = _analyse(frames, spaces, rc, 12)
    assert [g[0] for g in plain] == [w if w == "none" else "sort" for w in want]
    for step, (f, (how, res), (_, res0)) in enumerate(zip(frames, got, plain)):
        ok = T.finite(f)
        assert ok.all() == (how != "none"), (name, step)
        e, k = T.expected_cutoff(f, rc), T.expected_knn(f, 12)
        for key in ("rows", "dist", "counts", "cna"):
            assert res[key].shape == e[key].shape and np.array_equal(res[key][ok], e[key][ok]), (name, step, how, key)
        assert np.array_equal(res["knn_rows"][ok], k["rows"][ok]) and np.array_equal(res["knn_dist"][ok], k["dist"][ok]), (name, step, how)
        for key in res:
            assert np.array_equal(res[key][ok], res0[key][ok]), (name, step, how, key, "MDAPY_REUSE_ORDER=0")
        if name != "resize" and not np.any(f.box - np.diag(np.diag(f.box))):  # (a gas and a sheared crystal have few labelled atoms)
            assert (e["cna"] > 0).sum() > 0.5 * f.n, (name, step)


# ================================================================================================================================
# B3  k-nearest searches that share rows
# ================================================================================================================================
ANALYSES = {  # name -> (k of its search, call, columns it leaves)
    "csp": (12, lambda s: s.cal_centro_symmetry_parameter(12), ("csp",)),
    "acna": (14, lambda s: s.cal_common_neighbor_analysis(), ("cna",)),
    "ptm": (18, lambda s: s.cal_polyhedral_template_matching(return_rmsd=True), ("ptm", "rmsd")),
}


def _own_radius(k):
    return (k + 1.0) ** (1.0 / 3.0)  # (knn.hip r_own, up to the factor the density gives: the same for every k of one system)


@pytest.mark.parametrize("order", list(itertools.permutations(ANALYSES)), ids="-".join)
def test_analyses_of_one_system_share_candidate_rows_in_every_order(monkeypatch, order):
    """CSP (12 nearest), adaptive CNA (14) and PTM (18) on ONE System in all six orders: every column equals that of three fresh
    Systems.  Read from the event ranges: an analysis that searches (knn_rows_select) builds candidate rows (knn_rows_build) exactly
    when the rows kept with the position columns do not reach nine tenths of its own radius (mdh_knn_keyed_rows) — the first search
    always does, the 18-nearest search behind a 12-nearest one does, nothing else: ONE build per System when the rows reach, more
    when they do not.  An analysis that borrows the remembered list searches nothing and builds nothing."""
    import mdapy_amd as mp

    monkeypatch.setenv("MDH_KNN_ROWS_MIN", "1000")
    f = T.start("fcc", (14, 14, 14), seed=41, rattle=0.06, shuffle=False)
    box = mp.Box(f.box)
    alone = {}
    for name in ANALYSES:
        q = mp.System(pos=f.pos, box=box)
        ANALYSES[name][1](q)
        alone.update({c: q.data[c].to_numpy().copy() for c in ANALYSES[name][2]})
    s = mp.System(pos=f.pos, box=box)
    kept, builds, log = None, 0, []
    for name in order:
        k, call, _ = ANALYSES[name]
        b, sel = _report(lambda: call(s))
        log.append((name, b, sel))
        if sel == 0:
            assert b == 0, log
            continue
        reach = kept is not None and _own_radius(kept) >= 0.9 * _own_radius(k)
        assert (b, sel) == ((0, 1) if reach else (1, 1)), (log, kept)
        if b:
            kept = k
        builds += b
    assert log[0][1:] == (1, 1), log  # the rows path did take the first search
    searched = [n for n, _, sel in log if sel]
    assert builds == 1 + int(_rows_do_not_reach(searched)), log
    for c, want in alone.items():
        assert np.array_equal(s.data[c].to_numpy(), want, equal_nan=True), (order, c)
    assert (alone["ptm"] > 0).sum() > 0.5 * f.n and (alone["cna"] > 0).sum() > 0.5 * f.n  # (a rattled crystal: the analyses did label)


def _rows_do_not_reach(searched):
    """does some search of the sequence find kept rows that are too short?  (12 -> 18 is the one such pair: 13^(1/3) < 0.9 * 19^(1/3))"""
    kept = None
    for name in searched:
        k = ANALYSES[name][0]
        if kept is not None and _own_radius(kept) < 0.9 * _own_radius(k):
            return True
        if kept is None or _own_radius(kept) < 0.9 * _own_radius(k):
            kept = k
    return False


def test_new_positions_on_the_same_system_borrow_nothing(monkeypatch):
    """update_data with new position columns on a System that has searched: the candidate rows belonged to the OLD columns — a new
    knn_rows_build runs and the list equals the oracle's on the new positions"""
    import mdapy_amd as mp
    from mdapy_amd.devarray import as_numpy

    monkeypatch.setenv("MDH_KNN_ROWS_MIN", "1000")
    f = T.start("fcc", (14, 14, 14), seed=42, rattle=0.06, shuffle=False)
    g = T.drift(f, np.random.default_rng(43), 0.10)
    s = mp.System(pos=f.pos, box=mp.Box(f.box))
    assert _report(lambda: s.build_nearest_neighbor(12)) == (1, 1)
    assert _report(lambda: s.build_nearest_neighbor(14)) == (0, 1)  # (the rows are kept: that is what the next line must NOT use)
    x, y, z = g.xyz()
    s.update_data(s.data.with_columns(x=x, y=y, z=z), reset_neighbor=True)
    assert _report(lambda: s.build_nearest_neighbor(14)) == (1, 1)
    e = T.expected_knn(g, 14)
    assert np.array_equal(as_numpy(s.verlet_list), e["rows"]) and np.array_equal(as_numpy(s.distance_list), e["dist"])
    assert not np.array_equal(e["rows"], T.expected_knn(f, 14)["rows"])  # (the old positions' rows would not have passed)


def test_signature_table_of_the_rows_path_never_changes_a_result(monkeypatch):
    """knn.hip keeps, per (N, k, pbc, volume), how many queries of the last search the rows left to the cell walk; above 0.5 % the
    next 15 searches of that signature walk the cells at once.  (1) a gas leaves skip = 15; (2) a rattled crystal with the SAME N,
    k, pbc and volume therefore goes through the cell walk — and must equal the oracle exactly as it does on the rows path; (3) 17
    searches of distinct signatures wrap the 16-entry table; (4) the first two systems again: the gas is a new signature again.
    Results never depend on the path; the path is asserted where the code makes it certain (the signature is new, or was just set)."""
    from mdapy_amd import _fast_knn

    monkeypatch.setenv("MDH_KNN_ROWS_MIN", "1000")
    cells, k = (13, 12, 11), 12  # (6 864 atoms: a signature no other test of this process uses)
    gas, crystal = T.start("gas", cells, seed=51), T.start("fcc", cells, seed=52)
    assert gas.n == crystal.n and np.array_equal(gas.box, crystal.box)

    def search(f):
        idx, dist = np.zeros((f.n, k), np.int32), np.zeros((f.n, k))
        path = _report(lambda: _fast_knn.knn(*f.where(), k, idx, dist, 1))
        e = T.expected_knn(f, k)
        assert np.array_equal(dist, e["dist"]) and np.array_equal(idx, e["rows"]), path
        return path

    for visit in range(2):
        assert search(gas) == (1, 1), visit          # a new signature: rows built, most queries left over -> skip = 15
        assert search(crystal) == (0, 0), visit      # the gas's verdict sends the crystal through the cell walk
        if visit == 0:
            for extra in range(17):                  # 17 distinct (N, ...) signatures: the table wraps, the gas's entry is gone
                small = T.resize(gas, np.random.default_rng(60 + extra), share=(1200.5 + 7 * extra) / gas.n)
                assert small.n == 1200 + 7 * extra
                search(small)


def test_ids_only_rows_of_a_search_do_not_reach_the_next_build(monkeypatch):
    """A k-nearest search on the rows path asks its cutoff build for ids only (32-slot rows on the tile kernel's wide instance, which
    then neither computes nor stores a distance).  That belongs to the search's own build: build_neighbor(rc = 4.3, 32 slots,
    fill_pads) on the same thread right behind it — the same instance, asserted through mdh_debug_neighbor_plan — writes ids,
    distances and counts bit-equal to the oracle's, and so it does in front of the search; the search equals the oracle both times."""
    from mdapy_amd import _fast_knn, _lib, _neighbor
    from oracle import oracle as O

    monkeypatch.setenv("MDH_KNN_ROWS_MIN", "1000")
    f = T.start("fcc", (12, 12, 12), seed=71, rattle=0.05, shuffle=False)
    assert f.n == 6912
    k, rc, M = 18, 4.3, 32  # (the search's own radius is ~4.3 A here: the box spans >= 7.5 radii, >= 7 cells per axis)
    want_v, want_d, want_n = np.full((f.n, M), -1, np.int32), np.full((f.n, M), rc + 1.0), np.zeros(f.n, np.int32)
    O.build_neighbor(*f.where(), rc, want_v, want_d, want_n, 8)
    assert 12 < want_n.max() <= M
    want_knn = T.expected_knn(f, k)
    plan = np.zeros(8, np.int32)

    def search():
        idx, dist = np.zeros((f.n, k), np.int32), np.zeros((f.n, k))
        assert _report(lambda: _fast_knn.knn(*f.where(), k, idx, dist, 1)) == (1, 1)  # (rows built, searched from the rows)
        assert np.array_equal(idx, want_knn["rows"]) and np.array_equal(dist, want_knn["dist"])

    def build():
        v, d, n = np.empty((f.n, M), np.int32), np.full((f.n, M), np.nan), np.empty(f.n, np.int32)
        _lib.lib().mdh_debug_neighbor_plan(plan.ctypes.data)  # ([7] = 0 from here on: the plan read below is this build's)
        _neighbor.build_neighbor(*f.where(), rc, v, d, n, 1, fill_pads=True)
        _lib.lib().mdh_debug_neighbor_plan(plan.ctypes.data)
        assert plan[7] == 1 and plan[0] > 0 and not plan[4] & 2, plan.tolist()  # the tile kernel took it, wide instance
        assert np.array_equal(v, want_v) and np.array_equal(d, want_d) and np.array_equal(n, want_n)

    search(); build()
    build(); search()


# ================================================================================================================================
# B4  atoms the rows build does not bin
# ================================================================================================================================
def _rows_search(f, k, bag):
    from mdapy_amd import _fast_knn
    from mdapy_amd.devarray import HArray, as_numpy

    x, y, z = (HArray.from_numpy(c) for c in f.xyz())
    idx, dist = HArray.empty((f.n, k), np.int32), HArray.empty((f.n, k), np.float64)
    if bag is None:
        _fast_knn.knn(x, y, z, f.box, f.origin, f.boundary, k, idx, dist, 1)
    else:
        _fast_knn.knn(x, y, z, f.box, f.origin, f.boundary, k, idx, dist, 1, candidates=bag)
    return as_numpy(idx).copy(), as_numpy(dist).copy()


@pytest.mark.parametrize("case", ["nan_x", "nan_y", "far_above_an_open_box"])
def test_rows_path_with_an_atom_outside_the_build(monkeypatch, case):
    """_fast_knn.knn with a candidates dict (mdh_knn_keyed_rows with the caller's buffers, which nobody zeroed) on a frame whose rows
    build leaves one atom without a row: x = NaN (an absent atom: binned nowhere) and y = NaN (binned, but no distance to it
    compares).  Every finite atom's row equals the brute-force oracle over the finite atoms, the odd atom appears in no row, and its
    own row is what the cell walk writes for it: ids -1, distances -1.0 (include/mdapy_amd.h, mdh_knn_keyed_rows).  Twice with the
    same dict: the second search (k = 14) runs from the kept rows and counts.  An atom far outside an open box IS binned by the
    build (into the last cell of its axis, grid.hpp), so that case is an ordinary search: all rows equal the oracle's."""
    monkeypatch.setenv("MDH_KNN_ROWS_MIN", "1000")
    f = T.start("fcc", (14, 14, 14), seed=61, rattle=0.06)
    rng = np.random.default_rng(62)
    if case == "far_above_an_open_box":
        f = T.open_along(f, 2)
        pos = f.pos.copy()
        pos[int(rng.integers(f.n)), 2] += 3.0 * f.box[2, 2]
        f = T._frame(pos, f.box, f.origin, f.boundary)
    else:
        f = T.nan_atom(f, rng, coordinate=0 if case == "nan_x" else 1)
    ok = T.finite(f)
    bag = {}
    for k, path in ((12, (1, 1)), (14, (0, 1))):
        got = {}
        took = _report(lambda: got.update(rows=_rows_search(f, k, bag)))
        # (k = 14 from the rows kept of k = 12: certain in the bulk; the surface atoms of the open box leave more than 0.5 % of the
        # queries unfinished and the rows are built again — the path is not asserted there)
        assert (took == path or (k == 14 and case == "far_above_an_open_box" and took[1] >= 1)) and "rows" in bag, (case, k, took)
        idx, dist = got["rows"]
        e = T.expected_knn(f, k)
        assert np.array_equal(idx[ok], e["rows"][ok]) and np.array_equal(dist[ok], e["dist"][ok]), (case, k)
        if ok.all():
            continue
        odd = int(np.nonzero(~ok)[0][0])
        assert not (idx[ok] == odd).any(), (case, k)
        monkeypatch.setenv("MDH_KNN_ROWS_MIN", "1000000000")
        walk_idx, walk_dist = _rows_search(f, k, None)
        monkeypatch.setenv("MDH_KNN_ROWS_MIN", "1000")
        print(case, k, "the odd atom's row:", idx[odd].tolist(), dist[odd].tolist(), "cell walk:", walk_idx[odd].tolist(), walk_dist[odd].tolist())
        assert np.array_equal(walk_idx[ok], e["rows"][ok]) and np.array_equal(walk_dist[ok], e["dist"][ok]), (case, k)
        assert np.array_equal(idx[odd], walk_idx[odd]) and np.array_equal(dist[odd], walk_dist[odd], equal_nan=True), (case, k)
        assert (idx[odd] == -1).all() and (dist[odd] == -1.0).all(), (case, k)


def test_rows_of_a_width_that_is_no_multiple_of_four_are_refused():
    """k_knn_rows reads a row in 16-byte groups: mdh_knn_keyed_rows rejects such buffers with MDH_ERR_ARG before any kernel runs"""
    from mdapy_amd import _lib
    from mdapy_amd.devarray import HArray

    f = T.start("fcc", (6, 6, 6), seed=63)
    L = _lib.lib()
    keep, (pb, po, pp) = _lib.host_box(f.box, f.origin, f.boundary)
    x, y, z = (HArray.from_numpy(c) for c in f.xyz())
    idx, dist = HArray.empty((f.n, 12), np.int32), HArray.empty((f.n, 12), np.float64)
    rows, counts = HArray.empty((f.n, 34), np.int32), HArray.empty((f.n,), np.int32)
    radius = ctypes.c_double(0.0)
    rc_ = L.mdh_knn_keyed_rows(x.data_ptr(), y.data_ptr(), z.data_ptr(), f.n, pb, po, pp, 12, idx.data_ptr(), dist.data_ptr(), None,
                               rows.data_ptr(), counts.data_ptr(), 34, ctypes.addressof(radius), _lib.DEVICE, None)
    assert rc_ == _lib.ERR_ARG and b"multiple of four" in L.mdh_last_error()
