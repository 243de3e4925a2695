"""The cell-sorted twin of ``System`` (mdapy_amd/system.py): a system handed in in no spatial order is analysed on a sorted
copy and every result the user reads is translated back.  Checked here on the CPU with the kernels routed to the oracle
(fixture ``oracle_backend``; the sort itself is a numpy stand-in — any permutation serves the host logic): every analysis
of a shuffled system with the twin forced on (MDAPY_SPATIAL_SORT=1) against the same system analysed in the order it has
(MDAPY_SPATIAL_SORT=0) — labels, lists (ids, ROW ORDER, distances, counts) and floating-point columns bit for bit."""
import numpy as np
import pytest

import mdapy_amd as mp
from mdapy_amd.build_lattice import lattice_positions
from mdapy_amd.devarray import as_numpy


def _system(monkeypatch, mode, seed=3, with_types=False, cells=(7, 6, 6)):
    monkeypatch.setenv("MDAPY_SPATIAL_SORT", mode)
    pos, box = lattice_positions("fcc", 3.615, *cells)
    rng = np.random.default_rng(seed)
    pos = pos + rng.normal(0, 0.12, pos.shape)
    order = rng.permutation(len(pos))
    pos = pos[order]
    data = {"x": pos[:, 0], "y": pos[:, 1], "z": pos[:, 2]}
    if with_types:
        data["type"] = rng.integers(1, 3, len(pos)).astype(np.int32)
        data["vx"], data["vy"], data["vz"] = (rng.normal(0, 1.0, len(pos)) for _ in range(3))
        data["amass"] = np.where(data["type"] == 1, 63.5, 91.2)
    return mp.System(data=data, box=box)


def _same_columns(a, b, names):
    for n in names:
        va, vb = a.data[n].to_numpy(), b.data[n].to_numpy()
        assert va.dtype == vb.dtype and np.array_equal(va, vb, equal_nan=True), n


def test_twin_is_made_and_lists_translate_bit_for_bit(oracle_backend, monkeypatch):
    plain, twin = _system(monkeypatch, "0"), _system(monkeypatch, "1")
    plain.build_neighbor(3.9, max_neigh=30)
    twin.build_neighbor(3.9, max_neigh=30)
    assert plain._spatial() is None
    t = twin._spatial()
    assert t is not None and sorted(np.asarray(t._perm).tolist()) == list(range(twin.N))
    for name in ("verlet_list", "distance_list", "neighbor_number"):
        assert np.array_equal(as_numpy(getattr(plain, name)), as_numpy(getattr(twin, name))), name
    assert twin.rc == plain.rc == 3.9
    # exact-width rows
    plain.build_neighbor(3.3); twin.build_neighbor(3.3)
    for name in ("verlet_list", "distance_list", "neighbor_number"):
        assert np.array_equal(as_numpy(getattr(plain, name)), as_numpy(getattr(twin, name))), name
    # k nearest
    plain.build_nearest_neighbor(9)
    twin.build_nearest_neighbor(9)
    assert np.array_equal(as_numpy(plain.distance_list), as_numpy(twin.distance_list))
    assert np.array_equal(as_numpy(plain.verlet_list), as_numpy(twin.verlet_list))  # (no exact ties in a rattled crystal)
    assert "rc" in twin.__dict__  # (the reference keeps rc behind a k-nearest list, system.py:1256-1263)


def test_every_twin_analysis_equals_the_plain_one(oracle_backend, monkeypatch):
    out = {}
    for mode in ("0", "1"):
        s = _system(monkeypatch, mode, with_types=True)
        s.cal_common_neighbor_analysis(rc=0.854 * 3.615)
        s.cal_common_neighbor_analysis()
        s.data  # noqa
        cna_adaptive = s.data["cna"].to_numpy().copy()
        s.cal_centro_symmetry_parameter(12)
        s.cal_ackland_jones_analysis()
        s.cal_common_neighbor_parameter(3.6)
        s.cal_structure_entropy(4.0, 0.2, use_local_density=True, average_rc=3.2)
        s.cal_atomic_temperature(4.0)
        s.cal_steinhardt_bond_orientation([4, 6], rc=3.3, wl=True, wlhat=True, average=True)
        s.average_by_neighbor(3.4, "csp")
        g = s.cal_radial_distribution_function(4.5, nbin=40)
        w = s.cal_warren_cowley_parameter(3.4)
        s.cal_polyhedral_template_matching("fcc-hcp-bcc", return_rmsd=True, return_ordering=True, identify_fcc_planar_faults=True)
        s.cal_cluster_analysis(2.7)                 # numbering depends on the atom order: runs on the translated list
        s.cal_identify_diamond_structure()
        s.cal_steinhardt_bond_orientation([6], nnn=12, identify_liquid=True)
        out[mode] = (s, cna_adaptive, g, w)
    (a, ca, ga, wa), (b, cb, gb, wb) = out["0"], out["1"]
    assert a._spatial() is None and b._spatial() is not None
    assert np.array_equal(ca, cb)
    assert set(a.data.columns) == set(b.data.columns)
    _same_columns(a, b, [c for c in a.data.columns])
    assert np.array_equal(ga.g_total, gb.g_total) and set(ga.g_partial) == set(gb.g_partial)
    assert all(np.array_equal(ga.g_partial[k], gb.g_partial[k]) for k in ga.g_partial)
    assert np.array_equal(wa.WCP, wb.WCP)
    assert a.cluster_number == b.cluster_number
    assert np.array_equal(as_numpy(a.ptm_indices), as_numpy(b.ptm_indices))
    assert np.array_equal(as_numpy(a.verlet_list), as_numpy(b.verlet_list))


def test_user_weight_rows_keep_the_steinhardt_call_off_the_twin(oracle_backend, monkeypatch):
    """cal_steinhardt_bond_orientation(use_weight=True, weight=<array>): the weight rows line up with THIS system's list rows,
    which the twin holds permuted — the call must run in the system's own order: twin == plain bit for bit"""
    out = {}
    for mode in ("0", "1"):
        s = _system(monkeypatch, mode)
        s.build_neighbor(3.3, max_neigh=20)
        rows = as_numpy(s.verlet_list)
        w = np.where(rows >= 0, 1.0 + (rows % 7) * 0.25, 0.0)  # a weight that depends on the NEIGHBOUR's number: any row mix-up shows
        assert s._twin_for("cal_steinhardt_bond_orientation", ([4, 6],), dict(rc=3.3, use_weight=True, weight=w)) is None
        s.cal_steinhardt_bond_orientation([4, 6], rc=3.3, use_weight=True, weight=w)
        out[mode] = s
    _same_columns(out["0"], out["1"], ["ql4", "ql6"])
    assert out["1"]._spatial() is not None


def test_twin_follows_data_and_box_changes(oracle_backend, monkeypatch):
    s = _system(monkeypatch, "1", with_types=True)
    s.cal_centro_symmetry_parameter(12)
    first = s._spatial()
    assert first is not None
    # new per-atom columns reach the twin through the permutation
    s.update_data(s.data.with_columns(score=np.arange(s.N, dtype=np.float64)))
    s.average_by_neighbor(3.4, "score")
    assert s._spatial() is first
    ref = _system(monkeypatch, "0", with_types=True)
    ref.update_data(ref.data.with_columns(score=np.arange(ref.N, dtype=np.float64)))
    ref.average_by_neighbor(3.4, "score")
    assert np.array_equal(ref.data["score_ave"].to_numpy(), s.data["score_ave"].to_numpy())
    # forgetting the list forgets the twin's
    s.update_data(s.data, reset_neighbor=True)
    assert "verlet_list" not in s.__dict__ and "verlet_list" not in first.__dict__
    # a new box: a new twin; moved atoms: a new twin
    s.box = mp.Box(s.box.box * 1.0)
    s.build_neighbor(3.3)
    second = s._spatial()
    assert second is not None and second is not first
    s.wrap_pos()
    s.build_neighbor(3.3)
    assert s._spatial() is not second
    # a list the user put there himself is not the twin's: the plain path takes over
    s.verlet_list = as_numpy(s.verlet_list).copy()
    assert s._twin_for("cal_common_neighbor_parameter", (3.2,), {}) is None


def test_perfect_lattice_ties_fall_as_in_the_original_numbering(oracle_backend, monkeypatch):
    """a perfect bcc lattice: the twelve nearest of an atom are its eight first neighbours and FOUR of its six second ones — which
    four, the search decides by atom number; the twin's searches carry the original numbers as their tie-breaking key"""
    out = {}
    for mode in ("0", "1"):
        monkeypatch.setenv("MDAPY_SPATIAL_SORT", mode)
        pos, box = lattice_positions("bcc", 3.2, 6, 5, 5)
        pos = pos[np.random.default_rng(2).permutation(len(pos))]
        s = mp.System(pos=pos, box=box)
        s.cal_steinhardt_bond_orientation([4, 6], nnn=12)
        s.cal_centro_symmetry_parameter(8)
        s.build_nearest_neighbor(12)
        out[mode] = (s, as_numpy(s.verlet_list).copy())
    assert out["0"][0]._spatial() is None and out["1"][0]._spatial() is not None
    assert np.array_equal(out["0"][1], out["1"][1])
    _same_columns(out["0"][0], out["1"][0], ["ql4", "ql6", "csp"])


# ------------------------------------------------------------------------------------------------------------------------------
# Trajectories: the permutation of the last sorted System is carried to the next one (_twin.py _last / _sorted_as_last_time).
# The oracle backend's order statistic restates mdh_order_statistic, so the decision "read through the old permutation or sort
# afresh" is the one the HIP path takes; tests/test_gpu_sequences.py runs the same sequences on the kernels.
# ------------------------------------------------------------------------------------------------------------------------------
import _trajectory as T

RC_CNA = 0.854 * 3.615
SEQUENCES = {  # steps, and for every frame: "sort" (a fresh permutation), "reuse" (the previous twin's) or "none" (no twin)
    "drift_drift": (["drift", "drift"], ["sort", "reuse", "reuse"]),
    "drift_renumber_drift": (["drift", "renumber", "drift"], ["sort", "reuse", "sort", "reuse"]),
    "resize": (["resize"], ["sort", "sort"]),
    "reshape": (["reshape"], ["sort", "reuse"]),
    "repbc": (["repbc"], ["sort", "sort"]),
    "drift_nan_drift": (["drift", "nan_atom", "drift"], ["sort", "reuse", "none", "none"]),  # (the NaN stays in the last frame)
}


def _run_sequence(frames, analyse):
    """one System per frame, as a trajectory loop makes them -> per frame (what happened to the permutation, results or None)"""
    from mdapy_amd import _twin as twin_mod

    twin_mod.forget_order()
    out, last = [], None
    for f in frames:
        s = mp.System(pos=f.pos, box=mp.Box(f.box, boundary=[int(b) for b in f.boundary], origin=f.origin))
        twin = s._spatial()
        if twin is None:
            out.append(("none", None))
            continue
        perm = np.asarray(as_numpy(twin._perm))
        assert sorted(perm.tolist()) == list(range(f.n))
        how = "reuse" if last is not None and twin._perm is last else "sort"
        last = twin._perm
        res = None
        if analyse:
            s.cal_common_neighbor_analysis(rc=RC_CNA)
            res = {"cna": s.data["cna"].to_numpy().copy(), "rows": as_numpy(s.verlet_list).copy(), "dist": as_numpy(s.distance_list).copy(),
                   "counts": as_numpy(s.neighbor_number).copy()}
            s.cal_centro_symmetry_parameter(12)
            res["csp"] = s.data["csp"].to_numpy().copy()
        out.append((how, res))
    return out


@pytest.mark.parametrize("name", list(SEQUENCES))
def test_frames_of_a_trajectory_equal_the_oracle_whichever_permutation_they_are_read_through(oracle_backend, monkeypatch, name):
    """every frame of a sequence — analysed on a twin read through the PREVIOUS frame's permutation where system.py decides so —
    gives the lists, labels and centro-symmetry values the oracle computes from that frame alone, and what the same sequence gives
    with MDAPY_REUSE_ORDER=0 (every frame sorted).  Which frames reused the permutation is asserted: a run that sorts everywhere
    fails.  A frame with an absent atom (x = NaN) gets no twin, first frame or not (its analyses are left to the GPU test: the
    oracle's cell build, like the reference's, is not defined for a NaN)."""
    monkeypatch.setenv("MDAPY_SPATIAL_SORT", "1")
    steps, want = SEQUENCES[name]
    frames = T.sequence(T.start("fcc", (11, 11, 11), seed=21, rattle=0.10), steps, seed=22)  # (four 64-atom bins per axis: a shuffled order shows)
    got = _run_sequence(frames, analyse=True)
    assert [g[0] for g in got] == want
    monkeypatch.setenv("MDAPY_REUSE_ORDER", "0")
    sorted_everywhere = _run_sequence(frames, analyse=True)
    assert [g[0] for g in sorted_everywhere] == [w if w == "none" else "sort" for w in want]
    for f, (how, res), (_, res0) in zip(frames, got, sorted_everywhere):
        if how == "none":
            assert not T.finite(f).all()
            continue
        e = T.expected_cutoff(f, RC_CNA)
        k = T.expected_knn(f, 12, csp=12)
        for key in ("rows", "dist", "counts", "cna"):
            assert np.array_equal(res[key], e[key]), (name, how, key)
        assert np.array_equal(res["csp"], k["csp"]), (name, how)
        for key in res:
            assert np.array_equal(res[key], res0[key]), (name, how, key, "MDAPY_REUSE_ORDER=0")


def test_order_statistic_of_the_oracle_backend_tells_a_spatial_order_from_a_shuffled_one(oracle_backend):
    """the numpy restatement of mdh_order_statistic: ~0 for a lattice builder's order and for the stand-in sort's, ~1 shuffled, and a
    NaN is a bin-0 atom, not an error (include/mdapy_amd.h, "atom order")"""
    import mdapy_amd.kernels as K
    from mdapy_amd.system import SORT_FAR_FRACTION

    f = T.start("fcc", (16, 16, 16), seed=5, shuffle=False)  # (six bins per axis)
    g = T.renumber(f, np.random.default_rng(6))
    assert K.order.order_statistic(*f.where()) < 0.05 < SORT_FAR_FRACTION < 0.7 < K.order.order_statistic(*g.where())
    xs, ys, zs, perm, n = K.order.spatial_sort(*g.where())
    assert n == g.n and K.order.order_statistic(xs, ys, zs, g.box, g.origin, g.boundary) < SORT_FAR_FRACTION
    h = T.nan_atom(g, np.random.default_rng(7))
    assert K.order.spatial_sort(*h.where())[4] == h.n - 1
    assert 0.7 < K.order.order_statistic(*h.where()) <= 1.0


# ------------------------------------------------------------------------------------------------------------------------------
# The state between a System and its twin is one object (mdapy_amd/_twin.py): its edges, the names the decorator binds, and the
# remembered permutation as one record.
# ------------------------------------------------------------------------------------------------------------------------------
def test_edges_between_a_system_and_its_twin_in_one_sequence(oracle_backend, monkeypatch):
    """tests/_twin_walk.py: build, sort the front, ADF, a k-nearest list beside a stale rc, a user's list, a forgotten list, a new
    box, removed atoms — twin against plain bit for bit after every step, with which side ran and ``_listed_on_twin`` asserted"""
    import _twin_walk

    oracle_backend.install_consumers(monkeypatch)
    _twin_walk.walk()


def test_the_decorator_binds_the_functions_own_positional_names(oracle_backend, monkeypatch):
    """``_on_twin`` reads the positional parameter names off the function it wraps; ``_twin_for`` decides the same for a positional, a
    keyword and a mixed spelling of a call.  ``cal_chill_plus(3.5)`` and ``cal_structure_entropy(4.0, 0.2, False, 3.2)`` run on the
    twin in every box that has one (a box thinner than their two cutoffs, 7 and 8 A, is below the 15 A under which there is no twin
    at all).  The decision "no twin" that hangs on finding the reach under its name is therefore taken with 9.5 A in their place: two
    cutoffs are more than the 18.08 A of the thin box and less than the 21.69 A of the wide one."""
    import inspect

    from mdapy_amd.system import _NAMES, System

    wrapped = {name for name, member in vars(System).items() if hasattr(member, "__wrapped__")}
    assert wrapped == set(_NAMES) and len(wrapped) == 15
    for name in wrapped:
        params = list(inspect.signature(getattr(System, name).__wrapped__).parameters.values())[1:]
        assert all(q.kind is q.POSITIONAL_OR_KEYWORD for q in params), name
        assert _NAMES[name] == tuple(q.name for q in params), name
    wide = _system(monkeypatch, "1")                   # 25.31 x 21.69 x 21.69 A
    thin = _system(monkeypatch, "1", cells=(7, 6, 5))  # 18.08 A across z
    assert wide._spatial() is not None and thin._spatial() is not None

    def decisions(s, name, args):
        """positional, keyword, and first-positional-rest-keyword spelling -> whether each may run on the twin"""
        named = dict(zip(_NAMES[name], args))
        rest = {k: v for k, v in list(named.items())[1:]}
        got = [s._twin_for(name, args, {}), s._twin_for(name, (), named), s._twin_for(name, args[:1], rest)]
        assert all(g is None or g is s._spatial() for g in got)
        return [g is not None for g in got]

    for reach, on_wide, on_thin in ((None, True, True), (9.5, True, False)):
        for name, args in (("cal_chill_plus", (3.5,)), ("cal_structure_entropy", (4.0, 0.2, False, 3.2)), ("average_by_neighbor", (3.4, "x"))):
            if reach is not None:
                args = (reach,) + args[1:]
            assert decisions(wide, name, args) == [on_wide] * 3, (name, args)
            assert decisions(thin, name, args) == [on_thin] * 3, (name, args)
    # the reach is found behind other arguments too, and an argument that was not passed is not read (no defaults: no reach)
    assert thin._twin_for("cal_steinhardt_bond_orientation", ([6], False, 0, 9.5), {}) is None
    assert thin._twin_for("cal_steinhardt_bond_orientation", ([6],), dict(nnn=12, max_neigh=60, threshold=0.6)) is thin._spatial()
    assert thin._twin_for("cal_chill_plus", (), {}) is thin._spatial() and wide._twin_for("cal_chill_plus", (), {}) is wide._spatial()


def test_the_remembered_permutation_is_one_record_replaced_whole(oracle_backend, monkeypatch):
    """after frame A and frame B (another number of atoms; then another pbc) the snapshot a reader takes is wholly A's or wholly
    B's: the record held before the second sort still carries A's fields, and a new one stands in its place"""
    from mdapy_amd import _twin as twin_mod

    twin_mod.forget_order()
    assert twin_mod._last is None
    a = _system(monkeypatch, "1")
    ta = a._spatial()
    rec_a = twin_mod._last
    assert isinstance(rec_a, tuple) and rec_a._fields == ("perm", "n", "pbc", "host")
    assert rec_a.perm is ta._perm and rec_a.n == a.N == 1008 and rec_a.pbc == (1, 1, 1) and rec_a.host is True
    with pytest.raises(AttributeError):
        rec_a.n = 5
    b = _system(monkeypatch, "1", cells=(6, 6, 6))  # another N
    tb = b._spatial()
    rec_b = twin_mod._last
    assert rec_b is not rec_a and (rec_b.perm, rec_b.n, rec_b.pbc) == (tb._perm, 864, (1, 1, 1)) and tb._perm is not ta._perm
    assert rec_a.perm is ta._perm and rec_a.n == 1008 and rec_a.pbc == (1, 1, 1) and len(np.asarray(rec_a.perm)) == rec_a.n
    pos = np.column_stack([b.data[c].to_numpy() for c in "xyz"])
    c = mp.System(pos=pos, box=mp.Box(b.box.box, boundary=[1, 0, 1]))  # the same N, another pbc: sorted afresh
    tc = c._spatial()
    rec_c = twin_mod._last
    assert tc._perm is not tb._perm and rec_c is not rec_b and (rec_c.perm, rec_c.n, rec_c.pbc) == (tc._perm, 864, (1, 0, 1))
    assert (rec_b.perm, rec_b.n, rec_b.pbc) == (tb._perm, 864, (1, 1, 1))
    for rec in (rec_a, rec_b, rec_c):
        assert len(np.asarray(rec.perm)) == rec.n
    twin_mod.forget_order()
    assert twin_mod._last is None
