"""The trajectory unwrap and ``Trajectory`` without a GPU: the numpy restatement of tests/_unwrap_ref.py against the reference's
formulation and against walks whose true path is known; ``unwrap_trajectory`` with that restatement installed as
``kernels.unwrap``; ``Trajectory`` — its list interface and its readers on the files of tests/golden/trajectory.

Bound on ``unwrapped``, with u = 2^-53, p the wrapped position and s the shift: ``8 u (|p_d| + sum_k |s_k| |cell[k][d]|)``.
Derived, not measured: either side takes three products and three sums to one entry, each with a relative error of at most u on
a quantity no larger than the bracket, in any order and with any fusing; both sides, doubled for higher-order terms.  Equal
integer shifts are demanded of two formulations that round ``frac`` differently, which is fair only while no step lies at a
half-integer: every input's steps are asserted to keep 1e-6 away from one (by construction they keep 0.2 away: a walk's step is
shorter than 0.245 of the shortest cell height).

The ground-truth tests use the "dyadic" cells of _unwrap_ref.cells_of — entries that are small binary fractions — so that
taking whole cells off a position and putting them back are exact but for the final subtraction and addition (at most
u (|walk_d| + |p_d| + |unwrapped_d|) in all, inside the bound); with a general cell the wrap that makes the input would bring
rounding of its own, of the size of frame 0's offset, which the bound does not know about."""
import gzip
import os
import shutil
import warnings

import numpy as np
import pytest

import _unwrap_ref as R
import mdapy_amd as mp
from mdapy_amd import _unwrap, trajectory, unwrap_trajectory as unwrap_module  # noqa: F401  (what this file is about)

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "trajectory")
BOXES = ("cubic", "sheared", "npt")


@pytest.fixture
def restated(monkeypatch):
    import mdapy_amd.kernels as K

    monkeypatch.setattr(K, "unwrap", R)
    return R


# ---- the restatement
def _reference_formulation(pos, cells, pbc, image=None):
    """src/mdapy/unwrap_trajectory.py:212-255 in its own words: ``pos @ inv``, ``np.round``, ``pos + shift.astype(float) @ cell``"""
    F, N = pos.shape[:2]
    out, shifts = np.empty((F, N, 3)), np.zeros((F, N, 3), np.int64)
    if image is not None:
        for f in range(F):
            shifts[f] = image[f].astype(np.int64)
            out[f] = pos[f] + shifts[f].astype(np.float64) @ cells[f]
        return out, shifts
    shift = np.zeros((N, 3), np.int64)
    frac_prev = pos[0] @ np.linalg.inv(cells[0])
    out[0] = pos[0]
    for f in range(1, F):
        frac = pos[f] @ np.linalg.inv(cells[f])
        for d in range(3):
            if pbc[d]:
                shift[:, d] += np.round(frac_prev[:, d] - frac[:, d]).astype(np.int64)
        out[f] = pos[f] + shift.astype(np.float64) @ cells[f]
        shifts[f] = shift
        frac_prev = frac
    return out, shifts


@pytest.mark.parametrize("pbc", [(1, 1, 1), (1, 0, 1)])
@pytest.mark.parametrize("kind", BOXES)
def test_restatement_against_the_reference_formulation(kind, pbc):
    F, N = 35, 70
    walk, wrapped, n, cells = R.case(kind, F, N)
    gap = R.margin(wrapped, cells)
    print(f"{kind}: every step keeps {gap:.3f} from a half-integer (needed 1e-6)")
    assert gap >= 1e-6
    for image in (None, n.astype(np.int32)):
        got, shifts = R.restate(wrapped, cells, pbc, image=image)
        want, want_shifts = _reference_formulation(wrapped, cells, pbc, image)
        assert np.array_equal(shifts, want_shifts)
        allowed = R.bound(wrapped, shifts, cells)
        off = np.abs(got - want)
        print(f"{kind} pbc {pbc} {'image' if image is not None else 'min_image'}: worst error {float((off / allowed).max()) * 8:.2f} u (|p| + |s||cell|) (allowed 8), "
              f"{int(np.abs(shifts).max())} cells the largest shift")
        assert np.all(off <= allowed)
        if image is None:
            assert shifts[:, :, 1].any() == bool(pbc[1]), "an open axis is left alone, a periodic one is crossed"
            if kind == "cubic":  # (in a sheared cell a shift along c moves y as well)
                assert np.array_equal(got[:, :, 1], wrapped[:, :, 1]) == (not pbc[1])
    # the same through row_of: a stored order that differs in every frame
    row_of = R.permutations(F, N, 5)
    stored = np.empty_like(wrapped)
    stored[np.arange(F)[:, None], row_of] = wrapped
    plain = R.restate(wrapped, cells, pbc)
    through = R.restate(stored, cells, pbc, row_of=row_of)
    assert np.array_equal(plain[0], through[0]) and np.array_equal(plain[1], through[1])
    stored_n = np.empty_like(n)
    stored_n[np.arange(F)[:, None], row_of] = n
    by_image = R.restate(stored, cells, pbc, row_of=row_of, image=stored_n.astype(np.int32))
    assert np.array_equal(by_image[1], n)


@pytest.mark.parametrize("kind", ["dyadic_cubic", "dyadic_sheared", "dyadic_npt"])
def test_restatement_recovers_a_known_walk(kind):
    F, N = 35, 70
    walk, wrapped, n, cells = R.case(kind, F, N)
    assert R.margin(wrapped, cells) >= 1e-6
    got, shifts = R.restate(wrapped, cells, (1, 1, 1))
    assert np.array_equal(shifts, n - n[0]), "the shifts are the boundary crossings since frame 0"
    offset = np.einsum("nk,fkd->fnd", n[0].astype(np.float64), cells)  # frame 0's own wrap, in every frame's cell
    assert n[0].any() and offset.any()
    allowed = R.bound(wrapped, shifts, cells)
    off = np.abs(got - (walk - offset))
    print(f"{kind}: worst error {float((off / allowed).max()) * 8:.2f} u (|p| + |s||cell|) (allowed 8)")
    assert np.all(off <= allowed)
    crossings = np.diff(shifts[:, :, 0], axis=0)
    assert (crossings > 0).any() and (crossings < 0).any(), "crossings in both directions"
    assert (np.abs(shifts[-1, :, 0]) >= 2).any(), "several crossings of one atom"
    # an open axis is left alone
    open_y, open_shifts = R.restate(wrapped, cells, (1, 0, 1))
    assert not open_shifts[:, :, 1].any() and np.array_equal(open_shifts[:, :, 0], shifts[:, :, 0])
    if kind == "dyadic_cubic":
        assert np.array_equal(open_y[:, :, 1], wrapped[:, :, 1])


def test_restatement_refuses_what_is_not_finite():
    walk, wrapped, n, cells = R.case("cubic", 3, 4)
    bad = np.array(wrapped)
    bad[1, 2, 0] = np.nan
    with pytest.raises(ValueError, match="not finite"):
        R.restate(bad, cells, (1, 1, 1))


# ---- unwrap_trajectory with the restatement installed
def _system(cols, cell, boundary=(1, 1, 1)):
    return mp.System(data=mp.Frame(cols), box=mp.Box(np.asarray(cell, dtype=np.float64), list(boundary)))


def _xyz(s):
    return np.column_stack([s.data[c].to_numpy() for c in "xyz"])


def _frames(wrapped, cells, ids=None, extra=None, boundary=(1, 1, 1)):
    out = []
    for f in range(len(wrapped)):
        cols = {} if ids is None else {"id": ids[f]}
        cols.update({c: wrapped[f, :, d] for d, c in enumerate("xyz")})
        cols.update({k: v[f] for k, v in (extra or {}).items()})
        out.append(_system(cols, cells[f], boundary))
    return out


def test_method_choice(restated):
    walk, wrapped, n, cells = R.case("npt", 6, 9)
    want, _ = R.restate(wrapped, cells, (1, 1, 1))
    plain = mp.unwrap_trajectory(mp.Trajectory(systems=_frames(wrapped, cells)))
    assert isinstance(plain, mp.Trajectory) and plain._unwrap_method == "min_image" and len(plain) == 6
    assert np.array_equal(plain.positions(), want) and all(np.array_equal(_xyz(s), want[f]) for f, s in enumerate(plain))
    assert plain[3].data.columns == ["x", "y", "z"] and np.array_equal(plain[3].box.box, cells[3])
    # image flags, every frame with its own cell
    flags = {c: n[:, :, d].astype(np.int32) for d, c in enumerate(("ix", "iy", "iz"))}
    by_image = mp.Trajectory(systems=_frames(wrapped, cells, extra=flags)).unwrap()
    assert by_image._unwrap_method == "image"
    want_image, _ = R.restate(wrapped, cells, (1, 1, 1), image=n.astype(np.int32))
    assert np.array_equal(by_image.positions(), want_image)
    assert np.all(np.abs(want_image - walk) <= R.bound(wrapped, n, cells) + 8 * R.U * np.abs(walk))
    assert by_image[0].data.columns == ["x", "y", "z"]
    # xu yu zu come first, whatever else there is
    unwrapped = {c: walk[:, :, d] for d, c in enumerate(("xu", "yu", "zu"))}
    unwrapped.update(flags)
    given = mp.unwrap_trajectory(mp.Trajectory(systems=_frames(wrapped, cells, extra=unwrapped)))
    assert given._unwrap_method == "unwrapped" and np.array_equal(given.positions(), walk)
    assert np.array_equal(_xyz(given[4]), walk[4]) and given[4].data.columns == ["x", "y", "z"]


def test_rows_follow_the_ids(restated):
    F, N = 6, 9
    walk, wrapped, n, cells = R.case("sheared", F, N)  # row i: the atom with the i-th smallest id
    want, _ = R.restate(wrapped, cells, (1, 1, 1))
    row_of = R.permutations(F, N, 3)
    ids = np.array([2, 3, 5, 7, 11, 13, 17, 19, 23], np.int32)
    stored = np.empty_like(wrapped)
    stored_ids = np.empty((F, N), np.int32)
    for f in range(F):
        stored[f, row_of[f]] = wrapped[f]
        stored_ids[f, row_of[f]] = ids
    types = stored_ids % 3
    names = np.where(stored_ids % 2 == 1, "Cu", "Al").astype(object)
    assert not np.array_equal(stored_ids[0], ids), "frame 0's ids are not in order"
    assert any(not np.array_equal(stored_ids[f], stored_ids[0]) for f in range(1, F)), "the frames list the atoms differently"
    frames = _frames(stored, cells, ids=stored_ids, extra={"type": types, "element": names, "vx": stored[:, :, 0]})
    got = mp.Trajectory(systems=frames).unwrap()
    assert got._unwrap_method == "min_image"
    assert np.array_equal(got.positions(), want)
    for f, s in enumerate(got):
        assert s.data.columns == ["id", "type", "element", "x", "y", "z"], "what frame 0 carried of id, type, element; nothing else"
        assert np.array_equal(s.data["id"].to_numpy(), ids) and np.array_equal(s.data["type"].to_numpy(), ids % 3)
        assert list(s.data["element"].to_numpy()) == ["Cu" if i % 2 else "Al" for i in ids]
        assert np.array_equal(_xyz(s), want[f]) and np.array_equal(s.box.box, cells[f])


def test_what_is_refused(restated):
    walk, wrapped, n, cells = R.case("cubic", 3, 4)
    ids = np.tile(np.arange(1, 5, dtype=np.int32), (3, 1))
    with pytest.raises(ValueError, match="trajectory has no frames"):
        mp.unwrap_trajectory(mp.Trajectory(systems=[]))
    empty = _system({c: np.zeros(0) for c in "xyz"}, cells[0])
    with pytest.raises(ValueError, match="frames contain no atoms"):
        mp.Trajectory(systems=[empty]).unwrap()
    frames = _frames(wrapped, cells, ids=ids)
    frames[2] = _system({"id": ids[0][:3], **{c: wrapped[2, :3, d] for d, c in enumerate("xyz")}}, cells[2])
    with pytest.raises(ValueError, match="frame 0 has 4, frame 2 has 3"):
        mp.Trajectory(systems=frames).unwrap()
    twice = ids.copy()
    twice[0, 1] = twice[0, 0]
    with pytest.raises(ValueError, match="'id' column in frame 0 contains duplicates"):
        mp.Trajectory(systems=_frames(wrapped, cells, ids=twice)).unwrap()
    frames = _frames(wrapped, cells, ids=ids)
    frames[1] = _frames(wrapped, cells)[1]
    with pytest.raises(ValueError, match="frame 1 is missing the 'id' column that frame 0 carries"):
        mp.Trajectory(systems=frames).unwrap()
    other = ids.copy()
    other[2, 3] = 99
    with pytest.raises(ValueError, match="frame 2 has a different id set from frame 0"):
        mp.Trajectory(systems=_frames(wrapped, cells, ids=other)).unwrap()


def test_warnings_fire_once(restated):
    F = 5
    walk, wrapped, n, cells = R.case("cubic", F, 4)
    frames = _frames(wrapped, cells)
    for f in (2, 3):
        frames[f] = _system({c: wrapped[f, :, d] for d, c in enumerate("xyz")}, cells[f], (1, 0, 1))
    with pytest.warns(RuntimeWarning, match="PBC flags change between frame 0") as seen:
        got = mp.Trajectory(systems=frames).unwrap()
    assert len([w for w in seen if "PBC flags" in str(w.message)]) == 1
    assert np.array_equal(got.positions(), R.restate(wrapped, cells, (1, 1, 1))[0]), "frame 0's flags are used throughout"
    # a LAMMPS cell flip: the tilt xy jumps by a whole edge, twice; one warning, and none in image mode
    flipped = np.array(cells)
    flipped[2:, 1, 0] = 9.0
    flipped[4:, 1, 0] = -1.0
    with pytest.warns(RuntimeWarning, match="possible LAMMPS triclinic cell flip between frame 1 and frame 2") as seen:
        mp.Trajectory(systems=_frames(wrapped, flipped)).unwrap()
    assert len([w for w in seen if "cell flip" in str(w.message)]) == 1
    flags = {c: n[:, :, d].astype(np.int32) for d, c in enumerate(("ix", "iy", "iz"))}
    with warnings.catch_warnings():
        warnings.simplefilter("error")
        mp.Trajectory(systems=_frames(wrapped, flipped, extra=flags)).unwrap()
        mp.Trajectory(systems=_frames(wrapped, cells)).unwrap()


# ---- the shim and the library, before any device work
def test_shim_checks_arguments_without_the_library():
    from mdapy_amd import kernels

    shim = kernels.unwrap
    assert shim.__name__ == "mdapy_amd._unwrap" and "unwrap" not in kernels.NAMES
    pos, cells, out = np.zeros((3, 4, 3)), np.repeat(np.eye(3)[None], 3, axis=0), np.zeros((3, 4, 3))
    for bad in (np.zeros((3, 4)), np.zeros((3, 4, 2)), np.zeros((0, 4, 3)), np.zeros((3, 0, 3))):
        with pytest.raises(ValueError, match="pos has shape"):
            shim.unwrap(bad, cells, (1, 1, 1), out)
    with pytest.raises(ValueError, match="cells has shape"):
        shim.unwrap(pos, cells[:2], (1, 1, 1), out)
    with pytest.raises(ValueError, match="pbc has shape"):
        shim.unwrap(pos, cells, (1, 1), out)
    with pytest.raises(ValueError, match="unwrapped has shape"):
        shim.unwrap(pos, cells, (1, 1, 1), np.zeros((3, 5, 3)))
    with pytest.raises(ValueError, match="unwrapped has shape"):
        shim.unwrap(pos, cells, (1, 1, 1), None)
    with pytest.raises(ValueError, match="row_of has shape"):
        shim.unwrap(pos, cells, (1, 1, 1), out, row_of=np.zeros((3, 5), np.int64))
    with pytest.raises(ValueError, match="image has shape"):
        shim.unwrap(pos, cells, (1, 1, 1), out, image=np.zeros((3, 4), np.int32))
    with pytest.raises(ValueError, match="shifts has shape"):
        shim.unwrap(pos, cells, (1, 1, 1), out, shifts=np.zeros((2, 4, 3), np.int64))
    with pytest.raises(ValueError, match="chunks"):
        shim.unwrap(pos, cells, (1, 1, 1), out, chunks=-1)
    flat = np.array(cells)
    flat[1] = [[1.0, 1.0, 0.0], [2.0, 2.0, 0.0], [0.0, 0.0, 1.0]]
    with pytest.raises(ValueError, match="cell of frame 1 is singular"):
        shim.unwrap(pos, flat, (1, 1, 1), out)


def test_library_checks_arguments_before_any_device_work():
    from mdapy_amd import _lib, kernels

    L = _lib.lib()
    pos, cells, out = np.zeros((3, 4, 3)), np.ascontiguousarray(np.repeat(np.eye(3)[None], 3, axis=0)), np.zeros((3, 4, 3))
    pbc = np.ones(3, np.int32)
    image = np.zeros((3, 4, 3), np.int32)
    p, c, o, b, im = pos.ctypes.data, cells.ctypes.data, out.ctypes.data, pbc.ctypes.data, image.ctypes.data

    def call(pos=p, image=None, cell=c, inv=c, pbc=b, F=3, N=4, chunks=0, out=o):
        return L.mdh_unwrap_trajectory(pos, None, image, cell, inv, pbc, F, N, chunks, out, None, _lib.HOST, None)

    assert call(pos=None) == _lib.ERR_ARG and call(cell=None) == _lib.ERR_ARG and call(pbc=None) == _lib.ERR_ARG
    assert call(out=None) == _lib.ERR_ARG and call(inv=None) == _lib.ERR_ARG
    assert call(F=0) == _lib.ERR_ARG and call(N=0) == _lib.ERR_ARG and call(chunks=-1) == _lib.ERR_ARG
    assert call(F=(1 << 24) + 1) == _lib.ERR_ARG and call(N=(1 << 28) + 1) == _lib.ERR_ARG
    assert call(F=1 << 24, N=1 << 28, chunks=1 << 24) == _lib.ERR_ARG, "atoms x chunks beyond one launch"
    with pytest.raises(ValueError, match="chunks is negative"):
        _lib.check(call(chunks=-1))
    if _lib.device_count() > 0:
        return  # (with a device the valid calls compute: test_gpu_unwrap.py)
    assert call(image=im, inv=None) == _lib.ERR_HIP, "image mode needs no inverse; without a device the library says so"
    with pytest.raises(RuntimeError, match="HIP error"):
        kernels.unwrap.unwrap(pos, cells, pbc, out)


# ---- Trajectory
def _one(k):
    return mp.System(pos=np.full((k + 1, 3), float(k)), box=10.0)


def test_list_interface():
    assert mp.Trajectory is trajectory.Trajectory and {"Trajectory", "unwrap_trajectory"} <= set(mp.__all__)
    with pytest.raises(ValueError, match="Trajectory needs either filename= or systems="):
        mp.Trajectory()
    systems = [_one(k) for k in range(5)]
    traj = mp.Trajectory(systems=systems, verbose=False)
    assert len(traj) == 5 and list(traj) == systems and repr(traj) == "<Trajectory: 5 frame(s)>"
    counts = traj.get_atoms_count()
    assert isinstance(counts, np.ndarray) and counts.dtype == np.int64 and counts.tolist() == [1, 2, 3, 4, 5]
    assert traj[2] is systems[2] and traj[-1] is systems[4]
    part = traj[1:4]
    assert isinstance(part, mp.Trajectory) and list(part) == systems[1:4]
    assert list(traj[[0, -1, 2]]) == [systems[0], systems[4], systems[2]]
    assert list(traj[np.array([-5, 4])]) == [systems[0], systems[4]] and list(traj[(1, 3)]) == [systems[1], systems[3]]
    for bad in ([5], [-6], np.array([0, 7])):
        with pytest.raises(IndexError, match="out of bounds"):
            traj[bad]
    assert list(traj[counts > 3]) == systems[3:]
    with pytest.raises(IndexError, match="boolean mask must have length 5"):
        traj[np.array([True, False])]
    with pytest.raises(TypeError, match="bool or integer"):
        traj[np.array([0.5])]
    extra = _one(7)
    traj[1] = extra
    assert traj[1] is extra
    with pytest.raises(TypeError):
        traj[1] = "a frame"
    traj.append(systems[1])
    traj.extend([_one(8), _one(9)])
    assert len(traj) == 8 and traj.get_atoms_count().tolist() == [1, 8, 3, 4, 5, 2, 9, 10]
    traj.insert(0, extra)
    assert traj[0] is extra and len(traj) == 9
    for call in (traj.append, lambda s: traj.insert(0, s)):
        with pytest.raises(TypeError):
            call(3)
    assert traj.pop() .N == 10 and traj.pop(0) is extra and len(traj) == 7
    traj.remove([0, 2])
    assert traj.get_atoms_count().tolist() == [8, 4, 5, 2, 9]
    traj.remove(1)
    assert traj.get_atoms_count().tolist() == [8, 5, 2, 9]
    both = traj.concatenate(part)
    assert isinstance(both, mp.Trajectory) and len(both) == 7 and list(both)[4:] == systems[1:4] and len(traj) == 4
    assert systems[0] is not None and len(mp.Trajectory(systems=systems)) == 5, "the list given is copied, not kept"


def test_positions():
    same = mp.Trajectory(systems=[mp.System(pos=np.arange(12.0).reshape(4, 3) + k, box=20.0) for k in range(3)])
    pos = same.positions()
    assert isinstance(pos, np.ndarray) and pos.dtype == np.float64 and pos.shape == (3, 4, 3)
    assert np.array_equal(pos[2], np.arange(12.0).reshape(4, 3) + 2)
    with pytest.raises(ValueError, match="frame 0 has 1, frame 1 has 2"):
        mp.Trajectory(systems=[_one(0), _one(1)]).positions()


def test_format_inference(tmp_path):
    infer = trajectory._infer_format
    assert [infer(n) for n in ("a.xyz", "a.EXTXYZ", "b.xyz.gz", "b.extxyz.gz")] == ["xyz"] * 4
    assert [infer(n) for n in ("a.dump", "a.lammpstrj", "a.trj", "a.dump.gz", "a.lammpstrj.gz", "A.TRJ.GZ")] == ["dump"] * 6
    for name in ("a.data", "a.gz", "dump"):
        with pytest.raises(ValueError, match="Cannot infer trajectory format"):
            infer(name)
    with pytest.raises(ValueError, match="Cannot infer trajectory format"):
        mp.Trajectory(str(tmp_path / "frames.txt"))
    with pytest.raises(ValueError, match="Unsupported trajectory format"):
        mp.Trajectory(os.path.join(GOLDEN, "dump_multiframe.dump"), format="poscar")
    with pytest.raises(ValueError, match="fast_mode is not supported for LAMMPS dump format"):
        mp.Trajectory(os.path.join(GOLDEN, "dump_multiframe.dump"), fast_mode=True)
    named = tmp_path / "frames.txt"
    shutil.copy(os.path.join(GOLDEN, "dump_multiframe.dump"), named)
    assert len(mp.Trajectory(str(named), format="dump")) == 2


def test_golden_dumps(tmp_path):
    two = mp.Trajectory(os.path.join(GOLDEN, "dump_multiframe.dump"), verbose=False)
    assert len(two) == 2 and [s.global_info["timestep"] for s in two] == [0, 1] and two.get_atoms_count().tolist() == [2, 2]
    assert two[0].data["x"].to_numpy().tolist() == [0.0, 2.0] and two[1].data["x"].to_numpy().tolist() == [0.1, 2.1]
    assert two[0].data.columns == ["x", "y", "z", "id", "type"] and two[1].data["id"].to_numpy().tolist() == [1, 2]
    assert np.array_equal(two[1].box.box, np.diag([4.0, 4.0, 4.0])) and list(two[1].box.boundary) == [1, 1, 1]
    five = mp.Trajectory(os.path.join(GOLDEN, "dump_multiframe_5x8.dump"))
    assert len(five) == 5 and five.get_atoms_count().tolist() == [8] * 5
    assert [s.global_info["timestep"] for s in five] == [0, 100, 200, 300, 400]
    assert "vx" in five[4].data.columns and five.positions().shape == (5, 8, 3)
    spaced = mp.Trajectory(os.path.join(GOLDEN, "dump_multispace_2frames.dump"))
    assert len(spaced) == 2 and spaced.get_atoms_count().tolist() == [3, 3]
    assert spaced[1].data["x"].to_numpy().tolist() == [0.1, 2.6, 0.0] and spaced[1].data["y"].to_numpy().tolist() == [0.0, 0.0, 2.6]
    # one frame gives one frame, and the single-frame reader gives the same frame
    single = mp.Trajectory(os.path.join(GOLDEN, "dump_image_flags.dump"))
    alone = mp.System(os.path.join(GOLDEN, "dump_image_flags.dump"))
    assert len(single) == 1 and single[0].N == 3 and single[0].data.columns == alone.data.columns
    assert single[0].data["ix"].to_numpy().tolist() == [0, 1, -1] and np.array_equal(single[0].data.to_numpy(), alone.data.to_numpy())
    # compressed, the same
    packed = tmp_path / "five.dump.gz"
    with open(os.path.join(GOLDEN, "dump_multiframe_5x8.dump"), "rb") as src, gzip.open(packed, "wb") as dst:
        dst.write(src.read())
    again = mp.Trajectory(str(packed))
    assert len(again) == 5 and all(np.array_equal(a.data.to_numpy(), b.data.to_numpy()) for a, b in zip(again, five))
    assert [s.global_info["timestep"] for s in again] == [0, 100, 200, 300, 400]
    # the single-frame reader still refuses the file
    from mdapy_amd import load_save

    with pytest.raises(ValueError, match="multi-frame dump file. Use a trajectory reader or split the file first."):
        load_save.read_dump(os.path.join(GOLDEN, "dump_multiframe.dump"))
    with pytest.raises(ValueError, match="no ITEM: TIMESTEP header found"):
        mp.Trajectory(os.path.join(GOLDEN, "mixed_traj.xyz"), format="dump")


def test_golden_dump_unwraps_by_its_image_flags(restated):
    got = mp.Trajectory(os.path.join(GOLDEN, "dump_image_flags.dump")).unwrap()
    assert got._unwrap_method == "image" and got[0].data.columns == ["id", "type", "x", "y", "z"]
    assert got.positions()[0].tolist() == [[0.5, 0.5, 0.5], [6.0, 0.5, 0.5], [-3.5, 2.0, 0.5]]


def test_golden_xyz(tmp_path):
    mixed = mp.Trajectory(os.path.join(GOLDEN, "mixed_traj.xyz"), fast_mode=True)  # (accepted for XYZ: there is one reader)
    assert len(mixed) == 6 and mixed.get_atoms_count().tolist() == [1, 2, 3, 4, 2, 1]
    assert [list(s.box.boundary) for s in mixed] == [[0, 0, 0], [1, 1, 1], [1, 1, 1], [0, 0, 0], [1, 1, 1], [0, 0, 0]]
    assert np.array_equal(mixed[1].box.box, np.diag([10.0] * 3)) and np.array_equal(mixed[2].box.box, np.diag([20.0] * 3))
    assert list(mixed[2].data["element"].to_numpy()) == ["C", "H", "H"] and mixed[2].data["fx"].to_numpy().tolist() == [0.1, -0.05, -0.05]
    assert mixed[2].global_info["energy"] == "-12.34"
    # a classical frame keeps the extent box the single-frame reader gives it
    assert np.allclose(np.diag(mixed[3].box.box), [2.0, 2.0, 1e-9]) and mixed[3].box.origin.tolist() == [-1.0, -1.0, 0.0]
    assert mixed[3].data["x"].to_numpy().tolist() == [-1.0, 1.0, 0.0, 0.0] and list(mixed[4].data["element"].to_numpy()) == ["Cu", "Al"]
    assert mixed[4].data["z"].to_numpy().tolist() == [0.0, 2.5] and list(mixed[5].data["element"].to_numpy()) == ["Ne"]
    with pytest.raises(ValueError, match="frame 0 has 1, frame 1 has 2"):
        mixed.positions()
    spaced = mp.Trajectory(os.path.join(GOLDEN, "mixed_multispace.xyz"))
    assert len(spaced) == 2 and spaced[0].data["x"].to_numpy().tolist() == [0.0, 1.2] and spaced[1].data["x"].to_numpy().tolist() == [0.1, 1.3]
    assert spaced.positions().shape == (2, 2, 3)
    packed = tmp_path / "mixed.xyz.gz"
    with open(os.path.join(GOLDEN, "mixed_traj.xyz"), "rb") as src, gzip.open(packed, "wb") as dst:
        dst.write(src.read())
    again = mp.Trajectory(str(packed))
    assert again.get_atoms_count().tolist() == [1, 2, 3, 4, 2, 1] and again[2].data["fx"].to_numpy().tolist() == [0.1, -0.05, -0.05]
