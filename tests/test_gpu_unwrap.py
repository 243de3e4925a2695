"""The trajectory unwrap on the GPU: the raw ``_unwrap`` shim against the numpy restatement of tests/_unwrap_ref.py, bit for bit,
and ``Trajectory(file).unwrap().positions()`` through to ``MeanSquaredDisplacement``.

Bit equality (``np.array_equal`` on ``unwrapped`` and on ``shifts``) is a fair demand: both sides run the same binary64
operations in the same order with no contraction, on the same inverse cells (``np.linalg.inv`` of the stacked cells on either
side), and the shifts are integers.  The half-integer margin of the steps (test_unwrap_host.py) is asserted on these inputs too.
On the dyadic inputs — box lengths that are powers of two, positions on a 2^-10 grid — every product and sum is exact, so the
unwrapped wrapped-walk IS the walk."""
import numpy as np
import pytest

import _msd_ref
import _unwrap_ref as R
import mdapy_amd as mp
from mdapy_amd._unwrap import AB, T  # atoms per workgroup; chunks = 0 cuts F frames into at most ceil(F / T) runs

pytestmark = pytest.mark.gpu

EDGE_N = (1, AB - 1, AB, AB + 1, 2 * AB + 2)
EDGE_F = (1, 2, 3, T, T + 1, 2 * T + 3)
BIG = (2 * T + 3, 2 * AB + 2)
BOXES = ("cubic", "sheared", "npt")
INT64_MIN = np.iinfo(np.int64).min
EPS = 2.0 ** -53


@pytest.fixture(autouse=True)
def _need_gpu():
    from mdapy_amd import _lib

    if _lib.device_count() < 1:
        pytest.fail("test_gpu_unwrap needs a HIP device")


# ---- the device side, through the shim; outputs start as NaN / INT64_MIN
def _run(pos, cells, pbc, row_of=None, image=None, chunks=0, want_shifts=True):
    from mdapy_amd import kernels

    unwrapped = np.full(pos.shape, np.nan)
    shifts = np.full(pos.shape, INT64_MIN, np.int64) if want_shifts else None
    kernels.unwrap.unwrap(pos, cells, pbc, unwrapped, row_of=row_of, image=image, shifts=shifts, chunks=chunks)
    return unwrapped, shifts


def _stored(canonical, row_of):
    """the rows of every frame put where row_of says they are stored"""
    out = np.empty_like(canonical)
    out[np.arange(len(canonical))[:, None], row_of] = canonical
    return out


def _variants(kind, F, N):
    """(what, the shim's arguments) of every variant of one input: two boundaries x plain / row_of x min_image / image"""
    walk, wrapped, n, cells = R.case(kind, F, N)
    row_of = R.permutations(F, N, 7 * F + N)
    flags = n.astype(np.int32)
    for pbc in ((1, 1, 1), (1, 0, 1)):
        for rows in (None, row_of):
            pos = wrapped if rows is None else _stored(wrapped, rows)
            for image in (None, flags):
                stored_image = image if image is None or rows is None else _stored(image, rows)
                what = f"{kind}({F}, {N}) pbc {pbc} {'row_of ' if rows is not None else ''}{'image' if image is not None else 'min_image'}"
                yield what, dict(pos=pos, cells=cells, pbc=pbc, row_of=rows, image=stored_image)


def _same_bits(what, args, chunks=0):
    want, want_shifts = R.restate(args["pos"], args["cells"], args["pbc"], args["row_of"], args["image"])
    got, shifts = _run(chunks=chunks, **args)
    assert not np.isnan(got).any() and not (shifts == INT64_MIN).any(), f"{what}: an output entry was not written"
    print(f"{what}, chunks {chunks}: {int((got != want).sum())} positions and {int((shifts != want_shifts).sum())} shifts differ")
    assert np.array_equal(shifts, want_shifts), what
    assert np.array_equal(got, want), what
    return got, shifts


def test_inputs_hold_what_they_are_said_to():
    F, N = BIG
    for kind in BOXES:
        walk, wrapped, n, cells = R.case(kind, F, N)
        assert R.margin(wrapped, cells) >= 1e-6
        _, shifts = R.restate(wrapped, cells, (1, 1, 1))
        steps = np.diff(shifts, axis=0)
        assert (steps > 0).any() and (steps < 0).any() and np.abs(shifts[-1]).max() >= 2, "boundaries are crossed, both ways, repeatedly"
    assert np.any(np.diff(R.cells_of("npt", F), axis=0) != 0), "the NPT cell changes in every frame"


@pytest.mark.parametrize("N", EDGE_N)
@pytest.mark.parametrize("F", EDGE_F)
def test_tile_edges(F, N):
    for kind in BOXES:
        walk, wrapped, n, cells = R.case(kind, F, N)
        assert R.margin(wrapped, cells) >= 1e-6
        for what, args in _variants(kind, F, N):
            got, shifts = _same_bits(what, args)
            if F == 1 and args["image"] is None:
                assert not shifts.any() and np.array_equal(got, R.restate(args["pos"], cells, (0, 0, 0), args["row_of"])[0]), \
                    "one frame has no step"


@pytest.mark.parametrize("kind", BOXES)
def test_chunks_change_no_bit(kind):
    F, N = BIG
    for what, args in _variants(kind, F, N):
        first = _same_bits(what, args, chunks=0)
        for chunks in (1, 2, 3, F, F + 5):
            again = _run(chunks=chunks, **args)
            assert np.array_equal(again[0], first[0]) and np.array_equal(again[1], first[1]), f"{what}: chunks {chunks}"
    alone, none = _run(want_shifts=False, **args)
    assert none is None and np.array_equal(alone, first[0]), "without shifts, the same positions"


def _dyadic(F, N, seed):
    """(walk, wrapped, n, cells): box lengths 8, 16, 4, positions on a 2^-10 grid, starts inside the box, steps below a quarter
    of the shortest edge"""
    rng = np.random.default_rng(seed)
    lengths = np.array([8.0, 16.0, 4.0])
    grid = 2.0 ** -10
    start = rng.integers(0, (lengths / grid).astype(np.int64), (1, N, 3))
    steps = rng.integers(-300, 301, (F, N, 3))
    steps[:, 0::2, 2] += 600  # a drift along the shortest edge, up for even atoms and down for odd ones, and along x for some:
    steps[:, 1::2, 2] -= 600  # a step stays below 900 grid units = 0.22 of the shortest edge
    steps[:, 0::3, 0] += 600
    steps[0] = 0
    walk = (start + np.cumsum(steps, axis=0)) * grid
    n = np.floor(walk / lengths)
    wrapped = walk - n * lengths
    cells = np.repeat(np.diag(lengths)[None], F, axis=0)
    return walk, wrapped, n.astype(np.int64), cells


def test_dyadic_walk_comes_back_exactly():
    F, N = BIG
    walk, wrapped, n, cells = _dyadic(F, N, 11)
    assert R.margin(wrapped, cells) >= 1e-6 and not n[0].any() and np.abs(n[-1]).max() >= 2
    got, shifts = _run(wrapped, cells, (1, 1, 1))
    assert np.array_equal(shifts, n) and np.array_equal(got, walk)
    by_image, image_shifts = _run(wrapped, cells, (1, 1, 1), image=n.astype(np.int32))
    assert np.array_equal(by_image, walk) and np.array_equal(image_shifts, n)
    # the whole walk 2^20 boxes from the origin: image mode with large flags
    far = n + 2 ** 20
    moved = walk + 2.0 ** 20 * np.diag(cells[0])
    assert np.array_equal(moved - far * np.diag(cells[0]), wrapped)
    by_image, image_shifts = _run(wrapped, cells, (0, 0, 0), image=far.astype(np.int32))
    assert np.array_equal(image_shifts, far) and np.array_equal(by_image, moved)


# ---- through the public interface
def _write_dump(path, wrapped, lengths, seed):
    rng = np.random.default_rng(seed)
    F, N = wrapped.shape[:2]
    with open(path, "w") as f:
        for t in range(F):
            f.write(f"ITEM: TIMESTEP\n{10 * t}\nITEM: NUMBER OF ATOMS\n{N}\nITEM: BOX BOUNDS pp pp pp\n")
            f.write("".join(f"0.0 {float(v)!r}\n" for v in lengths))
            f.write("ITEM: ATOMS id type x y z\n")
            for i in rng.permutation(N):
                f.write(f"{i + 1} {1 + i % 2} " + " ".join(repr(float(v)) for v in wrapped[t, i]) + "\n")


def _check_direct_msd(pos, walk):
    """test_gpu_msd.py's direct-mode rule: particle_msd bit for bit, msd within (2 (1 + 2) + 2 (N + 2)) 2^-53 of fsum / N"""
    import math

    F, N = walk.shape[:2]
    want = _msd_ref.restate(walk).direct
    one = mp.MeanSquaredDisplacement(pos, mode="direct")
    one.compute()
    assert np.array_equal(one.particle_msd, want)
    want_msd = np.array([math.fsum(row) / float(N) for row in want])
    assert np.all(np.abs(one.msd - want_msd) <= (2.0 * 3.0 + 2.0 * (N + 2.0)) * EPS * want_msd)
    assert want_msd[-1] > 1.0, "the atoms went somewhere"


def test_file_to_msd(tmp_path):
    F, N = 2 * T + 3, AB + 1
    walk, wrapped, n, cells = _dyadic(F, N, 5)
    path = tmp_path / "walk.lammpstrj"
    _write_dump(path, wrapped, np.diag(cells[0]), 3)
    traj = mp.Trajectory(str(path))
    assert len(traj) == F and traj.get_atoms_count().tolist() == [N] * F
    assert not np.array_equal(traj[0].data["id"].to_numpy(), np.arange(1, N + 1)), "the rows are shuffled"
    unwrapped = traj.unwrap()
    assert unwrapped._unwrap_method == "min_image" and np.array_equal(unwrapped[3].data["id"].to_numpy(), np.arange(1, N + 1))
    pos = unwrapped.positions()
    assert isinstance(pos, np.ndarray) and np.array_equal(pos, walk)
    assert np.array_equal(unwrapped[F - 1].data["y"].to_numpy(), walk[F - 1, :, 1])
    _check_direct_msd(pos, walk)


def test_device_resident_frames_stay_on_the_device():
    import torch

    from mdapy_amd.devarray import HArray

    F, N = 2 * T + 3, AB + 1
    walk, wrapped, n, cells = _dyadic(F, N, 6)
    rng = np.random.default_rng(8)
    frames = []
    for t in range(F):
        order = rng.permutation(N)
        cols = {"id": HArray(torch.from_numpy((order + 1).astype(np.int32)).cuda())}
        cols.update({c: HArray(torch.from_numpy(np.ascontiguousarray(wrapped[t, order, d])).cuda()) for d, c in enumerate("xyz")})
        frames.append(mp.System(data=mp.Frame(cols), box=mp.Box(cells[t], [1, 1, 1])))
    unwrapped = mp.Trajectory(systems=frames).unwrap()
    pos = unwrapped.positions()
    assert isinstance(pos, HArray) and pos.dev().is_cuda and pos.shape == (F, N, 3)
    assert np.array_equal(pos.numpy(), walk)
    assert np.array_equal(unwrapped[2].data["id"].to_numpy(), np.arange(1, N + 1))
    assert np.array_equal(unwrapped[2].data["z"].to_numpy(), walk[2, :, 2])
    _check_direct_msd(pos, walk)


# ---- what is refused
def test_argument_errors():
    from mdapy_amd import _lib, kernels

    walk, wrapped, n, cells = R.case("cubic", 3, 4)
    out = np.zeros((3, 4, 3))
    with pytest.raises(ValueError):
        kernels.unwrap.unwrap(np.zeros((0, 4, 3)), cells[:0], (1, 1, 1), np.zeros((0, 4, 3)))
    with pytest.raises(ValueError):
        kernels.unwrap.unwrap(wrapped, cells, (1, 1, 1), out, chunks=-1)
    with pytest.raises(ValueError):
        kernels.unwrap.unwrap(wrapped, cells, (1, 1, 1), None)
    L = _lib.lib()
    pbc = np.ones(3, np.int32)
    pos = np.ascontiguousarray(wrapped)
    c = np.ascontiguousarray(cells)
    assert L.mdh_unwrap_trajectory(pos.ctypes.data, None, None, c.ctypes.data, c.ctypes.data, pbc.ctypes.data, 0, 4, 0,
                                   out.ctypes.data, None, _lib.HOST, None) == _lib.ERR_ARG
    assert L.mdh_unwrap_trajectory(pos.ctypes.data, None, None, c.ctypes.data, c.ctypes.data, pbc.ctypes.data, 3, 4, -1,
                                   out.ctypes.data, None, _lib.HOST, None) == _lib.ERR_ARG
    assert L.mdh_unwrap_trajectory(pos.ctypes.data, None, None, c.ctypes.data, c.ctypes.data, pbc.ctypes.data, 3, 4, 0,
                                   None, None, _lib.HOST, None) == _lib.ERR_ARG


def test_bad_data_raises_and_harms_nothing():
    """a NaN position and a row_of entry out of range are DATA the kernel meets: it uses neither (the step counts as 0, the atom's
    own row stands in), raises a flag, and the call fails; the next call computes as if nothing had happened"""
    F, N = BIG
    walk, wrapped, n, cells = R.case("sheared", F, N)
    bad = np.array(wrapped)
    bad[T + 2, AB + 1, 1] = np.nan
    for chunks in (1, 3):
        with pytest.raises(ValueError, match="not finite"):
            _run(bad, cells, (1, 1, 1), chunks=chunks)
    rows = R.permutations(F, N, 2)
    for entry in (N, -1, 2 ** 40):
        off = np.array(rows)
        off[F - 1, 0] = entry
        with pytest.raises(ValueError, match="row_of holds an entry outside"):
            _run(wrapped, cells, (1, 1, 1), row_of=off)
    _same_bits("after the refusals", dict(pos=wrapped, cells=cells, pbc=(1, 1, 1), row_of=None, image=None))
