"""The void analysis on the GPU: ``_neighbor._fill_cell_for_void``, the two helpers of ``_void`` and ``VoidAnalysis`` against the
numpy restatement of tests/_void_ref.py.

Grids, centres and the class's columns are compared with ``np.array_equal``: both sides take the same IEEE binary64 operations
in the same order (the library is built with -ffp-contract=off), and nothing in the kernels depends on the order threads run in.
The one exception is the sheared box, where the restatement's inverse and thickness (``mdapy_amd.Box``: LAPACK) and the
library's (adjugate over determinant) may differ in the last bits: that case first asserts on the CPU that no atom lies within
1e-9 of a face of a cell or of the box, so that such bits cannot move an atom into another cell.

What each seeded input is said to contain was checked on the CPU beforehand and is asserted here."""
import ctypes
import functools

import numpy as np
import pytest

import _void_cases as cases
import _void_ref
import mdapy_amd as mp
from mdapy_amd import _lib, kernels
from mdapy_amd.devarray import HArray, as_numpy

pytestmark = pytest.mark.gpu


@pytest.fixture(autouse=True)
def _need_gpu():
    if _lib.device_count() < 1:
        pytest.fail("test_gpu_void needs a HIP device")


# ---- inputs: name -> (positions (N, 3), Box, rc)
def _random(h, boundary, origin, n, seed, outside=False):
    rng = np.random.default_rng(seed)
    frac = rng.random((n, 3))
    if outside:  # every third atom up to three box lengths away along every axis
        frac[::3] += rng.integers(-3, 4, (len(frac[::3]), 3))
    h = np.asarray(h, np.float64)
    return frac @ h + np.asarray(origin, np.float64), mp.Box(h, boundary, origin)


SMALL = (np.diag([6.7, 9.1, 14.3]), [1, 1, 1], [-3.0, 2.5, 0.75])  # 3 x 4 x 7 cells of rc = 2
SHEARED = np.array([[14.0, 0.0, 0.0], [3.1, 17.0, 0.0], [-2.2, 4.0, 21.0]])


def _faces():
    """atoms exactly on the cell faces o + k rc and on the upper face of the box, along a periodic (x) and an open (y) axis"""
    h, origin, rc = np.diag([6.7, 9.1, 14.3]), np.array([-3.0, 2.5, 0.75]), 2.0
    rows = []
    for k in range(4):
        rows.append([origin[0] + k * rc, origin[1] + 0.3 + k, origin[2] + 1.0 + 2 * k])
    rows.append([origin[0] + 6.7, origin[1] + 5.0, origin[2] + 9.0])  # upper x face: wraps to cell 0
    for k in range(5):
        rows.append([origin[0] + 0.5 + k, origin[1] + k * rc, origin[2] + 0.4 + 2.5 * k])
    rows.append([origin[0] + 3.0, origin[1] + 9.1, origin[2] + 13.0])  # upper y face: clamps to the last cell
    for k in range(8):
        rows.append([origin[0] + 0.1 + 0.8 * k, origin[1] + 0.2 + k, origin[2] + k * rc])
    rows.append([origin[0] + 1.0, origin[1] + 1.0, origin[2] + 14.3])
    return np.array(rows), mp.Box(h, [1, 0, 1], origin), rc


@functools.lru_cache(maxsize=None)
def grid_case(name):
    if name in cases.FIXED:
        return cases.fixed(name)
    if name.startswith("small"):
        pos, cell = _random(*SMALL, n=int(name[5:]), seed=int(name[5:]))
        return pos, cell, 2.0
    if name == "faces":
        return _faces()
    if name == "outside_periodic":
        pos, cell = _random(*SMALL, n=257, seed=3, outside=True)
        return pos, cell, 2.0
    if name == "outside_open":
        pos, cell = _random(SMALL[0], [0, 0, 0], SMALL[2], n=257, seed=4, outside=True)
        return pos, cell, 2.0
    if name == "mixed":
        pos, cell = _random(SMALL[0], [1, 0, 1], SMALL[2], n=257, seed=5, outside=True)
        return pos, cell, 2.0
    if name == "remainder":  # L = 4.9 rc: four cells, the last one 1.9 rc wide
        pos, cell = _random(np.diag([9.8, 9.8, 9.8]), [1, 1, 1], [0, 0, 0], n=100, seed=6)
        return pos, cell, 2.0
    if name == "thin":  # L = 1.8 rc along y: three cells there, index 2 out of every atom's reach
        pos, cell = _random(np.diag([9.8, 3.6, 8.4]), [1, 1, 1], [0.5, 0.5, 0.5], n=2000, seed=7, outside=True)
        return pos, cell, 2.0
    if name == "thin_remainder":  # L = 2.5 rc along y: the third cell is the remainder, 0.5 rc wide
        pos, cell = _random(np.diag([9.8, 5.0, 8.4]), [1, 1, 1], [0.5, 0.5, 0.5], n=2000, seed=8)
        return pos, cell, 2.0
    if name == "sheared":
        pos, cell = _random(SHEARED, [1, 1, 0], [1.0, -2.0, 0.5], n=257, seed=9, outside=True)
        return pos, cell, 3.3
    if name == "big":  # 40 x 40 x 40 cells, 2000 atoms: more cells than one block of the scan takes
        pos, cell = _random(np.diag([40.5, 40.5, 40.5]), [1, 1, 1], [0, 0, 0], n=2000, seed=10)
        return pos, cell, 1.0
    raise KeyError(name)


GRID_CASES = sorted(cases.FIXED) + ["small1", "small63", "small64", "small65", "small257", "faces", "outside_periodic", "outside_open",
                                    "mixed", "remainder", "thin", "thin_remainder", "sheared", "big"]


@functools.lru_cache(maxsize=None)
def want_grid(name):
    pos, cell, rc = grid_case(name)
    grid = _void_ref._fill_cell_for_void(pos[:, 0], pos[:, 1], pos[:, 2], cell.box, cell.origin, cell.boundary, rc)
    grid.setflags(write=False)
    return grid


def _columns(pos):
    return tuple(np.ascontiguousarray(pos[:, k]) for k in range(3))


def _fill(pos, cell, rc, kind="harray"):
    cols = _columns(pos)
    if kind == "harray":
        cols = tuple(HArray.from_numpy(c) for c in cols)
    elif kind == "tensor":
        cols = tuple(HArray.from_numpy(c).dev() for c in cols)
    return kernels.neighbor._fill_cell_for_void(*cols, cell.box, cell.origin, cell.boundary, rc, 1)


def test_sheared_case_keeps_clear_of_every_face():
    """on the CPU: no fractional coordinate along a periodic axis within 1e-9 of a whole number (the wrap), no cell coordinate of a
    wrapped atom within 1e-9 of one (the floor)"""
    pos, cell, rc = grid_case("sheared")
    assert cell.triclinic
    inv, o = cell.inverse_box, cell.origin
    frac = (pos - o) @ inv
    periodic = cell.boundary == 1
    assert np.abs(frac[:, periodic] - np.round(frac[:, periodic])).min() > 1e-9
    coords = np.stack(_void_ref.cell_coordinates(cell, rc, *_void_ref.wrap(cell, pos[:, 0], pos[:, 1], pos[:, 2])), axis=1)
    assert np.abs(coords - np.round(coords)).min() > 1e-9


@pytest.mark.parametrize("name", GRID_CASES)
def test_grid_and_centres(name):
    pos, cell, rc = grid_case(name)
    want = want_grid(name)
    got = _fill(pos, cell, rc)
    assert isinstance(got, HArray) and got.dtype == np.int32 and got.shape == want.shape
    assert np.array_equal(got.numpy(), want)
    if name == "thin":
        assert want.shape[1] == 3 and want[:, :2, :].all() and not want[:, 2, :].any()
    if name == "thin_remainder":
        assert want.shape[1] == 3 and want[:, 2, :].any()
    if name == "remainder":
        assert want.shape == (4, 4, 4)
    if name.startswith("small") or name in ("faces", "mixed"):
        assert want.shape == (3, 4, 7)
    if name == "big":
        assert want.shape == (40, 40, 40) and 1900 < want.sum() <= 2000
    # the centres, in row-major order of their cells
    x, y, z, flat = kernels.void.void_points(got, cell.box, cell.origin, with_index=True)
    wx, wy, wz, wflat = _void_ref.void_points(want, cell.box, cell.origin, with_index=True)
    assert len(wx) == want.size - want.sum()
    if len(wx) == 0:
        assert len(x) == len(y) == len(z) == len(flat) == 0
        return
    assert isinstance(x, HArray) and x.dtype == np.float64 and flat.dtype == np.int32
    assert np.array_equal(flat.numpy(), wflat) and np.all(np.diff(flat.numpy()) > 0)
    assert np.array_equal(x.numpy(), wx) and np.array_equal(y.numpy(), wy) and np.array_equal(z.numpy(), wz)
    # without the index, and from a host grid: the same points
    hx, hy, hz = kernels.void.void_points(np.array(want), cell.box, cell.origin)
    assert isinstance(hx, np.ndarray) and np.array_equal(hx, wx) and np.array_equal(hy, wy) and np.array_equal(hz, wz)


@pytest.mark.parametrize("name", ["three_spheres", "mixed", "sheared"])
def test_grid_from_numpy_harray_and_tensor_input(name):
    pos, cell, rc = grid_case(name)
    want = want_grid(name)
    host = _fill(pos, cell, rc, kind="numpy")
    assert isinstance(host, np.ndarray) and host.dtype == np.int32 and np.array_equal(host, want)
    assert np.array_equal(_fill(pos, cell, rc, kind="tensor").numpy(), want)
    assert np.array_equal(_fill(pos, cell, rc, kind="harray").numpy(), want)
    # float32 input is converted, as every read-only argument is
    single = pos.astype(np.float32)
    narrow = kernels.neighbor._fill_cell_for_void(*_columns(single), cell.box, cell.origin, cell.boundary, rc)
    wide = single.astype(np.float64)
    assert np.array_equal(narrow, _void_ref._fill_cell_for_void(wide[:, 0], wide[:, 1], wide[:, 2], cell.box, cell.origin, cell.boundary, rc))


def test_output_buffer_is_cleared():
    """a buffer that held 7s comes back holding 0 and 1 only — in HBM and through the host staging"""
    pos, cell, rc = grid_case("small65")
    want = want_grid("small65")
    keep, (pb, po, pp) = _lib.host_box(cell.box, cell.origin, cell.boundary)
    cols = [HArray.from_numpy(c) for c in _columns(pos)]
    cells = HArray.full(want.shape, 7, np.int32)
    stream = int(mp.devarray.current_stream_ptr())
    _lib.check(_lib.lib().mdh_fill_cell_for_void(*(c.data_ptr() for c in cols), len(pos), pb, po, pp, rc, cells.data_ptr(), want.size,
                                                 _lib.DEVICE, stream))
    got = cells.dev().cpu().numpy()
    assert set(np.unique(got).tolist()) == {0, 1} and np.array_equal(got, want)
    host = np.full(want.shape, 7, np.int32)
    x, y, z = _columns(pos)
    _lib.check(_lib.lib().mdh_fill_cell_for_void(x.ctypes.data, y.ctypes.data, z.ctypes.data, len(pos), pb, po, pp, rc, host.ctypes.data,
                                                 want.size, _lib.HOST, None))
    assert np.array_equal(host, want)
    # no atom at all: every cell empty
    none = kernels.neighbor._fill_cell_for_void(x[:0], y[:0], z[:0], cell.box, cell.origin, cell.boundary, rc)
    assert none.shape == want.shape and not none.any()
    count = ctypes.c_int64(0)
    _lib.check(_lib.lib().mdh_void_points(cells.data_ptr(), *want.shape, pb, po, None, None, None, None, 0, ctypes.addressof(count),
                                          _lib.DEVICE, stream))
    assert count.value == want.size - want.sum()


@pytest.mark.parametrize("shape", ["mixed_waves", "one_giant", "all_single"])
def test_prune(shape):
    rng = np.random.default_rng(12)
    if shape == "mixed_waves":  # many ids per wave, ids outside 1 .. C among them
        m, c = 1000, 300
        ids = rng.integers(-2, c + 3, m).astype(np.int32)
    elif shape == "one_giant":  # every add of a wave lands on one word; more points than one block of the scan takes
        m, c = 70001, 5
        ids = np.full(m, 3, np.int32)
        ids[[5, 70000]] = [1, 5]
    else:
        m, c = 257, 257
        ids = rng.permutation(np.arange(1, 258)).astype(np.int32)
    x, y, z = rng.random((3, m))
    want = _void_ref.prune(x, y, z, ids, c)
    for kind in ("harray", "numpy"):
        args = [x, y, z, ids] if kind == "numpy" else [HArray.from_numpy(a) for a in (x, y, z, ids)]
        got = kernels.void.prune(*args, c)
        assert got[4] == want[4]
        for a, b in zip(got[:4], want[:4]):
            assert isinstance(a, np.ndarray if kind == "numpy" else HArray)
            assert as_numpy(a).dtype == b.dtype and np.array_equal(as_numpy(a), b)
    if shape == "one_giant":
        assert want[4] == 1 and len(want[0]) == m - 2 and set(want[3].tolist()) == {1}
    if shape == "all_single":
        assert want[4] == 0 and len(want[0]) == 0


# ---- the class
def _with_boundary(name, boundary):
    pos, cell, rc = cases.fixed(name)
    return pos, mp.Box(cell.box, boundary, cell.origin), rc


@functools.lru_cache(maxsize=None)
def class_case(name):
    """(positions, Box, rc, restated result)"""
    pos, cell, rc = _with_boundary("corner_periodic", [1, 0, 1]) if name == "corner_mixed" else cases.fixed(name)
    return pos, cell, rc, (cases.restated(name) if name in cases.FIXED else _void_ref.analyse(pos, cell, rc))


def _system(pos, cell, kind):
    if kind == "numpy":
        return mp.System(pos=np.array(pos), box=mp.Box(cell))
    if kind == "tensor":  # one (N, 3) device tensor, cut into columns on the device
        import torch

        cols = torch.from_numpy(np.array(pos)).to("cuda").t().contiguous()
        return mp.System(data={c: HArray(cols[k]) for k, c in enumerate("xyz")}, box=mp.Box(cell))
    return mp.System(data={c: HArray.from_numpy(np.ascontiguousarray(pos[:, k])) for k, c in enumerate("xyz")}, box=mp.Box(cell))


def _check(job, want, rc):
    assert type(job.void_number) is int and job.void_number == want.void_number
    assert type(job.void_volume) is float and job.void_volume == want.void_volume  # bit for bit
    if want.void_number == 0:
        assert job.void_system is None and job.void_volume == 0.0
        return
    found = job.void_system
    assert isinstance(found, mp.System) and found.N == len(want.x) and job.void_volume == found.N * rc ** 3
    assert list(found.data.columns) == ["x", "y", "z", "cluster_id", "element"]
    for column, values in zip(("x", "y", "z", "cluster_id"), (want.x, want.y, want.z, want.ids)):
        got = found.data[column].to_numpy()
        assert got.dtype == values.dtype and np.array_equal(got, values), column
    assert np.all(found.data["element"].to_numpy() == "X")
    assert sorted(set(want.ids.tolist())) == list(range(1, want.void_number + 1))


@pytest.mark.parametrize("name", sorted(cases.FIXED) + ["corner_mixed"])
def test_class_against_the_restatement(name):
    pos, cell, rc, want = class_case(name)
    if name in cases.FIXED:
        assert (want.void_number, 0 if want.x is None else len(want.x)) == cases.FIXED[name][1:]
    else:
        assert want.void_number == 2 and len(want.x) == 38  # the corner void cut along the one open axis
    runs = []
    for kind in ("numpy", "tensor", "harray", "harray"):  # the three kinds of input, and the last one again: identical bits
        job = mp.VoidAnalysis(_system(pos, cell, kind), rc)
        assert job.compute() is None
        _check(job, want, rc)
        runs.append(job)
    if want.void_number:
        for column in ("x", "y", "z", "cluster_id"):
            a, b = (r.void_system.data[column].to_numpy() for r in runs[2:])
            assert a.tobytes() == b.tobytes()
        assert isinstance(runs[1].void_system.data["x"].device_array(), HArray)


def test_only_single_cells_is_no_void():
    pos, cell, rc = cases.fixed("full")
    pos = cases._without_cells(pos, cell, rc, cases.SINGLE_CELLS[:3])
    want = _void_ref.analyse(pos, cell, rc)
    assert len(want.points) == 3 and want.cluster_number == 3 and want.void_number == 0
    job = mp.VoidAnalysis(_system(pos, cell, "harray"), rc)
    job.compute()
    assert job.void_system is None and job.void_number == 0 and job.void_volume == 0.0 and type(job.void_volume) is float


def test_input_system_is_left_alone():
    pos, cell, rc, want = class_case("three_spheres")
    system = _system(pos, cell, "numpy")
    system.build_neighbor(3.0)
    system.cal_centro_symmetry_parameter(12)
    frame, columns, rows, counts, reach = system.data, list(system.data.columns), system.verlet_list, system.neighbor_number, system.rc
    before = {c: system.data[c].to_numpy().copy() for c in columns}
    listed = as_numpy(rows).copy()
    state = set(system.__dict__)
    job = mp.VoidAnalysis(system, rc)
    job.compute()
    _check(job, want, rc)
    assert system.data is frame and list(system.data.columns) == columns and set(system.__dict__) == state
    assert system.verlet_list is rows and system.neighbor_number is counts and system.rc == reach
    assert np.array_equal(as_numpy(system.verlet_list), listed)
    for c in columns:
        assert np.array_equal(system.data[c].to_numpy(), before[c]), c


def test_one_void_through_most_of_the_box():
    """40^3 cells, 2000 atoms: one void of every empty cell (checked on the CPU by face connectivity, which is what 1.1 rc reaches
    in this cubic grid of 1.0125-wide cells); the compaction and the pruning run past one block of their scans"""
    pos, cell, rc = grid_case("big")
    grid = want_grid("big")
    empty = int(grid.size - grid.sum())
    job = mp.VoidAnalysis(_system(pos, cell, "harray"), rc)
    job.compute()
    assert job.void_number == 1 and job.void_system.N == empty and job.void_volume == empty * rc ** 3
    wx, wy, wz = _void_ref.void_points(grid, cell.box, cell.origin)
    for column, values in zip("xyz", (wx, wy, wz)):
        assert np.array_equal(job.void_system.data[column].to_numpy(), values)
    assert np.all(job.void_system.data["cluster_id"].to_numpy() == 1)


@pytest.mark.parametrize("rc", [0.0, -1.0])
def test_refuses_rc(rc):
    pos, cell, _ = cases.fixed("full")
    with pytest.raises(ValueError, match="rc"):
        mp.VoidAnalysis(_system(pos, cell, "numpy"), rc).compute()
    with pytest.raises(ValueError, match="rc must be a positive number"):
        _fill(pos, cell, rc)
