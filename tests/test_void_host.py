"""The void analysis without a GPU: the numpy restatement of tests/_void_ref.py against a per-atom loop and against the reference's
literal expression for the centres; ``VoidAnalysis`` — attributes, both ways of finding nothing, renumbering, the ``element``
column, the volume, the input system left alone — run through the oracle backend with the new shims replaced by that
restatement (the clustering is then the oracle's); the fixed cases, whose counts were checked beforehand with an independent
numpy / scipy restatement; and the argument checks of the real shims, which come before any device work."""
import math

import numpy as np
import pytest

import _void_cases as cases
import _void_ref
import mdapy_amd as mp
from mdapy_amd import _void, void_analysis  # noqa: F401  (what this file is about)

EPS = 2.0 ** -53


@pytest.fixture
def restated(oracle_backend, monkeypatch):
    import mdapy_amd.kernels as K

    monkeypatch.setattr(K.neighbor, "_fill_cell_for_void", _void_ref._fill_cell_for_void, raising=False)
    monkeypatch.setattr(K, "void", _void_ref)
    return _void_ref


BOXES = {
    "orthogonal": (np.diag([13.7, 17.2, 29.9]), [1, 1, 1], [-3.0, 2.5, 0.75]),
    "mixed": (np.diag([13.7, 17.2, 29.9]), [1, 0, 1], [-3.0, 2.5, 0.75]),
    "open": (np.diag([13.7, 17.2, 29.9]), [0, 0, 0], [0.0, 0.0, 0.0]),
    "thin": (np.diag([20.0, 9.0, 16.5]), [1, 1, 1], [0.0, 0.0, 0.0]),
    "triclinic": (np.array([[14.0, 0.0, 0.0], [3.1, 17.0, 0.0], [-2.2, 4.0, 21.0]]), [1, 1, 0], [1.0, -2.0, 0.5]),
}


def _atoms(name, n=300, seed=5):
    """random atoms, a fifth of them up to three box lengths outside"""
    h, boundary, origin = BOXES[name]
    rng = np.random.default_rng(seed)
    frac = rng.random((n, 3))
    frac[::5] += rng.integers(-3, 4, (len(frac[::5]), 3))
    return frac @ h + np.asarray(origin), mp.Box(h, boundary, origin)


def _loop_grid(pos, cell, rc):
    """src/neighbor.cpp:797-828 atom by atom in Python floats (IEEE binary64, one rounding per operation)"""
    h, inv, o, periodic = cell.box.tolist(), cell.inverse_box.tolist(), cell.origin.tolist(), [bool(p) for p in cell.boundary]
    thick = cell.get_thickness().tolist()
    ncell = [max(int(math.floor(t / rc)), 3) for t in thick]
    rc_inverse = 1.0 / rc
    grid = np.zeros(ncell, np.int32)

    def fractional(d):
        return [(d[0] * inv[0][e] + d[1] * inv[1][e]) + d[2] * inv[2][e] for e in range(3)]

    for p in pos.tolist():
        if any(periodic):
            if cell.triclinic:
                f = fractional([p[e] - o[e] for e in range(3)])
                f = [f[e] - math.floor(f[e]) if periodic[e] else f[e] for e in range(3)]
                p = [((o[e] + f[0] * h[0][e]) + f[1] * h[1][e]) + f[2] * h[2][e] for e in range(3)]
            else:
                for e in range(3):
                    if periodic[e]:
                        d = p[e] - o[e]
                        p[e] = (o[e] + d) - h[e][e] * math.floor(d / h[e][e])
        if cell.triclinic:
            n = fractional([p[e] - o[e] for e in range(3)])
            idx = [math.floor(n[e] * thick[e] * rc_inverse) for e in range(3)]
        else:
            idx = [math.floor((p[e] - o[e]) * rc_inverse) for e in range(3)]
        idx = [max(0, min(idx[e], ncell[e] - 1)) for e in range(3)]
        grid[idx[0], idx[1], idx[2]] = 1
    return grid


@pytest.mark.parametrize("name", sorted(BOXES))
def test_grid_against_a_per_atom_loop(name):
    pos, cell = _atoms(name)
    rc = 3.3
    got = _void_ref._fill_cell_for_void(pos[:, 0], pos[:, 1], pos[:, 2], cell.box, cell.origin, cell.boundary, rc)
    want = _loop_grid(pos, cell, rc)
    assert got.dtype == np.int32 and got.shape == want.shape == _void_ref.grid_dims(cell, rc)
    assert np.array_equal(got, want)
    assert set(np.unique(got)) <= {0, 1} and 0 < got.sum() <= len(pos)
    if name == "thin":  # 9.0 < 3 rc: two rc-wide cells and a third that starts at 2 rc = 6.6 ... and still takes atoms up to 9.0
        assert got.shape[1] == 3 and got[:, 2, :].any()
    assert not _void_ref._fill_cell_for_void(pos[:0, 0], pos[:0, 1], pos[:0, 2], cell.box, cell.origin, cell.boundary, rc).any()


def test_thin_axis_leaves_its_third_layer_empty():
    """thickness < 2 rc: floor(L / rc) < 2, the grid still has 3 cells there, and no wrapped atom reaches index 2"""
    h, boundary, origin = np.diag([20.0, 6.0, 16.5]), [1, 1, 1], [0.0, 0.0, 0.0]
    pos = np.random.default_rng(2).random((4000, 3)) @ h
    grid = _void_ref._fill_cell_for_void(pos[:, 0], pos[:, 1], pos[:, 2], h, np.asarray(origin), np.asarray(boundary), 3.3)
    assert grid.shape == (6, 3, 5) and grid[:, :2, :].all() and not grid[:, 2, :].any()
    assert np.array_equal(grid, _loop_grid(pos, mp.Box(h, boundary, origin), 3.3))


@pytest.mark.parametrize("name", sorted(BOXES))
def test_centres_against_the_literal_expression(name):
    pos, cell = _atoms(name, n=40)
    rc = 3.3
    grid = _void_ref._fill_cell_for_void(pos[:, 0], pos[:, 1], pos[:, 2], cell.box, cell.origin, cell.boundary, rc)
    x, y, z, flat = _void_ref.void_points(grid, cell.box, cell.origin, with_index=True)
    index = np.argwhere(grid == 0)
    assert len(index) >= 30 and len(x) == len(index) and flat.dtype == np.int32
    assert np.array_equal(flat, np.ravel_multi_index(index.T, grid.shape)) and np.all(np.diff(flat) > 0)
    ncell = np.array(grid.shape, np.int32)
    literal = ((index + 0.5) / ncell) @ cell.box + cell.origin  # void_analysis.py:77-79
    f = (index + 0.5) / ncell
    # one product rounding and at most three additions per side, two sides, f shared
    bound = 8 * EPS * (np.abs(f[:, :, None] * cell.box[None, :, :]).sum(axis=1) + np.abs(cell.origin)[None, :])
    got = np.stack([x, y, z], axis=1)
    worst = float((np.abs(got - literal) / bound).max())
    print(f"{name}: centres against the literal expression, worst difference {worst:.3f} of the bound")
    assert np.all(np.abs(got - literal) <= bound)
    # centres of EQUAL cells: strictly inside the box, (i + 0.5) / ncell of the way along every axis
    frac = (got - cell.origin) @ cell.inverse_box
    assert np.allclose(frac, f, rtol=0, atol=1e-12)


def test_prune_restated():
    x = np.arange(9.0)
    ids = np.array([3, 1, 3, 2, 5, 5, 0, 7, 5], np.int32)  # 0 and 7 are outside 1 .. 5: no cluster
    kx, ky, kz, new, voids = _void_ref.prune(x, x + 10, x + 20, ids, 5)
    assert voids == 2 and new.dtype == np.int32
    assert kx.tolist() == [0, 2, 4, 5, 8] and ky.tolist() == [10, 12, 14, 15, 18] and kz.tolist() == [20, 22, 24, 25, 28]
    assert new.tolist() == [1, 1, 2, 2, 2]
    assert _void_ref.prune(x, x, x, np.arange(1, 10, dtype=np.int32), 9)[4] == 0


# ---- the class
def _system(name):
    pos, cell, rc = cases.fixed(name)
    return mp.System(pos=np.array(pos), box=mp.Box(cell)), rc


def test_class_attributes(restated):
    assert mp.VoidAnalysis is mp.void_analysis.VoidAnalysis and "VoidAnalysis" in mp.__all__
    system, rc = _system("three_spheres")
    frame, columns = system.data, list(system.data.columns)
    x_before = system.data["x"].to_numpy().copy()
    job = mp.VoidAnalysis(system, rc)
    assert job.system is system and job.rc == rc and job.void_system is None
    assert job.compute() is None
    want = cases.restated("three_spheres")
    assert type(job.void_number) is int and job.void_number == want.void_number == 3
    assert type(job.void_volume) is float and job.void_volume == want.void_volume == 44 * rc ** 3
    found = job.void_system
    assert isinstance(found, mp.System) and found.N == 44
    assert list(found.data.columns) == ["x", "y", "z", "cluster_id", "element"]
    assert np.array_equal(found.box.box, system.box.box) and np.array_equal(found.box.boundary, system.box.boundary)
    for name, values in zip(("x", "y", "z"), (want.x, want.y, want.z)):
        assert found.data[name].dtype == np.float64 and np.array_equal(found.data[name].to_numpy(), values), name
    ids = found.data["cluster_id"].to_numpy()
    assert ids.dtype == np.int32 and np.array_equal(ids, want.ids)
    assert sorted(set(ids.tolist())) == [1, 2, 3] and np.all(np.diff(ids[np.sort(np.unique(ids, return_index=True)[1])]) > 0)
    assert np.all(found.data["element"].to_numpy() == "X")
    assert "verlet_list" not in found.__dict__  # (the list of the unpruned points does not describe these rows)
    # the input system: the same frame object, no list, no new column, no moved atom
    assert system.data is frame and list(system.data.columns) == columns == ["x", "y", "z"]
    assert not {"verlet_list", "rc", "cluster_number"} & set(system.__dict__)
    assert np.array_equal(system.data["x"].to_numpy(), x_before)


@pytest.mark.parametrize("name", sorted(cases.FIXED))
def test_fixed_cases(restated, name):
    atoms, voids, kept = cases.FIXED[name]
    pos, cell, rc = cases.fixed(name)
    want = cases.restated(name)
    if atoms is not None:
        assert len(pos) == atoms
    assert want.ncell == ((23, 23, 23) if name == "reference_scaled" else (11, 11, 11))
    assert want.void_number == voids and (0 if want.x is None else len(want.x)) == kept
    dropped = {"corner_small_open": 4, "single_cells": 2}.get(name, 0)  # single-cell "voids"
    assert len(want.points) == kept + dropped and want.cluster_number == voids + dropped
    system, _ = _system(name)
    job = mp.VoidAnalysis(system, rc)
    job.compute()
    assert job.void_number == voids and job.void_volume == want.void_volume == kept * rc ** 3
    if voids == 0:
        assert job.void_system is None and job.void_volume == 0.0 and type(job.void_volume) is float
        return
    assert job.void_system.N == kept
    for column, values in zip(("x", "y", "z", "cluster_id"), (want.x, want.y, want.z, want.ids)):
        assert np.array_equal(job.void_system.data[column].to_numpy(), values), column
    assert sorted(set(want.ids.tolist())) == list(range(1, voids + 1))


def test_only_single_cells_is_no_void(restated):
    """empty cells, but none with an empty neighbour: every cluster is dropped and void_system stays None"""
    pos, cell, rc = cases.fixed("full")
    pos = cases._without_cells(pos, cell, rc, cases.SINGLE_CELLS[:3])
    want = _void_ref.analyse(pos, cell, rc)
    assert len(want.points) == 3 and want.cluster_number == 3 and want.void_number == 0 and want.x is None
    job = mp.VoidAnalysis(mp.System(pos=pos, box=mp.Box(cell)), rc)
    job.compute()
    assert job.void_system is None and job.void_number == 0 and job.void_volume == 0.0


@pytest.mark.parametrize("rc", [0, 0.0, -4.1, float("nan")])
def test_class_refuses_rc(restated, rc):
    system, _ = _system("full")
    with pytest.raises(ValueError, match="rc"):
        mp.VoidAnalysis(system, rc).compute()


# ---- the real shims
def test_shims_check_arguments_before_any_device_work():
    from mdapy_amd import _lib, kernels

    assert kernels.void.__name__ == "mdapy_amd._void" and "void" not in kernels.NAMES
    fill = kernels.neighbor._fill_cell_for_void
    x = np.linspace(0.0, 9.0, 7)
    box, origin, boundary = np.eye(3) * 10.0, np.zeros(3), np.ones(3, np.int32)
    for rc in (0.0, -1.0, float("nan"), float("inf")):
        with pytest.raises(ValueError, match="rc must be a positive number"):
            fill(x, x, x, box, origin, boundary, rc)
    singular = np.array([[1.0, 1.0, 0.0], [2.0, 2.0, 0.0], [0.0, 0.0, 1.0]])
    with pytest.raises(ValueError, match="singular"):
        fill(x, x, x, singular, origin, boundary, 1.0)
    with pytest.raises(ValueError, match="singular"):
        fill(x, x, x, np.diag([10.0, 0.0, 10.0]), origin, boundary, 1.0)
    with pytest.raises(ValueError, match="too large"):  # 2000^3 cells
        fill(x, x, x, box, origin, boundary, 0.005)
    with pytest.raises(ValueError, match="rows"):
        fill(x, x[:3], x, box, origin, boundary, 3.0)
    with pytest.raises(ValueError, match="cell_id_list"):
        kernels.void.void_points(np.zeros((3, 3), np.int32), box, origin)
    with pytest.raises(ValueError, match="rows"):
        kernels.void.prune(x, x, x, np.ones(3, np.int32), 1)
    # the library itself: the grid's size needs no device, and a buffer of another size is refused
    import ctypes

    L = _lib.lib()
    dims = (ctypes.c_int * 3)()
    assert L.mdh_void_grid_dims(box.ctypes.data, origin.ctypes.data, boundary.ctypes.data, 3.0, ctypes.addressof(dims)) == 0
    assert list(dims) == [3, 3, 3]
    assert L.mdh_void_grid_dims(box.ctypes.data, origin.ctypes.data, boundary.ctypes.data, 2.3, ctypes.addressof(dims)) == 0
    assert list(dims) == [4, 4, 4]
    assert L.mdh_void_grid_dims(box.ctypes.data, origin.ctypes.data, boundary.ctypes.data, 0.0, ctypes.addressof(dims)) == _lib.ERR_ARG
    cells = np.zeros(28, np.int32)
    assert L.mdh_fill_cell_for_void(x.ctypes.data, x.ctypes.data, x.ctypes.data, 7, box.ctypes.data, origin.ctypes.data, boundary.ctypes.data,
                                    3.0, cells.ctypes.data, 28, _lib.HOST, None) == _lib.ERR_ARG
    count = ctypes.c_int64(-1)
    assert L.mdh_void_points(cells.ctypes.data, 0, 3, 3, box.ctypes.data, origin.ctypes.data, None, None, None, None, 0,
                             ctypes.addressof(count), _lib.HOST, None) == _lib.ERR_ARG
    assert L.mdh_void_prune(None, None, None, None, -1, 1, None, None, None, None, ctypes.addressof(count), ctypes.addressof(dims),
                            _lib.HOST, None) == _lib.ERR_ARG
    if _lib.device_count() > 0:
        return  # (with a device the valid calls compute: test_gpu_void.py)
    with pytest.raises(RuntimeError, match="HIP error"):
        fill(x, x, x, box, origin, boundary, 3.0)
    with pytest.raises(RuntimeError, match="HIP error"):
        kernels.void.void_points(np.zeros((3, 3, 3), np.int32), box, origin)
    with pytest.raises(RuntimeError, match="HIP error"):
        kernels.void.prune(x, x, x, np.ones(7, np.int32), 1)
