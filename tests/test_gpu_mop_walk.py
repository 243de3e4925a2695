"""-m gpu: the thread-per-atom and wave-per-atom kernels of neighbor.hip (k_neighbor, k_neighbor_mop) as a matrix of the kernel that
runs, the form of the cell grid it walks (CellView, grid.hpp), the row mode and the box.  Every comparison is bitwise against the
CPU oracle: O.build_neighbor_without_max_neigh for the counts, O.build_neighbor for rows two slots narrower than the largest
count — rows overflow, the count keeps running.

  kernel   thread per atom: mdh_debug_set_neighbor_variant(1), the whole call; wave per atom: the tiles the tile kernel lists for
           the packed cell of test_gpu_slot_grid._spread_and_packed under variant 0
  form     compact: mdh_debug_set_slot_grid(0); slot grid: a call behind a finished build of the same (N, grid) by the tile kernel
           (the history wants that kernel's report of the tiles it listed, which variant 1 never makes); slot grid with a spill
           list: the packed input behind a build of the spread one.  Asserted through mdh_debug_slot_grid_counters [0]
  mode     mdh_neighbor_count (counts and their maximum); caller's pads kept; pads written
  box      orthogonal; sheared by 5 % (test_gpu_slot_grid.test_small_shear)

The 3x3x3-cell fcc boxes (108 atoms, three grid cells per axis, so the tile kernel refuses them and nothing ever reports to the slot
grid's history) are compact builds only: fully periodic, no centre has a contiguous z-run and every neighbour cell is reached through
pmod on all three axes; with z open the centres of the middle z plane take the one-run path, the others three pieces.  The
wave-per-atom kernel on a compact grid wants tiles over the tile kernel's LDS budget: test_gpu_parity's dense_blob cases."""
import ctypes
import functools

import numpy as np
import pytest

from mdapy_amd import _lib, _neighbor
from oracle import oracle as O
from test_gpu_slot_grid import A_CU, ORG0, PBC, RC, _lattice, _slot_counters, _spread_and_packed, _xyz

pytestmark = pytest.mark.gpu

OPEN_Z = np.array([1, 1, 0], np.int32)
MODES = ("count", "keep_pads", "write_pads")


@pytest.fixture(autouse=True)
def fresh_history():
    L = _lib.lib()
    L.mdh_debug_set_slot_grid(2)
    yield
    L.mdh_debug_set_neighbor_variant(0)
    L.mdh_debug_set_slot_grid(1)


def _sheared(pos, box):
    """the box and its atoms sheared by 5 %"""
    sheared = box.copy()
    sheared[1][0] = 0.05 * box[1][1]
    return np.ascontiguousarray(pos @ np.linalg.inv(box) @ sheared), sheared


@functools.lru_cache(maxsize=None)
def _case(name, shear):
    """(x, y, z, box) of a named input, read-only"""
    if name in ("lattice", "spread", "packed"):
        pos, box = _lattice(10, 10, 10)
        assert len(pos) == 4000 and int(box[0][0] // RC) == 11
        if name != "lattice":
            spread, packed, box = _spread_and_packed()
            pos = spread if name == "spread" else packed
    else:
        pos, box = _lattice(3, 3, 3)
        assert len(pos) == 108 and int(box[0][0] // RC) == 3
    if shear:
        pos, box = _sheared(pos, box)
    out = _xyz(pos) + (box,)
    for a in out:
        a.setflags(write=False)
    return out


@functools.lru_cache(maxsize=None)
def _oracle(name, shear, open_z, cap):
    """counts, and the rows at two slots below the largest count (cap != 0: at most cap slots) with the caller's pads (-1, rc + 1)
    behind them: computed once"""
    x, y, z, box = _case(name, shear)
    bnd = OPEN_Z if open_z else PBC
    v0, d0, n0 = O.build_neighbor_without_max_neigh(x, y, z, box, ORG0, bnd, RC, 4)
    M = int(n0.max()) - 2
    if cap:
        M = min(M, cap)
    assert M >= 1
    va = np.full((len(x), M), -1, np.int32); da = np.full((len(x), M), RC + 1.0); na = np.zeros(len(x), np.int32)
    O.build_neighbor(x, y, z, box, ORG0, bnd, RC, va, da, na, 4)
    assert np.array_equal(na, n0) and (na > M).any()
    for a in (va, da, na):
        a.setflags(write=False)
    return va, da, na


def _run(mode, name, shear, open_z=False, cap=0):
    """one call of the library in `mode`, compared with the oracle"""
    x, y, z, box = _case(name, shear)
    bnd = OPEN_Z if open_z else PBC
    va, da, na = _oracle(name, shear, open_z, cap)
    n, M = va.shape
    if mode == "count":
        keep, (pb, po, pp) = _lib.host_box(box, ORG0, bnd)
        nb = np.full(n, -7, np.int32)
        most = ctypes.c_int(-1)
        _lib.check(_lib.lib().mdh_neighbor_count(x.ctypes.data, y.ctypes.data, z.ctypes.data, n, pb, po, pp, RC, nb.ctypes.data,
                                                 ctypes.addressof(most), 0, None))
        assert np.array_equal(nb, na) and most.value == int(na.max()), (mode, name, shear)
        return
    if mode == "keep_pads":
        vb = np.full((n, M), -1, np.int32); db = np.full((n, M), RC + 1.0); nb = np.zeros(n, np.int32)
        _neighbor.build_neighbor(x, y, z, box, ORG0, bnd, RC, vb, db, nb, 1)
    else:
        vb = np.full((n, M), -9, np.int32); db = np.full((n, M), -9.0); nb = np.full(n, -9, np.int32)
        _neighbor.build_neighbor(x, y, z, box, ORG0, bnd, RC, vb, db, nb, 1, fill_pads=True)
    assert np.array_equal(nb, na) and np.array_equal(vb, va) and np.array_equal(db, da), (mode, name, shear)


def _prime(name, shear):
    """a finished build of the signature by the tile kernel, its history forgotten before: the next build may be a slot build"""
    L = _lib.lib()
    L.mdh_debug_set_slot_grid(2)
    L.mdh_debug_set_neighbor_variant(0)
    _run("write_pads", name, shear)
    assert _slot_counters()[0] == 0  # (the first build of a signature is a compact one)


@pytest.mark.parametrize("shear", [False, True], ids=["orthogonal", "sheared"])
@pytest.mark.parametrize("form", ["compact", "slot"])
def test_thread_per_atom(form, shear):
    """the 10^3-cell lattice (4 000 atoms, 11 grid cells per axis, a wide last cell), the whole call by k_neighbor"""
    L = _lib.lib()
    if form == "slot":
        _prime("lattice", shear)
    else:
        L.mdh_debug_set_slot_grid(0)
    L.mdh_debug_set_neighbor_variant(1)
    for mode in MODES:
        _run(mode, "lattice", shear)
        assert _slot_counters()[0] == (form == "slot"), (mode, form)


@pytest.mark.parametrize("shear", [False, True], ids=["orthogonal", "sheared"])
@pytest.mark.parametrize("kernel", ["thread", "wave"])
@pytest.mark.parametrize("mode", MODES)
def test_overflowed_cell(mode, kernel, shear):
    """the packed cell of 13 to 16 atoms on a slot grid: eight in its slots, the rest on the spill list.  Variant 1: k_neighbor takes
    the call; variant 0: the tile kernel lists the cell's tiles for the wave-per-atom form.  (The build that meets the cell reports
    it, so every mode starts from the spread input's history.)  The largest count is 24; rows of more than 16 slots never take a slot
    grid (slot_grid_rule), so the rows here are 16 wide, not 22: they overflow all the same."""
    L = _lib.lib()
    _prime("spread", shear)
    L.mdh_debug_set_neighbor_variant(1 if kernel == "thread" else 0)
    _run(mode, "packed", shear, cap=16)
    s = _slot_counters()
    assert s[0] == 1 and s[1] == 1 and 13 <= s[2] <= 16 and s[3] == 8, s


@pytest.mark.parametrize("shear", [False, True], ids=["orthogonal", "sheared"])
@pytest.mark.parametrize("kernel", ["thread", "wave"])
def test_packed_cell_on_the_compact_grid(kernel, shear):
    """the same input with the slot grid switched off, rows of 22 slots: the atoms come as cell-sorted records"""
    L = _lib.lib()
    L.mdh_debug_set_slot_grid(0)
    L.mdh_debug_set_neighbor_variant(1 if kernel == "thread" else 0)
    for mode in MODES:
        _run(mode, "packed", shear)
        assert _slot_counters()[0] == 0, mode


@pytest.mark.parametrize("shear", [False, True], ids=["orthogonal", "sheared"])
@pytest.mark.parametrize("open_z", [False, True], ids=["periodic", "open_z"])
def test_three_cells_per_axis(open_z, shear):
    """108 atoms in 3 x 3 x 3 grid cells: every neighbour cell through pmod; z open: one run for the middle plane's centres, three
    pieces for the first and the last plane's"""
    L = _lib.lib()
    L.mdh_debug_set_slot_grid(0)
    L.mdh_debug_set_neighbor_variant(1)
    assert A_CU * 3 / RC < 4
    for mode in MODES:
        _run(mode, "fcc3", shear, open_z)
