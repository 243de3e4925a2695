"""The front of the tile neighbour kernel (neighbor_lane.hip): interior tiles take a short halo_of and stage without an image
shift, hit masks are cleaned with a bitwise select, the halo-cell offset of a run comes from a byte table, and a group of four
square roots asks one range question.  None of it may change a result: every case runs mdh_build_neighbor_fcna through the tile
kernel and through the thread-per-atom path of the same library (mdh_debug_set_neighbor_variant(1)) and compares rows, distances,
counts and labels entry for entry; mdh_debug_neighbor_plan says that the tile kernel ran and with which tile, and from the tile and
the grid the case checks that the input has a tile of the kind it is about (an interior one, or none).

Sizes: an fcc block of 12 x 12 x 12 unit cells has 14 grid cells per axis at rc = 0.854 a — a 4x4x5 tile then has tiles with the
halo strictly inside the grid next to tiles on every seam.  A case whose planner answers with another shape grows its block by
two unit cells until an interior tile exists (_build_until_interior)."""
import numpy as np
import pytest

from mdapy_amd import _lib, _neighbor
from mdapy_amd.build_lattice import lattice_positions

A_CU = 3.615
RC = 0.854 * A_CU
ORG0 = np.zeros(3)
PBC = np.array([1, 1, 1], np.int32)


def _xyz(pos):
    return tuple(np.ascontiguousarray(pos[:, k]) for k in range(3))


def _fused(pos, box, bnd, rc, M):
    x, y, z = _xyz(pos)
    n = len(x)
    v = np.empty((n, M), np.int32); d = np.empty((n, M)); c = np.empty(n, np.int32); p = np.zeros(n, np.int32)
    _neighbor.build_neighbor_fcna(x, y, z, box, ORG0, bnd, rc, v, d, c, p, 1, fill_pads=True)
    return v, d, c, p


def _plan():
    plan = np.zeros(8, np.int32)
    _lib.lib().mdh_debug_neighbor_plan(plan.ctypes.data)
    return plan


def _cells(box, rc):
    """cells per axis of the rc-wide grid: floor(thickness / rc) along every box vector (neighbor.cpp:29-62)"""
    h = np.asarray(box, float).reshape(3, 3)
    vol = abs(np.linalg.det(h))
    thick = [vol / np.linalg.norm(np.cross(h[(d + 1) % 3], h[(d + 2) % 3])) for d in range(3)]
    return [max(1, int(np.floor(t / rc))) for t in thick]


def _interior_tiles(plan, nc, bnd):
    """tiles whose whole halo lies inside the grid, one cell further in on an open axis (the kernel's rule)"""
    count = 1
    for d in range(3):
        T = int(plan[1] if d == 2 else plan[0])
        m = 1 if bnd[d] else 2
        count *= sum(1 for t in range(0, nc[d], T) if t >= m and t + T + m <= nc[d])
    return count


def _both(tag, pos, box, bnd=PBC, rc=RC, M=16):
    """tile kernel against the thread-per-atom path, entry for entry; returns (plan of the tile build, counts, labels)"""
    L = _lib.lib()
    _plan()  # (clears "a plan was made since the last query")
    got = _fused(pos, box, bnd, rc, M)
    plan = _plan()
    assert plan[0] > 0 and plan[7] == 1, (tag, "the tile kernel did not take the build", plan.tolist())
    L.mdh_debug_set_neighbor_variant(1)
    try:
        ref = _fused(pos, box, bnd, rc, M)
    finally:
        L.mdh_debug_set_neighbor_variant(0)
    for name, a, b in zip(("verlet", "dist", "nn", "pattern"), got, ref):
        assert np.array_equal(a, b), (tag, name, int((a != b).sum()))
    return plan, got[2], got[3]


def _build_until_interior(tag, make, bnd=PBC, rc=RC, M=16, n0=12):
    """make(n) -> (pos, box) of a block of n unit cells per axis; grown until the planner's tile has an interior one"""
    for n in range(n0, n0 + 9, 2):
        pos, box = make(n)
        plan, counts, labels = _both((tag, n), pos, box, bnd, rc, M)
        interior = _interior_tiles(plan, _cells(box, rc), bnd)
        if interior > 0:
            nt = np.prod([-(-c // int(plan[1] if d == 2 else plan[0])) for d, c in enumerate(_cells(box, rc))])
            assert interior < nt, (tag, "no seam or face tile", plan.tolist())
            return pos, box, plan, counts, labels
    raise AssertionError((tag, "no interior tile up to", n, plan.tolist()))


def _fcc(n, sigma=0.0, seed=1):
    pos, box = lattice_positions("fcc", A_CU, n, n, n)
    if sigma:
        pos = pos + np.random.default_rng(seed).normal(0.0, sigma, pos.shape)
    return pos, np.asarray(box, float)


gpu = pytest.mark.gpu


def test_run_offset_table_reproduces_run_cell():
    """host only (no device is touched): for every tile shape the planner can return (txy 1 ... 8, tz 1 ... 24, a halo of at most
    256 cells; tz = 1 is the slice pass's shape) the byte table, read as v_perm_b32 reads it — selector bytes 1 ... 3 zero, a
    selector >= 13 delivers 0xff — plus the bias gives ((r / 3 - 1) * HXY + (r % 3 - 1)) * HZ for the nine runs, modulo 2^32."""
    L = _lib.lib()
    out = np.zeros(3, np.uint32)
    shapes = 0
    for txy in range(1, 9):
        for tz in range(1, 25):
            hxy, hz = txy + 2, tz + 2
            rc_ = L.mdh_debug_run_offset_table(txy, tz, out.ctypes.data)
            if hxy * hxy * hz > 256:
                assert rc_ != 0, (txy, tz)
                continue
            assert rc_ == 0, (txy, tz)
            shapes += 1
            table = int(out[0]) | (int(out[1]) << 32)
            byte = lambda k: 0xFF if k >= 13 else (table >> (8 * k)) & 0xFF
            for cell in (0, 1, hxy * hz + hz + 1, 255):
                for r in range(9):
                    sel = 13 if r == 8 else r
                    perm = byte(sel) | (byte(0) << 8) | (byte(0) << 16) | (byte(0) << 24)
                    got = (cell + int(out[2]) + perm) & 0xFFFFFFFF
                    want = (cell + ((r // 3 - 1) * hxy + (r % 3 - 1)) * hz) & 0xFFFFFFFF
                    assert got == want, (txy, tz, r, cell, got, want)
    assert shapes == 24 + 14 + 8 + 5 + 3 + 2 + 1  # tz <= 256 / (txy + 2)^2 - 2 for txy = 1 ... 7


@gpu
@pytest.mark.parametrize("sigma", [0.0, 0.2], ids=["perfect", "rattled"])
def test_periodic_box_interior_and_seam_tiles(sigma):
    """interior tiles beside tiles on every seam; the rattle gives cells of more than four atoms (runs of more than 12 candidates:
    the general scan and its mask clean-up) and, out of lattice order, the compact grid"""
    pos, box, plan, counts, labels = _build_until_interior(("periodic", sigma), lambda n: _fcc(n, sigma))
    if sigma == 0.0:
        assert (counts == 12).all() and (labels == 1).all()
    else:
        perm = np.random.default_rng(3).permutation(len(pos))
        _both(("periodic, shuffled", sigma), np.ascontiguousarray(pos[perm]), box)
        assert counts.min() < 12 < counts.max()


@gpu
@pytest.mark.parametrize("bnd", [(0, 1, 1), (1, 1, 0), (0, 0, 0)], ids=["open_x", "open_z", "open_xyz"])
def test_open_boxes_face_tiles_keep_the_general_path(bnd):
    """atoms pushed outside an open face are clamped into the edge cells: a tile that touches such a cell must not take the short
    path (its atoms would lose the far-atom check), a tile one cell further in may"""
    bnd = np.array(bnd, np.int32)
    pos, box = _fcc(12, 0.05)
    rng = np.random.default_rng(4)
    out = rng.random(len(pos)) < 0.01  # a few atoms a little outside the box on the open axes
    for d in range(3):
        if not bnd[d]:
            pos[out, d] += np.where(pos[out, d] > 0.5 * box[d, d], 1.0, -1.0) * 0.9 * RC
    plan, counts, _ = _both(("open", bnd.tolist()), pos, box, bnd)
    nc = _cells(box, RC)
    assert _interior_tiles(plan, nc, bnd) > 0, plan.tolist()
    assert counts.min() < 12


@gpu
def test_atoms_handed_in_one_box_length_outside():
    """image codes present: such an atom is staged with its own image number in an interior tile as well"""
    pos, box = _fcc(12, 0.05)
    rng = np.random.default_rng(5)
    for d in range(3):
        far = rng.random(len(pos)) < 0.05
        pos[far, d] += rng.choice([-1.0, 1.0], far.sum()) * box[d, d]
    plan, counts, labels = _both("outside", pos, box)
    assert _interior_tiles(plan, _cells(box, RC), PBC) > 0
    assert (counts == 12).sum() > 0.9 * len(pos) and (labels == 1).sum() > 0.9 * len(pos)


@gpu
def test_slab_with_vacuum_list_mode():
    """a block in a box twice as high: the tiles that hold atoms come from a list"""
    pos, box = _fcc(12, 0.05)
    box = box.copy()
    box[2, 2] *= 2.0
    plan, counts, _ = _both("slab", pos, box)
    assert not (plan[4] & 1), ("the box counts as full of atoms", plan.tolist())
    assert _interior_tiles(plan, _cells(box, RC), PBC) > 0
    assert counts.min() < 12 and (counts == 12).any()


@gpu
def test_windowed_launch_with_a_centre_window():
    """a slab of a long box behind mdh_hint_cell_window, rows wanted for the planes of mdh_hint_centre_window only, as the decomposed
    step builds: the rows that are made are those of the thread-per-atom path on the same atoms without any hint, rows are made
    for every atom well inside the stretch and for none well outside it"""
    import torch

    pos, box = lattice_positions("fcc", A_CU, 40, 12, 12)
    box = np.asarray(box, float)
    pos = pos + np.random.default_rng(6).normal(0.0, 0.05, pos.shape)
    f = (pos[:, 0] / box[0, 0]) % 1.0
    pos = np.ascontiguousarray(pos[(f >= 0.30) & (f < 0.60)])
    f = (pos[:, 0] / box[0, 0]) % 1.0
    N, M = len(pos), 16
    L = _lib.lib()
    L.mdh_debug_set_neighbor_variant(1)
    try:
        ref = _fused(pos, box, PBC, RC, M)
    finally:
        L.mdh_debug_set_neighbor_variant(0)
    dev = torch.device("cuda", 0)
    x, y, z = (torch.from_numpy(np.ascontiguousarray(pos[:, k])).to(dev) for k in range(3))
    v = torch.full((N, M), -7, dtype=torch.int32, device=dev)
    d = torch.full((N, M), -7.0, dtype=torch.float64, device=dev)
    c = torch.full((N,), -7, dtype=torch.int32, device=dev)
    p = torch.zeros((N,), dtype=torch.int32, device=dev)
    _plan()
    lo, hi = 0.36, 0.54
    _neighbor.hint_cell_window(0, 0.28, 0.62)
    _neighbor.hint_centre_window(0, lo, hi)
    _neighbor.build_neighbor_fcna(x, y, z, box, ORG0, PBC, RC, v, d, c, p, 1, fill_pads=True)
    torch.cuda.synchronize()
    _neighbor.cell_window_check()
    plan = _plan()
    assert plan[0] > 0 and plan[7] == 1, plan.tolist()
    nc = _cells(box, RC)
    T = int(plan[0])
    planes = [t for t in range(0, nc[0], T) if t - 1 >= 0.28 * nc[0] + 1 and t + T + 1 <= 0.62 * nc[0] - 1 and t + T > lo * nc[0] and t < hi * nc[0]]
    assert planes and _interior_tiles(plan, nc, PBC) > 0, ("no interior tile inside the window", plan.tolist(), nc)
    v, d, c, p = v.cpu().numpy(), d.cpu().numpy(), c.cpu().numpy(), p.cpu().numpy()
    made = c != -7
    one = 1.0 / nc[0]
    assert made[(f >= lo + one) & (f < hi - one)].all() and not made[(f < lo - one) | (f >= hi + one)].any()
    assert 100 < made.sum() < N
    for name, a, b in zip(("verlet", "dist", "nn", "pattern"), (v, d, c, p), ref):
        assert np.array_equal(a[made], b[made]), (name, int((a[made] != b[made]).sum()))
    assert (p[~made] == 0).all()


@gpu
def test_sheared_box():
    """triclinic instances keep the general halo_of and the arithmetic run offset even in a tile that would count as interior;
    the mask clean-up and the grouped square-root test are theirs too"""
    def make(n):
        pos, box = _fcc(n, 0.05)
        sheared = box.copy()
        sheared[1, 0] = 0.2 * box[1, 1]
        sheared[2, 1] = -0.1 * box[2, 2]
        return np.ascontiguousarray(pos @ np.linalg.inv(box) @ sheared), sheared

    pos, box, plan, counts, labels = _build_until_interior("sheared", make, n0=13)
    assert (labels == 1).sum() > 0.9 * len(pos)


@gpu
def test_rows_of_twelve_slots():
    """M = 12: rows shorter than the hit count of some atoms, the last tickets of a row are run 8's only while they are listed"""
    pos, box = _fcc(12, 0.2, seed=7)
    plan, counts, _ = _both("M12", pos, box, M=12)
    assert _interior_tiles(plan, _cells(box, RC), PBC) > 0
    assert counts.max() > 12


@gpu
def test_bcc_block_fourteen_hits():
    """bcc with both neighbour shells inside rc: 14 hits, of which run 8 (the last of the walk) holds some — the tickets that
    the byte table answers with its selector past the table"""
    a = 2.87
    rc = 1.2 * a

    def make(n):
        pos, box = lattice_positions("bcc", a, n, n, n)
        return pos + np.random.default_rng(8).normal(0.0, 0.02, pos.shape), np.asarray(box, float)

    pos, box, plan, counts, labels = _build_until_interior("bcc", make, rc=rc, n0=17)
    assert (counts == 14).all() and len(np.unique(labels)) == 1 and labels[0] != 0
