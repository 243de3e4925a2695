"""Atomic strain on the GPU (mdapy_amd/csrc/strain.hip): every result bit for bit against the numpy restatement of the reference
(tests/_strain_ref.py) run on the list the System built — ``as_numpy`` of its rows and counts, in the compute view's
numbering — and the reference's own OVITO-derived fixture through ``AtomicStrain``."""
import os

import numpy as np
import pytest

import _strain_ref
import mdapy_amd as mp
from mdapy_amd import tool_function as tool
from mdapy_amd.build_lattice import lattice_positions
from mdapy_amd.devarray import as_numpy

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
GOLDEN = os.path.join(HERE, "golden", "strain")
A = 3.615
GRAD = np.array([[1.03, 0.0, 0.0], [0.04, 0.98, 0.0], [-0.02, 0.03, 1.01]])  # shear plus stretch of box and atoms


@pytest.fixture(autouse=True)
def _need_gpu():
    from mdapy_amd import _lib

    if _lib.device_count() < 1:
        pytest.fail("test_gpu_strain needs a HIP device")


def _columns(s):
    return s.data["shear_strain"].to_numpy(), s.data["volumetric_strain"].to_numpy()


def _check(strain, cur):
    """compute, and compare bitwise with the restatement on the reference system's own list"""
    strain.compute(cur)
    got, want = _columns(cur), _strain_ref.on_system_list(strain, cur)
    assert got[0].dtype == np.float64 and got[0].shape == (cur.N,) and got[1].shape == (cur.N,)
    assert np.array_equal(got[0], want[0], equal_nan=True), f"shear: {int((got[0] != want[0]).sum())} atoms differ"
    assert np.array_equal(got[1], want[1], equal_nan=True), f"volumetric: {int((got[1] != want[1]).sum())} atoms differ"
    return got


def _fcc(cells, seed, rattle=0.05):
    pos, box = lattice_positions("fcc", A, cells, cells, cells)
    return pos + np.random.default_rng(seed).normal(0, rattle, pos.shape), np.array(box, float)[:3]


def _deformed(pos, cell, seed, noise=0.03):
    return pos @ GRAD + np.random.default_rng(seed).normal(0, noise, pos.shape), cell @ GRAD


@pytest.mark.parametrize("affine", [False, True])
def test_rattled_fcc_under_shear_and_stretch(affine):
    pos, cell = _fcc(12, 0)
    moved, moved_cell = _deformed(pos, cell, 1)
    strain = mp.AtomicStrain(3.1, mp.System(pos=pos, box=cell), affine=affine)
    shear, vol = _check(strain, mp.System(pos=moved, box=mp.Box(moved_cell)))
    assert shear.min() > 0 and np.isfinite(vol).all()
    if affine:  # the homogeneous part is taken out: what is left is the rattle's
        assert shear.mean() < 0.05
    else:
        assert abs(vol.mean() - (np.trace(GRAD.T @ GRAD) - 3.0) / 6.0) < 5e-3


def test_purely_affine_deformation_has_no_affine_strain():
    pos, cell = _fcc(12, 2)
    moved, moved_cell = _deformed(pos, cell, 0, noise=0.0)
    strain = mp.AtomicStrain(3.1, mp.System(pos=pos, box=cell), affine=True)
    shear, vol = _check(strain, mp.System(pos=moved, box=mp.Box(moved_cell)))
    assert np.abs(shear).max() < 1e-12 and np.abs(vol).max() < 1e-12
    # and without the map every atom carries the strain of GRAD itself
    s = (GRAD.T @ GRAD - np.eye(3)) / 2.0
    shear, vol = _check(mp.AtomicStrain(3.1, mp.System(pos=pos, box=cell)), mp.System(pos=moved, box=mp.Box(moved_cell)))
    assert np.abs(vol - np.trace(s) / 3.0).max() < 1e-12


@pytest.mark.parametrize("affine", [False, True])
def test_triclinic_reference_box(affine):
    pos, cell = _fcc(10, 3)
    sheared = cell.copy()
    sheared[1, 0] = 0.3 * sheared[1, 1]
    sheared[2, 0], sheared[2, 1] = 0.2 * sheared[2, 2], -0.15 * sheared[2, 2]
    tri = (pos @ np.linalg.inv(cell)) @ sheared
    moved, moved_cell = _deformed(tri, sheared, 4)
    strain = mp.AtomicStrain(3.1, mp.System(pos=tri, box=mp.Box(sheared)), affine=affine)
    assert strain.ref.box.triclinic
    _check(strain, mp.System(pos=moved, box=mp.Box(moved_cell)))
    # a triclinic reference against an orthogonal current box, and the other way round
    _check(strain, mp.System(pos=pos + np.random.default_rng(5).normal(0, 0.03, pos.shape), box=mp.Box(cell)))
    back = mp.AtomicStrain(3.1, mp.System(pos=pos, box=mp.Box(cell)), affine=affine)
    _check(back, mp.System(pos=moved, box=mp.Box(moved_cell)))


@pytest.mark.parametrize("boundary", [[1, 1, 0], [0, 0, 1], [0, 0, 0]])
def test_open_boundaries_have_short_rows(boundary):
    pos, cell = _fcc(8, 6)
    moved, moved_cell = _deformed(pos, cell, 7)
    for affine in (False, True):
        ref = mp.System(pos=pos, box=mp.Box(cell, boundary))
        strain = mp.AtomicStrain(3.1, ref, affine=affine)
        counts = as_numpy(ref.neighbor_number)
        assert counts.min() <= 8 and counts.max() >= 12
        _check(strain, mp.System(pos=moved, box=mp.Box(moved_cell, boundary)))


def test_gas_with_empty_rows_and_the_identity_branch():
    rng = np.random.default_rng(0)
    pos = rng.random((1500, 3)) * 30.0
    moved = pos * 1.02 + rng.normal(0, 0.03, pos.shape)
    ref = mp.System(pos=pos, box=30.0)
    strain = mp.AtomicStrain(2.6, ref)
    cur = mp.System(pos=moved, box=30.0 * 1.02)
    shear, vol = _check(strain, cur)
    rows, counts = as_numpy(ref.verlet_list), as_numpy(ref.neighbor_number)
    V, W, used = _strain_ref.accumulate(rows, counts, ref.box.box, cur.box.box, ref.box.boundary, *pos.T, *moved.T)
    singular = _strain_ref.invariants(V, W)[2]
    assert np.array_equal(used, counts)
    # the seed gives all three kinds of row (checked on the CPU beforehand: 29 empty, 331 with one or two neighbours)
    assert (used == 0).sum() >= 10 and (singular & (used > 0)).sum() >= 100 and (~singular).sum() >= 1000
    assert (shear[used == 0] == 0.0).all() and (vol[used == 0] == -0.5).all()
    assert np.isfinite(shear).all() and np.isfinite(vol).all()
    _check(mp.AtomicStrain(2.6, mp.System(pos=pos, box=30.0), affine=True), mp.System(pos=moved, box=30.0 * 1.02))


@pytest.mark.parametrize("max_neigh", [None, 256, 251])
def test_wide_rows_take_several_chunks(max_neigh):
    rng = np.random.default_rng(3)
    pos = rng.random((1000, 3)) * 14.0
    moved = pos @ GRAD + rng.normal(0, 0.05, pos.shape)
    ref = mp.System(pos=pos, box=14.0)
    strain = mp.AtomicStrain(4.6, ref, max_neigh=max_neigh)
    assert ref.verlet_list.shape[1] > 64 and int(as_numpy(ref.neighbor_number).max()) > 64
    if max_neigh is not None:
        assert ref.verlet_list.shape[1] == max_neigh
    _check(strain, mp.System(pos=moved, box=mp.Box(np.eye(3) * 14.0 @ GRAD)))


@pytest.mark.parametrize("affine", [False, True])
def test_reference_fixture_end_to_end(affine):
    want = np.load(os.path.join(GOLDEN, "atomic_strain.npz"))
    ref = mp.System(os.path.join(GOLDEN, "strain.0.xyz"))
    cur = mp.System(os.path.join(GOLDEN, "strain.1.xyz"))
    strain = mp.AtomicStrain(float(want["cutoff"]), ref, max_neigh=30, affine=affine)
    shear, vol = _check(strain, cur)
    tag = "_affine" if affine else ""
    d_shear = float(np.abs(shear - want["shear_strain" + tag]).max())
    d_vol = float(np.abs(vol - want["volumetric_strain" + tag]).max())
    print(f"fixture affine={affine}: max |d shear| = {d_shear:.3e}, max |d volumetric| = {d_vol:.3e}")
    assert d_shear < 1e-12
    assert d_vol < 1e-12


def test_raw_shim_with_host_and_with_device_arrays():
    import torch

    from mdapy_amd import _strain
    from mdapy_amd.devarray import HArray

    pos, cell = _fcc(9, 8)
    moved, moved_cell = _deformed(pos, cell, 9)
    ref = mp.System(pos=pos, box=cell)
    ref.build_neighbor(3.3, max_neigh=27)
    rows, counts = as_numpy(ref.verlet_list), as_numpy(ref.neighbor_number)
    n = len(pos)
    origin, boundary = np.zeros(3), np.array([1, 1, 1], np.int32)
    cols = [np.ascontiguousarray(a[:, k]) for a in (pos, moved) for k in range(3)]
    boxes = (cell, moved_cell, origin, origin, boundary)
    want = np.empty(n), np.empty(n)
    _strain_ref.cal_atomic_strain(rows, counts, *boxes, *cols, *want)
    host = np.full(n, 7.0), np.full(n, 7.0)
    _strain.cal_atomic_strain(rows, counts, *boxes, *cols, *host, 4)
    assert np.array_equal(host[0], want[0]) and np.array_equal(host[1], want[1])
    up = lambda a: HArray(torch.from_numpy(np.ascontiguousarray(a)).cuda())
    dev = HArray.empty((n,), np.float64), HArray.empty((n,), np.float64)
    _strain.cal_atomic_strain(ref.verlet_list, ref.neighbor_number, *boxes, *(up(c) for c in cols), *dev)
    assert np.array_equal(dev[0].numpy(), want[0]) and np.array_equal(dev[1].numpy(), want[1])
    # device rows with host columns and host outputs
    mixed = np.empty(n), np.empty(n)
    _strain.cal_atomic_strain(ref.verlet_list, ref.neighbor_number, *boxes, *cols, *mixed)
    assert np.array_equal(mixed[0], want[0]) and np.array_equal(mixed[1], want[1])
    # the map in the kernel equals the map on the host
    mapped = _strain_ref.affine_mapped(moved_cell, cell, *cols[3:])
    boxes_affine = (cell, cell, origin, origin, boundary)
    _strain_ref.cal_atomic_strain(rows, counts, *boxes_affine, *cols[:3], *mapped, *want)
    _strain.cal_atomic_strain(rows, counts, *boxes_affine, *cols, *host, affine_map=np.linalg.solve(moved_cell, cell))
    assert np.array_equal(host[0], want[0]) and np.array_equal(host[1], want[1])
    # records made once, on the host and in HBM, give the same bits
    for space in (lambda a: a, up):
        ref_records = _strain.pack_records(*(space(c) for c in cols[:3]))
        cur_records = _strain.pack_records(*(space(c) for c in cols[3:]), np.linalg.solve(moved_cell, cell))
        assert tuple(ref_records.shape) == (n, 4) and np.array_equal(as_numpy(ref_records)[:, :3], pos)
        assert np.array_equal(as_numpy(cur_records)[:, :3], np.column_stack(mapped))
        out = np.empty(n), np.empty(n)
        _strain.cal_atomic_strain_records(space(rows), space(counts), *boxes_affine, ref_records, cur_records, *out)
        assert np.array_equal(out[0], want[0]) and np.array_equal(out[1], want[1])
    with pytest.raises(ValueError):
        _strain.cal_atomic_strain(rows, counts, *boxes, *cols[:5], cols[5][:-1], *host)
    with pytest.raises(ValueError):
        _strain.cal_atomic_strain_records(rows, counts, *boxes, as_numpy(ref_records)[:-1], as_numpy(ref_records), *host)


def test_one_reference_against_a_sequence_of_frames():
    """the packed reference records are state that outlives a call: five different frames through one object, each equal to the
    restatement on that frame alone, with the map on and off in two objects that share the reference System"""
    pos, cell = _fcc(11, 10)
    ref = mp.System(pos=pos, box=cell)
    plain, mapped = mp.AtomicStrain(3.1, ref), mp.AtomicStrain(3.1, ref, affine=True)
    rng = np.random.default_rng(11)
    drifted = pos + rng.normal(0, 0.04, pos.shape)
    other_box = _deformed(pos, cell, 12)
    squeezed = (pos * 0.97 + rng.normal(0, 0.02, pos.shape), cell * 0.97)
    frames = [(drifted, cell), other_box, (drifted, cell), squeezed, (pos, cell)]
    seen = []
    for k, (xyz, box) in enumerate(frames):
        for strain in (plain, mapped) if k % 2 == 0 else (mapped, plain):
            got = _check(strain, mp.System(pos=xyz, box=mp.Box(box)))
            seen.append((k, strain.affine, got))
        assert plain._packed is not None and mapped._packed is not None
        if k == 0:
            records = plain._packed[1]
        assert plain._packed[1] is records  # packed once
    first = {a: g for k, a, g in seen if k == 0}
    again = {a: g for k, a, g in seen if k == 2}
    for a in (False, True):
        assert np.array_equal(first[a][0], again[a][0]) and np.array_equal(first[a][1], again[a][1])
    same = [g for k, a, g in seen if k == 4 and not a][0]  # the reference against itself
    assert np.abs(same[0]).max() < 1e-12 and np.abs(same[1]).max() < 1e-12
    # a new list on the reference System: the records follow it
    ref.build_neighbor(4.0)
    _check(plain, mp.System(pos=drifted, box=mp.Box(cell)))
    assert plain._packed[1] is not records


def test_current_columns_in_hbm_equal_host_columns():
    import torch

    from mdapy_amd.devarray import HArray
    from mdapy_amd.frame import Frame

    pos, cell = _fcc(10, 13)
    moved, moved_cell = _deformed(pos, cell, 14)
    strain = mp.AtomicStrain(3.1, mp.System(pos=pos, box=cell), affine=True)
    host = _check(strain, mp.System(pos=moved, box=mp.Box(moved_cell)))
    cols = {c: HArray(torch.from_numpy(np.ascontiguousarray(moved[:, k])).cuda()) for k, c in enumerate("xyz")}
    cur = mp.System(data=Frame(cols), box=mp.Box(moved_cell))
    strain.compute(cur)
    assert cur.data["shear_strain"]._host_arr is None  # the result stays in HBM until it is read
    dev = _columns(cur)
    assert np.array_equal(host[0], dev[0]) and np.array_equal(host[1], dev[1])


@pytest.mark.parametrize("affine", [False, True])
def test_shuffled_frames_run_on_the_twin_without_translating_its_rows(affine):
    from mdapy_amd import _twin as twin_mod
    from mdapy_amd.devarray import LazyHArray

    cells = 37
    pos, cell = _fcc(cells, 15)
    assert len(pos) >= twin_mod.SORT_MIN_ATOMS
    moved, moved_cell = _deformed(pos, cell, 16)
    order = np.random.default_rng(17).permutation(len(pos))
    ref = mp.System(pos=pos[order], box=cell)
    strain = mp.AtomicStrain(3.1, ref, affine=affine)
    assert ref._spatial() is not None, "the shuffled reference has a cell-sorted twin"
    shown = ref._twin.shown
    assert shown.mirror is ref.verlet_list and isinstance(ref.verlet_list, LazyHArray)
    cur = mp.System(pos=moved[order], box=mp.Box(moved_cell))
    strain.compute(cur)
    second = mp.System(pos=(moved + 0.01)[order], box=mp.Box(moved_cell))
    strain.compute(second)
    assert not ref.verlet_list.produced and not ref.distance_list.produced, "compute translated the N x M rows of the mirror"
    assert ref._twin.shown is shown
    # now the rows are read (and translated): the restatement in the shuffled numbering
    for frame in (cur, second):
        got, want = _columns(frame), _strain_ref.on_system_list(strain, frame)
        assert np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1])
    assert ref.verlet_list.produced


@pytest.mark.parametrize("affine", [False, True])
def test_small_periodic_box_equals_the_replicated_pair(affine):
    pos, box = lattice_positions("fcc", A, 2, 2, 6)  # 7.23 A across x and y: a 3.7 A list is built on a 2 x 2 x 1 replica
    cell = np.array(box, float)[:3]
    pos = pos + np.random.default_rng(18).normal(0, 0.05, pos.shape)
    moved, moved_cell = _deformed(pos, cell, 19)
    ref = mp.System(pos=pos, box=cell)
    strain = mp.AtomicStrain(3.7, ref, affine=affine)
    assert "_enlarge_data" in ref.__dict__ and tuple(int(c) for c in strain.repeat) == (2, 2, 1)
    cur = mp.System(pos=moved, box=mp.Box(moved_cell))
    got = _check(strain, cur)
    big_ref = mp.System(pos=ref._enlarge_data.select("x", "y", "z").to_numpy(), box=ref._enlarge_box)
    big_data, big_box = tool._replicate_pos(cur.data, cur.box, 2, 2, 1)
    big_cur = mp.System(pos=big_data.select("x", "y", "z").to_numpy(), box=big_box)
    big = mp.AtomicStrain(3.7, big_ref, affine=affine)
    assert "_enlarge_data" not in big_ref.__dict__
    want = _check(big, big_cur)
    n = len(pos)
    assert np.array_equal(got[0], want[0][:n]) and np.array_equal(got[1], want[1][:n])
    assert got[0].max() > 1e-3
