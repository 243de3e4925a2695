"""CHILL+ on the GPU (mdapy_amd/csrc/chill.hip) against the float64 restatement of tests/_chill_ref.py run on the list the
System built, under the parity rule stated there: every atom none of whose bonds has c within 5e-6 of a threshold carries the
yardstick's label, and at most 0.5 % of the atoms are that close.  The reference's OVITO-derived fixture keeps 9.8e-6 clear of
every threshold, so it is compared exactly; so are perfect crystals and everything that compares the kernel with itself."""
import os

import numpy as np
import pytest

import _chill_ref
import mdapy_amd as mp
from mdapy_amd.build_lattice import lattice_positions
from mdapy_amd.devarray import as_numpy

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
GOLDEN = os.path.join(HERE, "golden", "chill", "chill_water.npz")
A = 6.37
ROW_CHUNK = 16  # csrc/common.hpp


@pytest.fixture(autouse=True)
def _need_gpu():
    from mdapy_amd import _lib

    if _lib.device_count() < 1:
        pytest.fail("test_gpu_chill needs a HIP device")


def _labels(s):
    return s.data["chill_plus"].to_numpy()


def _water():
    want = np.load(GOLDEN)
    return mp.System(pos=want["pos"], box=mp.Box(want["box"], want["boundary"])), want["chill_plus"], float(want["chill_plus_cutoff"])


_ICE = {}


def _ice(sigma, seed):
    """5 x 5 x 5 cells of cubic ice (1000 sites) with N(0, sigma) noise — made once per (sigma, seed) and never written to"""
    if (sigma, seed) not in _ICE:
        pos, box = lattice_positions("diamond", A, 5, 5, 5)
        pos = pos + np.random.default_rng(seed).normal(0, sigma, pos.shape)
        pos.setflags(write=False)
        _ICE[sigma, seed] = pos, np.array(box, float)[:3]
    return _ICE[sigma, seed]


def _check(s, cutoff=3.5, what=""):
    """cal_chill_plus, and the parity rule against the yardstick on the system's own list"""
    s.cal_chill_plus(cutoff)
    want, c, ambiguous = _chill_ref.on_system_list(s, cutoff)
    got = _labels(s)
    _chill_ref.check(got, want, ambiguous, what)
    return got, want, c


def test_reference_fixture_through_system():
    s, want, cutoff = _water()
    s.cal_chill_plus(cutoff)
    assert s.data["chill_plus"]._host_arr is None  # the labels stay in HBM until they are read
    got = _labels(s)
    assert got.dtype == np.int32 and got.shape == (8000,)
    assert np.array_equal(got, want), f"{int((got != want).sum())} of 8000 labels differ from the stored ones"
    assert np.bincount(got, minlength=6).tolist() == [4392, 553, 517, 2305, 20, 213]


def test_reference_fixture_through_the_bare_shim_host_and_device_arrays():
    import torch

    from mdapy_amd import _chill_plus
    from mdapy_amd.devarray import HArray

    s, want, cutoff = _water()
    s.build_neighbor(cutoff)
    cols = [np.ascontiguousarray(s.data[k].to_numpy()) for k in "xyz"]
    box = (s.box.box, s.box.origin, s.box.boundary)
    rows, dist, counts = as_numpy(s.verlet_list), as_numpy(s.distance_list), as_numpy(s.neighbor_number)
    host = np.full(8000, 7, np.int32)
    _chill_plus.compute_chill_plus(*cols, *box, rows, dist, counts, cutoff, host, 4)
    assert np.array_equal(host, want)
    up = lambda a: HArray(torch.from_numpy(np.ascontiguousarray(a)).cuda())
    dev = HArray.empty((8000,), np.int32)
    _chill_plus.compute_chill_plus(*(up(c) for c in cols), *box, s.verlet_list, s.distance_list, s.neighbor_number, cutoff, dev)
    assert np.array_equal(dev.numpy(), want)
    with pytest.raises(ValueError):
        _chill_plus.compute_chill_plus(*cols, *box, rows, dist, counts[:-1], cutoff, host)
    with pytest.raises(ValueError):
        _chill_plus.compute_chill_plus(*cols, *box, rows, dist, counts, 0.0, host)
    with pytest.raises(ValueError):
        _chill_plus.compute_chill_plus(*cols, *box, rows[:, :0], dist[:, :0], counts, cutoff, host)


@pytest.mark.parametrize("structure, a, cells, code", [("diamond", A, 1, 2), ("diamond", A, 2, 2), ("lonsdaleite", 4.5, 1, 1),
                                                       ("lonsdaleite", 4.5, 2, 1)])
def test_perfect_ice(structure, a, cells, code):
    s = mp.build_crystal("O", structure, a, nx=cells, ny=cells, nz=cells)
    s.cal_chill_plus(3.5)
    if cells == 1:
        assert "_enlarge_data" in s.__dict__  # thinner than two cutoffs: the list is the replica's
    got = _labels(s)
    assert got.dtype == np.int32 and got.shape == (s.N,) and s.N == (8 if structure == "diamond" else 4) * cells ** 3
    assert (got == code).all(), np.bincount(got, minlength=6).tolist()
    want, _, ambiguous = _chill_ref.on_system_list(s, 3.5)
    assert np.array_equal(got, want) and not ambiguous.any()


@pytest.mark.parametrize("sigma, seed", [(0.15, 1), (0.30, 2)])
def test_noisy_ice(sigma, seed):
    pos, cell = _ice(sigma, seed)
    got, want, c = _check(mp.System(pos=pos, box=cell), what=f"noisy ice sigma={sigma}")
    if sigma == 0.30:
        coordination = (~np.isnan(c)).sum(axis=1)
        assert (np.bincount(want, minlength=6) > 0).sum() >= 5 and coordination.min() <= 2 and coordination.max() >= 6


def test_noisy_ice_in_a_triclinic_box():
    pos, cell = _ice(0.30, 2)
    sheared = cell.copy()
    sheared[1, 0] = 0.3 * sheared[1, 1]
    sheared[2, 0], sheared[2, 1] = 0.2 * sheared[2, 2], -0.15 * sheared[2, 2]
    s = mp.System(pos=(pos @ np.linalg.inv(cell)) @ sheared, box=mp.Box(sheared))
    assert s.box.triclinic
    got, want, _ = _check(s, what="triclinic")
    assert (np.bincount(want, minlength=6) > 0).sum() >= 3


@pytest.mark.parametrize("boundary", [[1, 1, 0], [0, 0, 1], [0, 0, 0]])
def test_noisy_ice_with_open_boundaries(boundary):
    pos, cell = _ice(0.30, 2)
    s = mp.System(pos=pos, box=mp.Box(cell, boundary))
    _check(s, what=f"boundary {boundary}")
    assert int(as_numpy(s.neighbor_number).min()) <= 2  # surface atoms have short rows


def test_gas_with_empty_rows():
    pos = np.random.default_rng(7).random((1500, 3)) * 36.0
    s = mp.System(pos=pos, box=36.0)
    got, want, c = _check(s, what="gas")
    counts = as_numpy(s.neighbor_number)
    assert counts.min() == 0 and counts.max() == 15 and s.verlet_list.shape == (1500, 15) and (got[counts == 0] == 0).all()
    assert np.array_equal((~np.isnan(c)).sum(axis=1), counts)


def test_rows_longer_than_one_staged_chunk():
    pos, cell = _ice(0.30, 2)
    s = mp.System(pos=pos, box=cell)
    s.build_neighbor(5.0)
    rows = s.verlet_list
    assert rows.shape[1] > ROW_CHUNK
    s.cal_chill_plus(3.5)
    assert s.verlet_list is rows and s.rc == 5.0  # reused, not rebuilt
    fresh = mp.System(pos=pos, box=cell)
    fresh.cal_chill_plus(3.5)
    assert fresh.verlet_list.shape[1] <= ROW_CHUNK
    assert np.array_equal(_labels(s), _labels(fresh))  # the entries beyond 3.5 are passed over, wherever they sit in a row
    _chill_ref.check(_labels(s), *_chill_ref.on_system_list(s, 3.5)[::2], "wide rows")


def _shim(pos, cell, rows, dist, counts, rc=3.5):
    from mdapy_amd import _chill_plus

    cols = [np.ascontiguousarray(pos[:, k]) for k in range(3)]
    box = (np.ascontiguousarray(cell), np.zeros(3), np.array([1, 1, 1], np.int32))
    got = np.full(len(pos), 7, np.int32)
    _chill_plus.compute_chill_plus(*cols, *box, rows, dist, counts, rc, got)
    want, c, ambiguous = _chill_ref.analyse(*cols, *box, rows, dist, counts, rc)
    return got, want, c, ambiguous


def test_row_semantics_on_a_hand_made_list():
    pos, cell = _ice(0.15, 1)
    s = mp.System(pos=pos, box=cell)
    s.build_neighbor(3.5)
    rows, dist, counts = (np.array(as_numpy(a)) for a in (s.verlet_list, s.distance_list, s.neighbor_number))
    assert rows.shape[1] >= 4 and (counts == 4).mean() > 0.9
    base = _shim(pos, cell, rows, dist, counts)
    _chill_ref.check(*base[:2], base[3], "hand-made: as built")
    assert (base[0] == 2).mean() > 0.5
    four = np.flatnonzero(counts == 4)

    # neighbor_number cut below the filled length: the entries behind it are no bonds
    cut = counts.copy()
    cut[four[::2]] = 3
    got, want, c, ambiguous = _shim(pos, cell, rows, dist, cut)
    _chill_ref.check(got, want, ambiguous, "hand-made: counts cut")
    assert ((~np.isnan(c)).sum(axis=1)[four[::2]] == 3).all() and (got[four[::2]] == 0).all()

    # a -1 in the middle of a row, followed by valid entries: passed over, the row goes on
    holed = rows.copy()
    holed[four[::3], 1] = -1
    got, want, c, ambiguous = _shim(pos, cell, holed, dist, counts)
    _chill_ref.check(got, want, ambiguous, "hand-made: -1 in the middle")
    assert ((~np.isnan(c)).sum(axis=1)[four[::3]] == 3).all() and (got[four[::3]] == 0).all()

    # an entry with distance > rc between valid ones
    far = dist.copy()
    far[four[1::3], 2] = 3.6
    got, want, c, ambiguous = _shim(pos, cell, rows, far, counts)
    _chill_ref.check(got, want, ambiguous, "hand-made: a far entry in the middle")
    assert ((~np.isnan(c)).sum(axis=1)[four[1::3]] == 3).all() and (got[four[1::3]] == 0).all()

    # M = 1: nobody has four bonds
    got, want, c, ambiguous = _shim(pos, cell, np.ascontiguousarray(rows[:, :1]), np.ascontiguousarray(dist[:, :1]), np.minimum(counts, 1))
    _chill_ref.check(got, want, ambiguous, "hand-made: M = 1")
    assert (got == 0).all()

    # N = 1: an atom bonded four times to itself (d = 0 adds nothing to q: c = 0, four eclipsed bonds)
    one = _shim(pos[:1], cell, np.zeros((1, 4), np.int32), np.zeros((1, 4)), np.array([4], np.int32))
    assert one[0].tolist() == one[1].tolist() == [4]
    one = _shim(pos[:1], cell, np.full((1, 4), -1, np.int32), np.full((1, 4), 4.5), np.array([0], np.int32))
    assert one[0].tolist() == one[1].tolist() == [0]


def test_an_index_beyond_the_system_never_faults():
    """an entry >= N that is not negative reads the atom itself (safe_id) and counts as a bond; the reference reads out of bounds
    there, so only this is pinned: the call returns, every code is one of the six, and rows without such an entry keep their label"""
    from mdapy_amd import _chill_plus

    pos, cell = _ice(0.15, 1)
    s = mp.System(pos=pos, box=cell)
    s.build_neighbor(3.5)
    rows, dist, counts = (np.array(as_numpy(a)) for a in (s.verlet_list, s.distance_list, s.neighbor_number))
    base = _shim(pos, cell, rows, dist, counts)[0]
    wild = rows.copy()
    wild[::29, 0] = len(pos)
    wild[3::29, 1] = np.iinfo(np.int32).max
    got = np.full(len(pos), 7, np.int32)
    cols = [np.ascontiguousarray(pos[:, k]) for k in range(3)]
    _chill_plus.compute_chill_plus(*cols, np.ascontiguousarray(cell), np.zeros(3), np.array([1, 1, 1], np.int32), wild, dist, counts, 3.5, got)
    assert got.dtype == np.int32 and ((got >= 0) & (got <= 5)).all()
    touched = (wild != rows).any(axis=1)
    touched |= np.isin(rows, np.flatnonzero(touched)).any(axis=1)  # (a changed atom's q reaches its neighbours' c)
    assert (~touched).sum() > 100 and np.array_equal(got[~touched], base[~touched])


def test_shuffled_atoms_on_the_twin_and_off_it():
    pos, cell = _ice(0.30, 2)
    plain = mp.System(pos=pos, box=cell)
    plain.cal_chill_plus()
    order = np.random.default_rng(3).permutation(len(pos))
    got = {}
    for mode in ("1", "0"):
        os.environ["MDAPY_SPATIAL_SORT"] = mode
        try:
            s = mp.System(pos=pos[order], box=cell)
        finally:
            del os.environ["MDAPY_SPATIAL_SORT"]
        assert (s._spatial() is not None) == (mode == "1")
        s.cal_chill_plus()
        got[mode] = _labels(s)
        if mode == "1":
            assert s._twin.shown.mirror is s.verlet_list
        _chill_ref.check(got[mode], *_chill_ref.on_system_list(s, 3.5)[::2], f"shuffled, sort={mode}")
    # the twin's rows are keyed by the original index: the same sums in the same order, the same labels bit for bit
    assert np.array_equal(got["1"], got["0"])
    # and both are the unshuffled labels put through the permutation (the bonds of a row come in another order there: the sums
    # differ in their last bits, which moves no c of this input across a threshold)
    assert np.array_equal(got["1"], _labels(plain)[order])


def test_a_second_frame_on_the_same_system():
    first, cell = _ice(0.15, 1)
    second, _ = _ice(0.30, 2)
    s = mp.System(pos=first, box=cell)
    s.cal_chill_plus()
    before = _labels(s).copy()
    frame = s.data.with_columns(x=second[:, 0].copy(), y=second[:, 1].copy(), z=second[:, 2].copy())
    s.update_data(frame, reset_neighbor=True)
    assert "verlet_list" not in s.__dict__
    s.cal_chill_plus()
    fresh = mp.System(pos=second, box=cell)
    fresh.cal_chill_plus()
    assert np.array_equal(_labels(s), _labels(fresh)) and (before != _labels(s)).any()
