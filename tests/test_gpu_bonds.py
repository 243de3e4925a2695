"""Bond pairs and chemical species on the GPU: mdh_build_bond, mdh_cluster_composition and mdh_species_match against the numpy
restatements of tests/_bond_pairs_ref.py — the reference's rule taken literally: all rows, ``% N``, ``sort(axis=1)``, self pairs
dropped, ``np.unique``.  Everything is integers; the one float operation is ``dist <= cutoff`` on numbers the list already
holds, so every comparison is ``np.array_equal``."""
import ctypes
import gzip
import os

import numpy as np
import pytest

import _bond_pairs_ref as ref
import mdapy_amd as mp
from mdapy_amd import _lib, kernels
from mdapy_amd.devarray import HArray, as_numpy
from mdapy_amd.system import _normalize_bond_cutoff

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "bond")
SCAN_BLOCK = 256 * 4  # items per block of exclusive_scan_u32 below 2^19 items (csrc/cell_grid.hip: SCAN_BLOCK x SCAN_ITEMS)
SIZES = (0, 1, 63, 64, 65, 2 * SCAN_BLOCK + 77)  # the last: three blocks of the scan over the per-row counts
WIDTHS = (1, 7, 16, 64, 65, 100)  # groups of 8, 8, 16 and 64 lanes; 65 and 100: the path over chunks of 64
CUT3 = np.array([[0.9, 1.4, 0.6], [1.4, 1.1, 1.7], [0.6, 1.7, 1.2]])  # symmetric, every row another order


def _list(N, M, seed, ntype=3, bad_types=False, garbage=-1):
    """a synthetic (N, M) list: random entries (a row may name an atom twice, itself, or nobody: -1), random counts, and behind
    a row's count -1 or garbage"""
    rng = np.random.default_rng(seed)
    rows = rng.integers(-1, max(N, 1), (N, M)).astype(np.int32)
    dist = rng.random((N, M)) * 2.0
    nn = rng.integers(0, M + 1, N).astype(np.int32)
    nn[::7] = 0
    nn[3::7] = M
    beyond = np.arange(M)[None, :] >= nn[:, None]
    if garbage == -1:
        rows[beyond] = -1
    else:  # whatever: indices far outside the list, distances that would bond
        rows[beyond] = rng.choice(np.array([2 ** 30, -2 ** 31, N, N + 5, 0], np.int64), int(beyond.sum())).astype(np.int32)
        dist[beyond] = 0.0
    types = rng.integers(-1 if bad_types else 0, ntype + (1 if bad_types else 0), N).astype(np.int32)
    return rows, dist, nn, types


def _both_ways(rows, dist, nn, types, cut, n_real=0):
    """the shim with the list in HBM and with host arrays (staged by the library): the same bits"""
    want = ref.build_bond(rows, dist, nn, types, cut, 1, n_real)
    dev = [None if a is None else HArray.from_numpy(a) for a in (rows, dist, nn, types)]
    got = kernels.build_bond.build_bond(*dev, cut, 1, n_real)
    assert isinstance(got, HArray) and got.dtype == np.int32 and got.shape == want.shape
    assert np.array_equal(as_numpy(got), want)
    host = kernels.build_bond.build_bond(rows, dist, nn, types, cut, 1, n_real)
    assert isinstance(host, np.ndarray) and host.dtype == np.int32 and np.array_equal(host, want)
    return want


@pytest.mark.parametrize("M", WIDTHS)
def test_synthetic_lists(M):
    seen = 0
    for N in SIZES:
        rows, dist, nn, types = _list(N, M, seed=N + M, garbage=(N + M) % 2 - 1)
        seen += len(_both_ways(rows, dist, nn, types, CUT3))
        seen += len(_both_ways(rows, dist, nn, None, np.array([[1.0]])))  # ntype 1, no type array
    assert seen > 50


@pytest.mark.parametrize("M", WIDTHS)
def test_types_out_of_range_and_rows_without_a_bond(M):
    N = 200
    rows, dist, nn, types = _list(N, M, seed=11 * M, bad_types=True, garbage=0)
    assert (types < 0).any() and (types >= 3).any()
    dist[::2] = 5.0  # every other row: nothing qualifies
    want = _both_ways(rows, dist, nn, types, CUT3)
    if M > 1:
        assert len(want) > 0
    assert not np.isin(want[:, 0], np.arange(0, N, 2)).any()
    # no bonds at all
    none = _both_ways(rows, np.full_like(dist, 5.0), nn, types, CUT3)
    assert none.shape == (0, 2)


@pytest.mark.parametrize("M", (7, 64, 100))
def test_ties_descending_keys_and_duplicates(M):
    N = 150
    rng = np.random.default_rng(M)
    # every row lists M atoms in DESCENDING order, half of them twice over; distances exactly at, just under and just over the cutoff
    rows = np.empty((N, M), np.int32)
    for i in range(N):
        picks = np.sort(rng.choice(N, M, replace=M > N))[::-1]
        picks[1::4] = picks[0::4][:len(picks[1::4])]
        rows[i] = picks
    cut = np.array([[1.25, 0.75], [0.75, 1.5]])
    types = rng.integers(0, 2, N).astype(np.int32)
    limit = cut[types[:, None], types[rows]]
    dist = np.where(rng.random((N, M)) < 0.4, limit, np.where(rng.random((N, M)) < 0.5, np.nextafter(limit, 0.0), np.nextafter(limit, 9.0)))
    nn = np.full(N, M, np.int32)
    want = _both_ways(rows, dist, nn, types, cut)
    assert len(want) > N  # (ties count as bonded)
    assert len(want) < int(((rows > np.arange(N)[:, None]) & (dist <= limit)).sum())  # (a key a row holds twice is listed once)
    assert np.array_equal(want, np.unique(want, axis=0))


def _replica_list(n, copies, M, seed):
    """a list as one built on an enlarged periodic box is: copy c of atom a is entry c * n + a; SYMMETRIC (whatever row i says of
    j, row j says of i, at the same distance) and invariant under the replica's translations (row (c, a) is row (0, a) shifted by
    c copies) — with several images of one atom inside a row and images of the row's own atom; slots in random order"""
    rng = np.random.default_rng(seed)
    out = [[] for _ in range(n)]  # row (0, a): (shift, atom, distance)
    for _ in range(n * M):
        a, b, s, d = int(rng.integers(n)), int(rng.integers(n)), int(rng.integers(copies)), float(rng.random() * 2.0)
        if rng.random() < 0.3 and out[a]:
            b = out[a][int(rng.integers(len(out[a])))][1]  # another image of an atom the row already holds
        back = (-s) % copies
        if a == b and s == 0:
            continue
        both = [(a, (s, b, d)), (b, (back, a, d))]
        if a == b and back == s:
            both = both[:1]
        if len(out[a]) + (2 if a == b and len(both) == 2 else 1) > M or len(out[b]) + 1 > M or (a, (s, b)) in [(a, e[:2]) for e in out[a]]:
            continue
        for row, entry in both:
            out[row].append(entry)
    N = n * copies
    rows, dist, nn = np.full((N, M), -1, np.int32), np.full((N, M), 0.01), np.zeros(N, np.int32)
    for a in range(n):
        order = rng.permutation(len(out[a]))
        for c in range(copies):
            i = c * n + a
            nn[i] = len(order)
            for q, k in enumerate(order):
                s, b, d = out[a][k]
                rows[i, q], dist[i, q] = ((s + c) % copies) * n + b, d
    return rows, dist, nn, np.tile(rng.integers(0, 3, n).astype(np.int32), copies)


@pytest.mark.parametrize("M", (7, 16, 64, 100))
def test_replica_mode(M):
    """the kernel reads the rows of the n real atoms and names a neighbour by the atom it copies; the restatement reads all rows,
    takes % n, sorts the two ends, drops self pairs and takes np.unique"""
    n, copies = 37, 4
    rows, dist, nn, types = _replica_list(n, copies, M, seed=100 + M)
    assert np.array_equal(rows[n:2 * n][rows[n:2 * n] >= 0] % n, rows[:n][rows[:n] >= 0] % n) and nn.max() == M
    keys = np.where(rows[:n] >= 0, rows[:n] % n, -1)
    assert any(len(set(r[r >= 0].tolist())) < (r >= 0).sum() for r in keys)  # (two images of one atom inside a row)
    assert (keys == np.arange(n)[:, None]).any()  # (an image of the row's own atom)
    want = _both_ways(rows, dist, nn, types, CUT3, n_real=n)
    assert len(want) > 20 and want.max() < n and np.all(want[:, 0] < want[:, 1])
    plain = ref.build_bond(rows, dist, nn, types, CUT3)  # (the same list read as a plain one has the copies' pairs as well)
    assert len(plain) > len(want)


def test_capacity_protocol():
    import torch

    rows, dist, nn, types = _list(500, 16, seed=8)
    want = ref.build_bond(rows, dist, nn, types, CUT3)
    total = len(want)
    assert total > 20
    dev = [torch.from_numpy(a).cuda() for a in (rows, dist, nn, types)]
    L, count = _lib.lib(), ctypes.c_int64(-1)
    stream = torch.cuda.current_stream().cuda_stream
    args = (dev[0].data_ptr(), dev[1].data_ptr(), dev[2].data_ptr(), 500, 16, dev[3].data_ptr(), CUT3.ctypes.data, 3, 0)
    assert L.mdh_build_bond(*args, None, 0, ctypes.addressof(count), _lib.DEVICE, stream) == 0 and count.value == total
    out = torch.full((total + 1, 2), -7, dtype=torch.int32, device="cuda")
    count.value = -1
    assert L.mdh_build_bond(*args, out.data_ptr(), total, ctypes.addressof(count), _lib.DEVICE, stream) == 0 and count.value == total
    got = out.cpu().numpy()
    assert np.array_equal(got[:total], want) and np.all(got[total] == -7)  # (cap == count: filled, nothing behind it touched)
    out.fill_(-7)
    count.value = -1
    assert L.mdh_build_bond(*args, out.data_ptr(), total - 1, ctypes.addressof(count), _lib.DEVICE, stream) == _lib.ERR_ARG
    assert count.value == total and b"room for" in L.mdh_last_error()  # (one short: the error, the count still delivered)
    assert np.all(out.cpu().numpy() == -7)


# ---- System
def _line(**extra):
    data = {"x": [0.0, 1.0, 2.3, 5.0], "y": [0.0] * 4, "z": [0.0] * 4}
    data.update(extra)
    return mp.System(data=data, box=mp.Box([10.0, 10.0, 10.0], boundary=[0, 0, 0]))


def test_reference_cases():
    system = _line(type=[1, 2, 2, 1])
    bond = system.create_bonds(1.5)
    assert np.array_equal(bond, np.array([[0, 1], [1, 2]], np.int32)) and system.bond is bond and bond.dtype == np.int32
    assert np.array_equal(_line(type=[1, 2, 2, 1]).create_bonds({(1, 1): 0.5, (1, 2): 1.1, (2, 2): 1.2}), [[0, 1]])
    cut = {("Cu", "Cu"): 0.5, ("Cu", "Zr"): 1.1, ("Zr", "Zr"): 1.2}
    assert np.array_equal(_line(element=["Cu", "Zr", "Zr", "Cu"]).create_bonds(cut), [[0, 1]])
    small = mp.System(pos=np.array([[0.0, 0.0, 0.0], [1.0, 0.0, 0.0]]), box=mp.Box([2.0, 2.0, 2.0]))
    assert np.array_equal(small.create_bonds(1.1), [[0, 1]]) and "_enlarge_data" in small.__dict__
    none = _line().create_bonds(0.5)
    assert isinstance(none, np.ndarray) and none.shape == (0, 2) and none.dtype == np.int32
    pair = mp.System(pos=np.array([[1.0, 0, 0], [1.05, 0, 0], [5.0, 0, 0]]), box=mp.Box([20.0, 20.0, 20.0]))
    pair.create_bonds(0.5)
    assert np.array_equal(pair.bond, [[0, 1]])
    pair.delete_overlap(0.1)
    assert not hasattr(pair, "bond") and not hasattr(pair, "verlet_list")


BOXES = {
    "orthogonal": (np.diag([13.7, 17.2, 29.9]), [1, 1, 1]),
    "triclinic": (np.array([[14.0, 0.0, 0.0], [3.1, 17.0, 0.0], [-2.2, 4.0, 21.0]]), [1, 1, 1]),
    "open_axis": (np.diag([13.7, 17.2, 29.9]), [1, 0, 1]),
    "thin": (np.diag([24.0, 5.0, 19.0]), [1, 1, 1]),  # 5.0 < 2 x 3.4: the list is built on a replica
}
MATRIX = np.array([[2.2, 2.8, 3.1], [2.8, 2.5, 2.9], [3.1, 2.9, 3.4]])


def _random_system(name, perm=None):
    h, boundary = BOXES[name]
    rng = np.random.default_rng(17)
    pos = rng.random((300, 3)) @ h
    types = rng.integers(1, 4, 300).astype(np.int32) * 2  # 2, 4, 6: compact types are not the types themselves
    if perm is not None:
        pos, types = pos[perm], types[perm]
    return mp.System(data={"x": pos[:, 0], "y": pos[:, 1], "z": pos[:, 2], "type": types}, box=mp.Box(h, boundary))


@pytest.mark.parametrize("name", sorted(BOXES))
def test_random_atoms(name):
    system = _random_system(name)
    bond = system.create_bonds(MATRIX)
    replica = "_enlarge_data" in system.__dict__
    assert replica == (name == "thin")
    frame = system._get_compute_view()[1]
    _, compact, matrix = _normalize_bond_cutoff(MATRIX, frame)
    lists = (system.verlet_list, system.distance_list, system.neighbor_number)
    assert ref.margin(*lists, compact, matrix) > 1e-9  # (checked on the CPU: no pair sits on its cutoff)
    want = ref.build_bond(*lists, compact, matrix, 1, system.N if replica else 0)
    assert len(want) > 200 and np.array_equal(as_numpy(bond), want) and as_numpy(bond).max() < system.N
    # the dict spells the same cutoffs; the same call twice gives the same bits
    pairs = {(2 * a + 2, 2 * b + 2): MATRIX[a, b] for a in range(3) for b in range(a, 3)}
    again = system.create_bonds(pairs)
    assert again is not bond and np.array_equal(as_numpy(again), want)
    assert as_numpy(system.create_bonds(MATRIX)).tobytes() == as_numpy(bond).tobytes()
    # the same frame shuffled: the same bonds through the permutation
    perm = np.random.default_rng(5).permutation(300)
    moved = perm[as_numpy(_random_system(name, perm).create_bonds(MATRIX)).astype(np.int64)]
    moved.sort(axis=1)
    assert np.array_equal(np.unique(moved, axis=0).astype(np.int32), want) and len(moved) == len(want)
    # one cutoff for all
    flat = system.create_bonds(2.6)
    assert np.array_equal(as_numpy(flat), ref.build_bond(*lists, None, np.array([[2.6]]), 1, system.N if replica else 0))


# ---- the water frame: 24 576 atoms, 8 192 molecules
def test_water_frame(tmp_path):
    path = tmp_path / "water.xyz"
    with gzip.open(os.path.join(GOLDEN, "water.xyz.gz"), "rb") as src:
        path.write_bytes(src.read())
    system = mp.System(str(path))
    assert system.N == 24576
    assert system.cal_chemical_species(["H2O"], scale=0.4, add_mol_id=True) == {"H2O": 8192}
    mol = system.data["mol_id"].to_numpy()
    assert mol.dtype == np.int32 and mol.shape == (24576,) and not mol.any()
    cut = {("H", "H"): 2.4 * 0.4, ("H", "O"): 2.7 * 0.4, ("O", "O"): 3.0 * 0.4}
    bond = as_numpy(system.create_bonds(cut))
    assert bond.shape == (16384, 2)
    oxygen = system.data["element"].to_numpy() == "O"
    ends = np.bincount(bond.ravel(), minlength=system.N)
    assert np.all(ends[oxygen] == 2) and np.all(ends[~oxygen] == 1)
    _, compact, matrix = _normalize_bond_cutoff(cut, system.data)
    lists = (system.verlet_list, system.distance_list, system.neighbor_number)
    assert 2.0e-3 < ref.margin(*lists, compact, matrix) < 2.1e-3
    assert np.array_equal(bond, ref.build_bond(*lists, compact, matrix))

    system = mp.System(str(path))
    wide = np.array([[2.4, 2.7], [2.7, 3.0]]) * 0.6
    system.build_neighbor(float(wide.max()))
    lists = (system.verlet_list, system.distance_list, system.neighbor_number)
    assert ref.margin(*lists, compact, wide) > 1e-9  # (no pair within 1e-9 of its cutoff at scale 0.6)
    assert system.cal_chemical_species(scale=0.6, check_most=3) == {"HHO": 7760, "HHHHOO": 199, "HHHHHHOOO": 10}
    assert system.cluster_number == 7970
    names = system.data["element"].to_numpy()
    grouped = ref.species_grouping(system.data["cluster_id"].to_numpy(), names)
    assert sorted(grouped.values(), reverse=True) == [7760, 199, 10, 1]
    assert system.cal_chemical_species(scale=0.6) == ref.most_frequent(grouped, 10)
    assert system.cal_chemical_species(["H2O", "H4O2", "OH2"], scale=0.6, add_mol_id=True) == {"H2O": 7760, "H4O2": 199, "OH2": 7760}
    mol = system.data["mol_id"].to_numpy()
    assert np.bincount(mol + 1).tolist() == [24576 - 3 * 7760 - 6 * 199, 0, 6 * 199, 3 * 7760]  # (H2O and OH2: the last index)
    wide_bond = as_numpy(system.create_bonds(wide))
    assert len(wide_bond) == 16844 and np.array_equal(wide_bond, ref.build_bond(*lists, compact, wide))


# ---- compositions and species, directly
def _compose(ids, types, n_cluster, ntype):
    want = ref.cluster_composition(ids, types, n_cluster, ntype)
    got = kernels.build_bond.cluster_composition(HArray.from_numpy(ids), HArray.from_numpy(types), n_cluster, ntype)
    assert isinstance(got, HArray) and got.shape == want.shape and np.array_equal(as_numpy(got), want)
    assert np.array_equal(kernels.build_bond.cluster_composition(ids, types, n_cluster, ntype), want)  # host arrays, staged
    return got, want


def test_composition_and_species():
    rng = np.random.default_rng(4)
    N = 3000
    types = rng.integers(0, 3, N).astype(np.int32)
    _, one = _compose(np.ones(N, np.int32), types, 1, 3)  # one cluster
    assert one.tolist() == [np.bincount(types, minlength=3).tolist()]
    own, want = _compose(np.arange(1, N + 1, dtype=np.int32)[::-1].copy(), types, N, 3)  # every atom its own cluster
    assert np.all(want.sum(axis=1) == 1)
    ids = rng.integers(1, 41, N).astype(np.int32)
    some, want = _compose(ids, types, 45, 3)  # clusters 41 .. 45 have no atom
    assert not want[40:].any()
    # two species with the same composition: both counts, the last index; a species nobody has; -1 rows
    spec = np.array([want[3], want[7], want[3], [0, 0, 0], [-1, -1, -1]], np.int32)
    for table, cluster in ((some, HArray.from_numpy(ids)), (want, ids)):
        counts, mol = kernels.build_bond.species_match(table, spec, cluster)
        rcounts, rmol = ref.species_match(want, spec, ids)
        assert counts.dtype == np.int64 and np.array_equal(counts, rcounts) and counts[0] == counts[2] >= 1 and counts[3] == 5 and counts[4] == 0
        assert as_numpy(mol).dtype == np.int32 and np.array_equal(as_numpy(mol), rmol)
        assert set(as_numpy(mol)[ids == 4].tolist()) == {2} and 0 not in set(as_numpy(mol).tolist())
        assert kernels.build_bond.species_match(table, spec)[1] is None
        assert np.array_equal(kernels.build_bond.species_match(table, spec)[0], rcounts)
    counts, mol = kernels.build_bond.species_match(own, np.eye(3, dtype=np.int32), HArray.from_numpy(np.arange(1, N + 1, dtype=np.int32)[::-1].copy()))
    assert counts.tolist() == np.bincount(types, minlength=3).tolist() and np.array_equal(as_numpy(mol), types)


@pytest.mark.parametrize("what", ["id_zero", "id_beyond", "type_negative", "type_beyond"])
def test_composition_refuses_what_is_out_of_range(what):
    ids, types = np.ones(500, np.int32), np.zeros(500, np.int32)
    {"id_zero": ids, "id_beyond": ids, "type_negative": types, "type_beyond": types}[what][321] = \
        {"id_zero": 0, "id_beyond": 2, "type_negative": -1, "type_beyond": 2}[what]
    with pytest.raises(ValueError, match="outside"):
        kernels.build_bond.cluster_composition(HArray.from_numpy(ids), HArray.from_numpy(types), 1, 2)
