"""numpy restatements of the bond pairs and the chemical species (TEST INFRASTRUCTURE): what tests/test_bonds_host.py installs as
``kernels.build_bond`` and what tests/test_gpu_bonds.py compares the kernels with.

``build_bond`` is the reference's rule taken literally — src/build_bond.cpp:37-62 over ALL rows with j > i, then the steps of
``System.create_bonds`` (src/mdapy/system.py:1402-1411): ``% N`` on a replica list, ``sort(axis=1)``, drop i == j, ``np.unique``.
It knows nothing of the shortcut the kernel takes on a replica list (the rows of the real atoms only)."""
import numpy as np

from mdapy_amd.devarray import as_numpy


def build_bond(verlet_list, distance_list, neighbor_number, type_list, cutoff_matrix, num_t=1, n_real=0):
    rows, dist, nn = as_numpy(verlet_list), as_numpy(distance_list), as_numpy(neighbor_number)
    N, M = rows.shape
    cut = np.asarray(cutoff_matrix, np.float64)
    ntype = cut.shape[1]
    types = np.zeros(N, np.int64) if type_list is None else as_numpy(type_list).astype(np.int64)
    own = np.arange(N, dtype=np.int64)[:, None]
    j = rows.astype(np.int64)
    # (an entry outside 0 .. N - 1 — the reference would read types[j] out of bounds — is no bond)
    listed = (np.arange(M)[None, :] < np.clip(nn, 0, M)[:, None]) & (j > own) & (j < N)
    tj = types[np.where(listed, j, 0)]
    ti = np.broadcast_to(types[:, None], (N, M))
    listed &= (ti >= 0) & (ti < ntype) & (tj >= 0) & (tj < ntype)
    limit = cut[np.where(listed, ti, 0), np.where(listed, tj, 0)]
    listed &= dist <= limit
    i_idx, slot = np.nonzero(listed)
    bond = np.stack([i_idx, j[i_idx, slot]], axis=1).astype(np.int32).reshape(-1, 2)
    if bond.size == 0:
        return np.empty((0, 2), np.int32)
    if n_real:
        bond %= np.int32(n_real)
    bond.sort(axis=1)
    bond = bond[bond[:, 0] != bond[:, 1]]
    if bond.size == 0:
        return np.empty((0, 2), np.int32)
    return np.unique(bond, axis=0)


def margin(verlet_list, distance_list, neighbor_number, type_list, cutoff_matrix):
    """the smallest |dist - cutoff| over the listed slots whose types lie inside the matrix: how far the nearest pair is from
    changing sides"""
    rows, dist, nn = as_numpy(verlet_list), as_numpy(distance_list), as_numpy(neighbor_number)
    N, M = rows.shape
    cut = np.asarray(cutoff_matrix, np.float64)
    types = np.zeros(N, np.int64) if type_list is None else as_numpy(type_list).astype(np.int64)
    listed = (np.arange(M)[None, :] < np.clip(nn, 0, M)[:, None]) & (rows >= 0) & (rows < N)
    tj = types[np.where(listed, rows, 0)]
    ti = np.broadcast_to(types[:, None], (N, M))
    listed &= (ti >= 0) & (ti < len(cut)) & (tj >= 0) & (tj < len(cut))
    if not listed.any():
        return np.inf
    return float(np.abs(dist - cut[np.where(listed, ti, 0), np.where(listed, tj, 0)])[listed].min())


def cluster_composition(cluster_id, type_list, cluster_number, ntype):
    """comp[c - 1][t] = atoms of compact type t in cluster c; an id or a type outside its range is an error"""
    ids, types = as_numpy(cluster_id).astype(np.int64), as_numpy(type_list).astype(np.int64)
    if len(ids) and (ids.min() < 1 or ids.max() > cluster_number or types.min() < 0 or types.max() >= ntype):
        raise ValueError("cluster_composition: a cluster id or a type outside its range")
    comp = np.zeros((int(cluster_number), int(ntype)), np.int32)
    np.add.at(comp, (ids - 1, types), 1)
    return comp


def species_match(composition, want, cluster_id=None):
    """counts[s] = rows equal to want[s]; mol_id = the LAST species an atom's cluster equals, -1 for none"""
    comp, want = as_numpy(composition), np.asarray(want, np.int32).reshape(-1, as_numpy(composition).shape[1])
    same = (comp[None, :, :] == want[:, None, :]).all(axis=2)  # (species, cluster)
    counts = same.sum(axis=1).astype(np.int64)
    if cluster_id is None:
        return counts, None
    label = np.full(comp.shape[0], -1, np.int32)
    for s in range(want.shape[0]):
        label[same[s]] = s
    ids = as_numpy(cluster_id).astype(np.int64)
    inside = (ids >= 1) & (ids <= comp.shape[0])
    return counts, np.append(label, np.int32(-1))[np.where(inside, ids - 1, comp.shape[0])]


def species_grouping(cluster_id, names):
    """the reference's grouping (system.py:2723-2739) atom by atom: {sorted element names of a cluster, joined: clusters}"""
    members = {}
    for c, name in zip(as_numpy(cluster_id).tolist(), list(names)):
        members.setdefault(c, []).append(str(name))
    found = {}
    for parts in members.values():
        key = "".join(sorted(parts))
        found[key] = found.get(key, 0) + 1
    return found


def most_frequent(found, check_most):
    """the check_most largest of {key: count}; equal counts by ascending key"""
    return dict(sorted(found.items(), key=lambda kv: (-kv[1], kv[0]))[:check_most])
