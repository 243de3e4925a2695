#!/usr/bin/env python
"""Randomised parity sweep on the GPU box: the parity checks of tests/test_gpu_parity.py (HIP path vs the CPU
oracle / the oracle/_ref libraries) on freshly drawn systems instead of the fixed cases.

    python tests/fuzz_parity.py [seconds] [first_seed]

Every seed draws one system — orthogonal or triclinic box, random boundary flags, origin, density, lattice or
gas, optionally out-of-box ("unwrapped") atoms — and runs the checks that support that kind of input.  A failure
prints the seed and the check; the exit code is the number of failures.  Test infrastructure, like tests/.

The entries ``bond``, ``adf``, ``chill``, ``strain`` and ``ws`` (``consumer_checks``) compare the shims of the analyses the oracle
does not have with their numpy restatements, on lists the oracle built and the sweep then altered: padded, truncated, k-nearest,
counts lowered, entries beyond the cutoff; ``ws`` also asks for sites at exactly equal distances (``ws_ties``).  They also run on the water-like systems of ``draw_water`` (every third seed), where
CHILL+ finds something to classify.  FUZZ_ONLY=<prefix> runs the entries whose name starts with it.
"""
import os
import sys
import time
import traceback

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np

import test_gpu_parity as T
from mdapy_amd.build_lattice import lattice_positions


def draw(seed):
    rng = np.random.default_rng(seed)
    sigma = -1.0
    kind = rng.choice(["gas", "fcc", "bcc", "hcp", "blob", "tiny", "big"])
    tri = rng.random() < 0.4
    bnd = np.array(rng.random(3) < 0.75, np.int32)
    origin = rng.normal(0, 5.0, 3) if rng.random() < 0.5 else np.zeros(3)
    if kind == "big":  # 10-16 cells per axis: large enough for the tile kernels (orthogonal and sheared, periodic and open)
        n = [int(rng.integers(10, 17)) for _ in range(3)]
        pos, box = lattice_positions("fcc", 3.615, *n)
        box = np.asarray(box, float)
        sigma = float(rng.choice([0.03, 0.15, 0.4]))
        pos = pos + rng.normal(0, sigma, pos.shape)
        if rng.random() < 0.6:
            bnd = np.array([1, 1, 1], np.int32)
        if tri:
            sh = np.eye(3)
            sh[1, 0], sh[2, 0], sh[2, 1] = rng.uniform(-0.15, 0.15, 3)
            pos, box = pos @ sh, box @ sh
    elif kind in ("fcc", "bcc", "hcp"):
        a = {"fcc": 3.615, "bcc": 2.87, "hcp": 2.95}[kind]
        n = [int(rng.integers(4, 9)) for _ in range(3)]
        pos, box = lattice_positions(kind, a, *n)
        box = np.asarray(box, float)
        sigma = float(rng.choice([0.0, 0.03, 0.15]))
        pos = pos + rng.normal(0, sigma, pos.shape)
        if tri:  # shear the whole crystal (still a periodic crystal of the sheared box)
            sh = np.eye(3)
            sh[1, 0], sh[2, 0], sh[2, 1] = rng.uniform(-0.3, 0.3, 3)
            pos, box = pos @ sh, box @ sh
    elif kind == "tiny":  # a few atoms in a box of a few cutoffs: replication policies, rows with periodic twins
        L = rng.uniform(5.0, 11.0, 3)
        box = np.diag(L)
        if tri:
            box[1, 0], box[2, 0], box[2, 1] = rng.uniform(-0.3, 0.3, 3) * L[0]
        pos = rng.random((int(rng.integers(3, 60)), 3)) @ box
    else:
        L = rng.uniform(12.0, 34.0, 3)
        box = np.diag(L)
        if tri:
            box[1, 0], box[2, 0], box[2, 1] = rng.uniform(-0.35, 0.35, 3) * L[0]
        rho = rng.uniform(0.01, 0.07)
        N = int(min(max(rho * abs(np.linalg.det(box)), 150), 5000))
        frac = rng.random((N, 3))
        if kind == "blob":
            frac[: N // 2] = 0.3 + 0.25 * frac[: N // 2]
        pos = frac @ box
    pos = pos + origin
    if tri and rng.random() < 0.4:  # general orientation: upper-triangular entries, cell vectors off the axes
        q, _ = np.linalg.qr(rng.normal(size=(3, 3)))
        q *= np.sign(np.linalg.det(q))
        pos, box, origin = pos @ q, box @ q, origin @ q
    unwrapped = rng.random() < 0.2
    if unwrapped:
        far = int(rng.choice([2, 2, 13, 20]))  # (up to 14 box lengths the tile kernel keeps the call, beyond the thread-per-atom one takes it)
        pos = pos + (rng.integers(-far, far + 1, pos.shape) * bnd) @ box
    return dict(seed=seed, sigma=sigma, kind=kind, tri=tri, unwrapped=unwrapped, pos=pos, box=box, origin=origin, bnd=bnd)


def rdf_stream_check(s):
    """streaming partial RDF (tile kernel for orthogonal boxes, thread-per-atom otherwise) against the oracle: integer counts"""
    r = np.random.default_rng(s["seed"] + 23)
    pos = s["pos"]
    nt = int(r.integers(1, 4))
    ty = r.integers(0, nt, len(pos)).astype(np.int32)
    thick = np.abs(np.linalg.det(s["box"])) / np.array([np.linalg.norm(np.cross(s["box"][(d + 1) % 3], s["box"][(d + 2) % 3])) for d in range(3)])
    rc = float(r.uniform(2.5, max(3.0, min(9.0, thick.min() * 0.45))))
    nbin = int(r.integers(10, 400))
    x, y, z = T._xyz(pos)
    g0, g1 = np.zeros((nt, nt, nbin)), np.zeros((nt, nt, nbin))
    T.O._rdf_streaming(x, y, z, ty, s["box"], s["origin"], s["bnd"], g0, rc, nbin, 8)
    T._rdf._rdf_streaming(x, y, z, ty, s["box"], s["origin"], s["bnd"], g1, rc, nbin, 1)
    assert np.array_equal(g0, g1)


def fused_check(s):
    """mdh_build_neighbor_fcna against mdh_build_neighbor followed by mdh_fcna: lists and labels bit for bit"""
    r = np.random.default_rng(s["seed"] + 31)
    x, y, z = T._xyz(s["pos"])
    n = len(x)
    rc = float(r.uniform(2.7, 3.9))
    M = int(r.choice([12, 14, 16, 20, 30]))
    va = np.full((n, M), -1, np.int32); da = np.full((n, M), rc + 1.0); na = np.zeros(n, np.int32); pa = np.zeros(n, np.int32)
    T._neighbor.build_neighbor(x, y, z, s["box"], s["origin"], s["bnd"], rc, va, da, na, 1)
    T._cna.fcna(x, y, z, s["box"], s["origin"], s["bnd"], va, na, pa, rc, 1)
    vb = np.empty((n, M), np.int32); db = np.empty((n, M)); nb = np.empty(n, np.int32); pb = np.zeros(n, np.int32)
    T._neighbor.build_neighbor_fcna(x, y, z, s["box"], s["origin"], s["bnd"], rc, vb, db, nb, pb, 1, fill_pads=True)
    assert np.array_equal(nb, na) and np.array_equal(vb, va) and np.array_equal(db, da) and np.array_equal(pb, pa)


def wide_rows_check(s):
    """rows of 65 ... 128 slots (rc 5.4 ... 6.1 A on the big crystals): exact-width and fixed-width rows bit for bit vs the oracle"""
    r = np.random.default_rng(s["seed"] + 41)
    x, y, z = T._xyz(s["pos"])
    n = len(x)
    rc = float(r.uniform(5.4, 6.1))
    v2, d2, n2 = T._neighbor.build_neighbor_without_max_neigh(x, y, z, s["box"], s["origin"], s["bnd"], rc, 1)
    vo, do, no = T.O.build_neighbor_without_max_neigh(x, y, z, s["box"], s["origin"], s["bnd"], rc, 8)
    assert np.array_equal(n2, no) and np.array_equal(v2, vo) and np.array_equal(d2, do)
    M = int(r.choice([66, 80, 97, 128]))
    va = np.full((n, M), -1, np.int32); da = np.full((n, M), rc + 1.0); na = np.zeros(n, np.int32)
    T.O.build_neighbor(x, y, z, s["box"], s["origin"], s["bnd"], rc, va, da, na, 8)
    vb = np.empty((n, M), np.int32); db = np.empty((n, M)); nb = np.empty(n, np.int32)
    T._neighbor.build_neighbor(x, y, z, s["box"], s["origin"], s["bnd"], rc, vb, db, nb, 1, fill_pads=True)
    assert np.array_equal(nb, na) and np.array_equal(vb, va) and np.array_equal(db, da)


def draw_water(seed):
    """a water-like system (molecule centres only), in ``draw``'s format: cubic ice (diamond, a = 6.37), hexagonal ice (lonsdaleite,
    a = 4.5) or ``mixed`` — cubic ice whose upper half in z is replaced by uniformly random points — so that CHILL+ has
    four-coordinated sites to classify, which the metals and gases of ``draw`` do not offer"""
    rng = np.random.default_rng(seed)
    kind = str(rng.choice(["diamond", "lonsdaleite", "mixed"]))
    structure, a = ("lonsdaleite", 4.5) if kind == "lonsdaleite" else ("diamond", 6.37)
    n = [int(rng.integers(3, 8)) for _ in range(3)]
    if rng.random() < 0.15:  # one cell across some axes: thinner than two cutoffs, System analyses a replica
        single = rng.random(3) < 0.5
        single[int(rng.integers(0, 3))] = True
        n = [1 if one else min(v, 4) for one, v in zip(single, n)]
    pos, box = lattice_positions(structure, a, *n)
    box = np.asarray(box, float)
    if kind == "mixed":
        up = pos[:, 2] > 0.5 * box[2, 2]
        pos[up] = rng.random((int(up.sum()), 3)) * np.array([box[0, 0], box[1, 1], 0.5 * box[2, 2]]) + np.array([0.0, 0.0, 0.5 * box[2, 2]])
    sigma = float(rng.choice([0.0, 0.1, 0.2, 0.3]))
    if sigma:
        pos = pos + rng.normal(0, sigma, pos.shape)
    tri = rng.random() < 0.4
    if tri:
        sh = np.eye(3)
        sh[1, 0], sh[2, 0], sh[2, 1] = rng.uniform(-0.3, 0.3, 3)
        pos, box = pos @ sh, box @ sh
    bnd = np.array(rng.random(3) < 0.75, np.int32)
    origin = rng.normal(0, 5.0, 3) if rng.random() < 0.5 else np.zeros(3)
    pos = pos + origin
    if tri and rng.random() < 0.4:  # general orientation, as in draw
        q, _ = np.linalg.qr(rng.normal(size=(3, 3)))
        q *= np.sign(np.linalg.det(q))
        pos, box, origin = pos @ q, box @ q, origin @ q
    return dict(seed=seed, sigma=sigma, kind=kind, tri=tri, unwrapped=False, pos=pos, box=box, origin=origin, bnd=bnd, water=True)


# ----------------------------------------------------------------------------------------------------------------------
# The consumers of a neighbour list that the oracle does not have — bond / angular distribution, CHILL+, atomic strain — and the
# Wigner-Seitz search, at the C ABI against the numpy restatements of tests/_bond_ref.py, _chill_ref.py, _strain_ref.py and
# _ws_ref.py, on lists that System's policy layer would never pass but a caller of the shims may.
# ----------------------------------------------------------------------------------------------------------------------
STATS = None  # a dict, while somebody wants to know what the yardsticks saw (tests/test_gpu_fuzz_consumers.py)
PAD_WIDTHS = (15, 16, 17, 32, 33, 64)  # around ROW_CHUNK = 16 (csrc/common.hpp) and its multiples
NBINS = (1, 2, 180, 2050)  # and odd values; 2050 is one above BA_EDGES_LDS + 1 (csrc/bond.hip): its step points do not fit in LDS


def _note(key, value=1):
    if STATS is not None:
        STATS[key] = STATS.get(key, 0) + value


def _thickness(box):
    return np.abs(np.linalg.det(box)) / np.array([np.linalg.norm(np.cross(box[(d + 1) % 3], box[(d + 2) % 3])) for d in range(3)])


def draw_nbin(r):
    return int(r.choice(list(NBINS) + [2 * int(r.integers(1, 60)) + 1] * 2))


def draw_patterns(r, codes, reach, many=False, at_least=1):
    """ADF patterns over the type codes ``codes``: [(centre, j, k)], [[rij_min, rij_max, rik_min, rik_max]], and what each one is —
    ``same`` (j and k of one type), ``mixed``, and ``lower`` beside either where a lower bound is not zero.  Every triple at most
    once (System's patterns are the keys of a dict); ``many``: more of them than BA_PAT = 32 (csrc/bond.hip), one launch's worth"""
    triples = [(a, b, c) for a in codes for b in codes for c in codes]
    count = min(len(triples), int(r.integers(33, 41)) if many else int(r.integers(at_least, 7)))
    picked = [triples[k] for k in r.permutation(len(triples))[:count]]
    ranges, kinds = [], []
    for a, b, c in picked:
        hi = reach * r.uniform(0.6, 1.0, 2)
        lo = np.where(r.random(2) < 0.3, hi * r.uniform(0.2, 0.7, 2), 0.0)
        ranges.append([lo[0], hi[0], lo[1], hi[1]])
        kinds.append(("same" if b == c else "mixed") + (" lower" if lo.any() else ""))
    return picked, ranges, kinds


def note_adf(hist, kinds, nbin):
    """which kinds of pattern set have counted something (on the yardstick's histogram)"""
    hist = np.asarray(hist).reshape(len(kinds), -1)
    for row, kind in zip(hist, kinds):
        if row.sum() > 0:
            for word in kind.split():
                _note("adf nonempty " + word)
    if hist.sum() > 0 and len(kinds) > 32:
        _note("adf nonempty many")
    # the library launches the patterns BA_PAT = 32 at a time, each launch with a histogram of its own patterns x nbin: beyond
    # BA_HIST_LDS = 8192 bins that one goes straight to HBM (csrc/bond.hip)
    for first in range(0, len(kinds), 32):
        group = hist[first:first + 32]
        if group.size > 8192 and group.sum() > 0:
            _note("adf nonempty wide")


def note_chill(want, ambiguous):
    _note("chill atoms", len(want))
    _note("chill ambiguous", int(ambiguous.sum()))
    for code, count in enumerate(np.bincount(want, minlength=6).tolist()):
        _note(f"chill class {code}", count)


def chill_rule(got, want, ambiguous):
    """the parity rule of tests/_chill_ref.py for one drawn system: every atom that is not ambiguous carries the yardstick's label,
    and at most max(3, MAX_AMBIGUOUS N) atoms are ambiguous (one atom of a 240-atom draw is already 0.42 %; the share over a
    whole seed range is asserted by the tests, from the figures noted here)"""
    import _chill_ref

    got, want = np.asarray(got), np.asarray(want)
    note_chill(want, ambiguous)
    assert got.dtype == np.int32 and got.shape == want.shape
    assert ambiguous.sum() <= max(3, _chill_ref.MAX_AMBIGUOUS * len(want)), f"{int(ambiguous.sum())} of {len(want)} atoms sit on a threshold"
    bad = np.flatnonzero((got != want) & ~ambiguous)
    assert bad.size == 0, f"{bad.size} unambiguous atoms differ, e.g. atom {bad[:5].tolist()}: got {got[bad[:5]].tolist()}, want {want[bad[:5]].tolist()}"


def deformation(r):
    """a deformation gradient: shear plus stretch of a few per cent"""
    return np.eye(3) + r.uniform(-0.04, 0.04, (3, 3))


def consumer_case(s, salt, whole=False):
    """positions (a random subset of the system's atoms — one atom, 33, a few hundred — unless ``whole``), the box made two
    cutoffs thick by doubling it along thin periodic axes, and a list of those atoms: built by the oracle and then altered"""
    r = np.random.default_rng(s["seed"] + salt)
    rc = float(r.uniform(3.2, 3.8) if s.get("water") else r.uniform(2.6, 4.2))
    n = len(s["pos"])
    m = n if whole else min(n, int(r.choice([1, 33, 64, 97, 130, int(r.integers(100, 600)), int(r.integers(100, 600))])))
    pos, box, bnd = s["pos"][np.sort(r.choice(n, m, replace=False))], np.array(s["box"], float), s["bnd"]
    for d in range(3):
        while bnd[d] and _thickness(box)[d] < 2.0 * rc + 0.1:
            pos, box[d] = np.vstack([pos, pos + box[d]]), 2.0 * box[d]
    x, y, z = T._xyz(pos)
    where = (box, s["origin"], bnd)
    v, d, nn = T.O.build_neighbor_without_max_neigh(x, y, z, *where, rc, 8)
    N, M = v.shape
    how = str(r.choice(["exact", "padded", "padded", "nearest", "lowered", "beyond"]))
    k = int(r.choice([4, 12, 16, 17]))
    if how == "nearest" and (s["unwrapped"] or N < k + 20):  # (the reference's search wants wrapped atoms and more atoms than k)
        how = "exact"
    if how == "padded":  # pads behind the rows — or, narrower than the rows, a fixed-width list that truncated them
        width = int(r.choice(PAD_WIDTHS))
        if width < M:
            how = "truncated"
            v, d, nn = np.ascontiguousarray(v[:, :width]), np.ascontiguousarray(d[:, :width]), np.minimum(nn, width).astype(np.int32)
        else:
            v = np.hstack([v, np.full((N, width - M), -1, np.int32)])
            d = np.hstack([d, np.full((N, width - M), rc + 1.0)])
    elif how == "nearest":  # asymmetric rows, distances beyond rc, every count k
        v, d, nn = np.empty((N, k), np.int32), np.empty((N, k)), np.full(N, k, np.int32)
        T.O.knn(x, y, z, *where, k, v, d, 8)
    elif how == "lowered":  # counts below the rows' content
        nn = r.integers(0, nn + 1).astype(np.int32)
    elif how == "beyond":  # entries beyond rc scattered inside the rows
        far = (np.arange(M)[None, :] < nn[:, None]) & (r.random(v.shape) < 0.2)
        d = np.where(far, rc + r.uniform(0.05, 2.0, v.shape), d)
    _note("list " + how)
    return r, rc, pos, (x, y, z), where, (np.ascontiguousarray(v), np.ascontiguousarray(d), np.ascontiguousarray(nn))


def bond_check(s):
    import _bond_ref
    from mdapy_amd import _bond_analysis

    r, rc, pos, cols, where, lists = consumer_case(s, 51)
    nbin = draw_nbin(r)
    got, want = [np.zeros(nbin, np.int64) for _ in range(2)], [np.zeros(nbin, np.int64) for _ in range(2)]
    _bond_ref.compute_bond(*cols, *where, *lists, *want, rc / nbin, 180.0 / nbin, rc, nbin)
    _bond_analysis.compute_bond(*cols, *where, *lists, *got, rc / nbin, 180.0 / nbin, rc, nbin)
    _note("bond lengths", int(want[0].sum()))
    _note("bond angles", int(want[1].sum()))
    assert np.array_equal(got[0], want[0]), "bond lengths"
    assert np.array_equal(got[1], want[1]), "bond angles"


def adf_check(s):
    import _bond_ref
    from mdapy_amd import _bond_analysis

    r, rc, pos, cols, where, lists = consumer_case(s, 53)
    many = r.random() < 0.2
    ntypes = 4 if many else int(r.integers(1, 4))
    types = r.integers(0, ntypes, len(pos)).astype(np.int32)
    codes = list(range(ntypes)) + ([ntypes] if r.random() < 0.2 else [])  # (a code no atom carries: an empty row)
    triples, ranges, kinds = draw_patterns(r, codes, rc, many)
    nbin = int(r.choice([263, 300])) if many and r.random() < 0.5 else draw_nbin(r)  # (32 x 257 is the first launch beyond 8192 bins)
    got, want = (np.zeros((len(triples), nbin), np.int64) for _ in range(2))
    _bond_ref.compute_adf(*cols, *where, *lists, 180.0 / nbin, ranges, triples, types, nbin, want)
    note_adf(want, kinds, nbin)
    _bond_analysis.compute_adf(*cols, *where, *lists, 180.0 / nbin, ranges, triples, types, nbin, got)
    assert np.array_equal(got, want)


def chill_check(s):
    import _chill_ref
    from mdapy_amd import _chill_plus

    r, rc, pos, cols, where, lists = consumer_case(s, 57, whole=bool(s.get("water")))  # (a subset of an ice has no four-coordinated site)
    got = np.full(len(pos), 7, np.int32)
    _chill_plus.compute_chill_plus(*cols, *where, *lists, rc, got)
    want, _, ambiguous = _chill_ref.analyse(*cols, *where, *lists, rc)
    chill_rule(got, want, ambiguous)


def strain_check(s):
    import _strain_ref
    from mdapy_amd import _strain

    r, rc, pos, cols, where, lists = consumer_case(s, 59)
    box, origin, bnd = where
    grad = deformation(r)
    cur = _xyz_of((pos - origin) @ grad + origin @ grad + r.normal(0, 0.03, pos.shape))
    rows, counts = lists[0], lists[2]
    n = len(pos)
    boxes = (box, box @ grad, origin, origin @ grad, bnd)
    got, want = (np.full(n, 7.0), np.full(n, 7.0)), (np.empty(n), np.empty(n))
    _strain_ref.cal_atomic_strain(rows, counts, *boxes, *cols, *cur, *want)
    _strain.cal_atomic_strain(rows, counts, *boxes, *cols, *cur, *got)
    _note("strain finite", int(np.isfinite(want[0]).sum()))
    assert np.array_equal(got[0], want[0], equal_nan=True), "shear"
    assert np.array_equal(got[1], want[1], equal_nan=True), "volumetric"
    # records made once, the affine map in the packing kernel
    mapped = _strain_ref.affine_mapped(box @ grad, box, *cur)
    boxes = (box, box, origin, origin, bnd)
    _strain_ref.cal_atomic_strain(rows, counts, *boxes, *cols, *mapped, *want)
    ref_records = _strain.pack_records(*cols)
    cur_records = _strain.pack_records(*cur, np.linalg.solve(box @ grad, box))
    _strain.cal_atomic_strain_records(rows, counts, *boxes, ref_records, cur_records, *got)
    assert np.array_equal(got[0], want[0], equal_nan=True), "shear, records"
    assert np.array_equal(got[1], want[1], equal_nan=True), "volumetric, records"


def _xyz_of(pos):
    return tuple(np.ascontiguousarray(pos[:, k]) for k in range(3))


def ws_check(s):
    import _ws_ref
    from mdapy_amd import _fast_knn

    r = np.random.default_rng(s["seed"] + 61)
    n = len(s["pos"])
    # 1, 4, 50 and 201 sites: where the reference's image count 200 // clamp(N, 50, 200) changes
    ns = min(n, int(r.choice([1, 4, 50, 201, int(r.integers(2, 700))])))
    sites = s["pos"][np.sort(r.choice(n, ns, replace=False))]
    box, origin, bnd = np.array(s["box"], float), s["origin"], s["bnd"]
    kept = sites[r.random(ns) < 0.9]
    atoms = np.vstack([kept + r.normal(0, 0.3, kept.shape), r.random((int(r.integers(1, 8)), 3)) @ box + origin])
    atoms = atoms + (r.integers(-2, 3, atoms.shape) * (r.random((len(atoms), 1)) < 0.2)) @ box  # some of them images away
    affine_map = np.linalg.solve(box @ deformation(r), box) if r.random() < 0.5 else None
    want, got = np.zeros(len(atoms), np.int32), np.full(len(atoms), 7, np.int32)
    for tree, out in ((_ws_ref.Tree(), want), (_fast_knn.Tree(), got)):
        tree.build_with_coords(*_xyz_of(sites), box, origin, bnd)
        tree.query_nearest_batch(*_xyz_of(atoms), out, affine_map=affine_map)
    assert np.array_equal(got, want), f"{int((got != want).sum())} of {len(atoms)} atoms on another site"
    types = r.integers(1, 4, ns).astype(np.int32)
    w = np.zeros(ns, np.int32), np.zeros(len(atoms), np.int32), np.zeros(len(atoms), np.int32)
    g = np.zeros(ns, np.int32), np.zeros(len(atoms), np.int32), np.zeros(len(atoms), np.int32)
    counts = _ws_ref.cal_site_occupancy(want, types, *w)
    _note("ws vacancies", counts[0])
    _note("ws interstitials", counts[1])
    assert _fast_knn.cal_site_occupancy(got, types, *g) == counts
    assert all(np.array_equal(a, b) for a, b in zip(g, w))
    ws_ties(s)


def ws_ties(s):
    """queries at EXACTLY equal distance from two, four or eight sites, which random positions never are: a simple cubic grid of
    spacing 2 in a box of 4, 8 or 16 (integers and powers of two: every product and difference of the search is exact), the site
    ids shuffled so that the lowest id is anywhere in the order the cells are visited in; queries on bond midpoints, face centres
    and cell centres, some of them whole boxes away.  The lowest tied id must win — worked out here from the integer distances,
    for the restatement as well as for the library"""
    import _ws_ref
    from mdapy_amd import _fast_knn

    r = np.random.default_rng(s["seed"] + 67)
    n = int(r.choice([2, 4, 8]))
    L = 2.0 * n
    origin = r.integers(-3, 4, 3).astype(float)
    bnd = np.array(s["bnd"], np.int32)
    grid = np.stack(np.meshgrid(*[2.0 * np.arange(n)] * 3, indexing="ij"), axis=-1).reshape(-1, 3)
    sites = grid[r.permutation(len(grid))] + origin
    nq = 40
    offsets = r.integers(0, 2, (nq, 3)).astype(float) * r.choice([-1.0, 1.0], (nq, 3))
    atoms = sites[r.integers(0, len(sites), nq)] + offsets + r.integers(-2, 3, (nq, 3)) * bnd * L
    diff = sites[None, :, :] - atoms[:, None, :]
    diff = np.where(bnd[None, None, :] != 0, (diff + L / 2) % L - L / 2, diff)
    d2 = (diff * diff).sum(axis=-1)
    tied = d2 == d2.min(axis=1, keepdims=True)
    expect = np.array([int(np.flatnonzero(row)[0]) for row in tied], np.int32)
    _note("ws ties", int((tied.sum(axis=1) > 1).sum()))
    for tree in (_ws_ref.Tree(), _fast_knn.Tree()):
        out = np.full(nq, 7, np.int32)
        tree.build_with_coords(*_xyz_of(sites), np.eye(3) * L, origin, bnd)
        tree.query_nearest_batch(*_xyz_of(atoms), out)
        assert np.array_equal(out, expect), f"{type(tree).__module__}: {int((out != expect).sum())} of {nq} tied queries not on the lowest site id"


def chill_defined(s):
    """not on the unrattled fcc, bcc and hcp crystals of ``draw``.  Bonds in opposite directions cancel in q_3m (l is odd): every
    fcc and bcc site is a centre of inversion of its shells, and the six in-plane neighbours of an hcp site are three such pairs.
    An atom of an unrattled crystal whose counted bonds come in opposite pairs — any bulk fcc or bcc site; in all three the
    few-coordinated atoms of a subset, a surface or a row with lowered counts — has for q what rounding left of zero, and the
    reference divides one such residue by another (src/chill_plus.cpp:153-158, in float32): c, and with it the label of a
    four-coordinated atom, is rounding noise.  (Seen at the C ABI on subsets of all three, hcp at seed 70030.)  The ices have no
    such sites."""
    return bool(s.get("water")) or s["sigma"] != 0.0


def consumer_checks(s):
    return [("bond", lambda: bond_check(s)), ("adf", lambda: adf_check(s))] + ([("chill", lambda: chill_check(s))] if chill_defined(s) else []) \
        + [("strain", lambda: strain_check(s)), ("ws", lambda: ws_check(s))]


def checks(s):
    if s.get("water"):  # the water draws are for the consumers alone
        return consumer_checks(s)
    return parity_checks(s) + consumer_checks(s)


def parity_checks(s):
    case = ("fuzz", s["pos"], s["box"], s["origin"], s["bnd"])
    if s["kind"] == "big":  # the tile kernels: neighbour rows bit for bit (fixed and exact width), pair counts
        rc_big = float(np.random.default_rng(s["seed"] + 7).uniform(2.8, 3.7))
        T._cases = lambda: [(n, ) + case[1:] for n in NAMES]
        return [("neighbor", lambda: T.test_neighbor_bit_exact_vs_oracle(case, rc_big)), ("rdf_stream", lambda: rdf_stream_check(s)),
                ("fused_cna", lambda: fused_check(s))] + ([("wide_rows", lambda: wide_rows_check(s))] if s["seed"] % 3 == 0 else [])
    T._cases = lambda: [(n, ) + case[1:] for n in NAMES]
    rc = float(np.random.default_rng(s["seed"] + 7).uniform(2.6, 4.6))
    out = [("neighbor", lambda: T.test_neighbor_bit_exact_vs_oracle(case, rc)),
           ("rdf_stream", lambda: rdf_stream_check(s)),
           ("fused_cna", lambda: fused_check(s)),
           ("sort_cna", lambda: T.test_sort_and_cna_vs_oracle(case)),
           ("overlap", lambda: T.test_filter_overlap_atom_vs_oracle("fuzz"))]
    if len(s["pos"]) >= 300 and s["kind"] in ("fcc", "bcc", "blob"):  # (the check also wants some atoms removed by its last cutoff set)
        out += [("overlap_grain", lambda: T.test_filter_overlap_atom_with_grain_vs_oracle("fuzz"))]
    if not s["unwrapped"] and (len(s["pos"]) >= 20 or all(s["bnd"])):  # open box with fewer atoms than neighbours asked for: the reference indexes x[-1]
        out += [("knn", lambda: T.test_knn_general_vs_oracle(case)),
                ("steinhardt_rc", lambda: T.test_steinhardt_vs_oracle(case, "rc")),
                ("steinhardt_nnn", lambda: T.test_steinhardt_vs_oracle(case, "nnn")),
                ("aja_cnp_entropy", lambda: T.test_aja_cnp_entropy_vs_oracle("fuzz")),
                ]
        if len(s["pos"]) >= 100:  # that check also asserts that its type filter removes something
            out += [("temp_cluster", lambda: T.test_atomic_temperature_and_cluster_vs_oracle("fuzz"))]
        if T.O.have_ref() and s["sigma"] != 0.0:  # perfect lattices: exact ties / degenerate hulls decide by rounding noise
            r2 = np.random.default_rng(s["seed"] + 13)
            structure = str(r2.choice(["default", "all", "fcc-hcp-bcc-ico-sc", "fcc-hcp-bcc", "dcub-dhex", "bcc,sc", "graphene-fcc", "ico"]))
            types = r2.integers(1, 4, len(s["pos"])).astype(np.int32) if r2.random() < 0.4 else None
            pc = ("fuzz", s["pos"] - s["origin"], s["box"], tuple(int(v) for v in s["bnd"]), structure, types, float(r2.choice([0.0, 0.05, 0.1, 0.3])))
            out += [("ptm", lambda: T.test_ptm_vs_reference_library(pc))]
        ortho = not np.any(s["box"] - np.diag(np.diag(s["box"])))  # the orthogonal entry points (hcp cells are hexagonal)
        if T.O.have_voro_ref() and ortho and s["kind"] != "blob" and all(s["bnd"]):
            out += [("voronoi", lambda: T.test_voronoi_vs_reference_library("fuzz")),
                    ("voronoi_nb", lambda: T.test_voronoi_neighbors_vs_reference_library("fuzz"))]
        if T.O.have_voro_ref() and ortho and s["kind"] == "gas":  # (a 400-atom corner of a crystal in its full periodic box is the
            # cluster-in-vacuum case the Voronoi driver refuses)
            out += [("cell_info", lambda: T.test_voronoi_cell_info_vs_reference_library("random_gas"))]
    return out


NAMES = ["fuzz", "random_gas"]  # "random_gas": the name under which the cell-info check takes a 400-atom subset


def main():
    budget = float(sys.argv[1]) if len(sys.argv) > 1 else 120.0
    seed = int(sys.argv[2]) if len(sys.argv) > 2 else 1000
    t0 = time.time()
    fails, ran = [], 0
    while time.time() - t0 < budget:
        s = draw(seed)
        only = os.environ.get("FUZZ_ONLY")
        # (every third seed draws a water-like system as well, for the consumer entries; the systems of ``draw`` stay what they were)
        for name, fn in checks(s) + ([(n + "@water", f) for n, f in checks(draw_water(seed))] if seed % 3 == 0 else []):
            if only and not name.startswith(only):
                continue
            if os.environ.get("FUZZ_TRACE"):
                print("seed", seed, name, flush=True)
            try:
                fn()
                ran += 1
            except AssertionError:
                tb = traceback.extract_tb(sys.exc_info()[2])[-1]
                fails.append((seed, name, f"assert at {os.path.basename(tb.filename)}:{tb.lineno}"))
            except Exception as e:  # loud refusals are findings too: list them
                fails.append((seed, name, f"{type(e).__name__}: {str(e)[:120]}"))
        seed += 1
    print(f"fuzz: {ran} checks passed over seeds up to {seed - 1}; {len(fails)} failures", flush=True)
    by = {}
    for f in fails:
        by[f[1]] = by.get(f[1], 0) + 1
    print("  by check:", by)
    for f in fails[:60]:
        s = draw_water(f[0]) if f[1].endswith("@water") else draw(f[0])
        print("  FAIL seed=%d check=%s %s  [kind=%s tri=%s unwrapped=%s bnd=%s N=%d]" % (f + (s["kind"], s["tri"], s["unwrapped"], s["bnd"].tolist(), len(s["pos"]))))
    return len(fails)


if __name__ == "__main__":
    sys.exit(min(main(), 100))
