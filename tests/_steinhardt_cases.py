"""Inputs of the Steinhardt tests (tests/test_steinhardt_host.py on the CPU, tests/test_gpu_steinhardt.py on the GPU): the
systems with their neighbour lists, the degree lists with the launch path each takes in ``mdh_get_sq``, and the run of one
(case, degree list) through a backend against the exact values of tests/_steinhardt_ref.py.

Lists are built by the CPU oracle.  Everything is built on first use and kept: the exact bond harmonics of a case are computed
once per degree, whichever test asks first."""
import functools
from types import SimpleNamespace

import numpy as np

import _steinhardt_ref as R
from mdapy_amd.build_lattice import lattice_positions
from oracle import oracle as O

PBC = np.array([1, 1, 1], np.int32)
A_FCC, RC = 3.615, 3.4


def _xyz(pos):
    return tuple(np.ascontiguousarray(pos[:, k]) for k in range(3))


def _rattled_fcc():
    pos, box = lattice_positions("fcc", A_FCC, 4, 4, 4)
    return pos + np.random.default_rng(5).normal(0.0, 0.15, pos.shape), box


def _cutoff(pos, box, org, bnd, rc=RC, **more):
    x, y, z = _xyz(pos)
    v, d, n = O.build_neighbor_without_max_neigh(x, y, z, box, org, bnd, rc, 2)
    return SimpleNamespace(x=x, y=y, z=z, box=box, org=org, bnd=bnd, v=v, d=d, n=n, nnn=0, rc=rc, use_voronoi=False, **more)


def _nearest(pos, box, org, bnd, k, rc):
    x, y, z = _xyz(pos)
    v = np.zeros((len(x), k), np.int32); d = np.zeros((len(x), k))
    O.knn(x, y, z, box, org, bnd, k, v, d, 2)
    return SimpleNamespace(x=x, y=y, z=z, box=box, org=org, bnd=bnd, v=v, d=d, n=np.full(len(x), k, np.int32), nnn=k, rc=rc, use_voronoi=False)


def _fcc256():  # full 64-row workgroups
    pos, box = _rattled_fcc()
    return _cutoff(pos, box, np.zeros(3), PBC)


def _fcc250_open_z():
    """six atoms fewer, open along z: a last workgroup of 58 rows, surface atoms with short rows, pad entries.  Handed in with
    use_voronoi set and nnn = 7: the flag keeps neighbor_number as the row length (rows would be cut at 7 entries without it)"""
    pos, box = _rattled_fcc()
    keep = np.setdiff1d(np.arange(256), np.random.default_rng(6).choice(256, 6, replace=False))
    c = _cutoff(pos[keep], box, np.zeros(3), np.array([1, 1, 0], np.int32))
    c.nnn, c.use_voronoi = 7, True
    return c


def _tri256():
    """the fractional coordinates of fcc256 in a sheared box with an origin away from zero, eight atoms handed in one box vector
    outside.  Thinnest direction 14.3: every listed bond (<= 3.4) is under a third of it"""
    pos, box = _rattled_fcc()
    frac = pos / box[0, 0]
    L = box[0, 0]
    tri = np.array([[L, 0.0, 0.0], [0.1 * L, L, 0.0], [-0.05 * L, 0.1 * L, L]])
    rng = np.random.default_rng(7)
    out = rng.choice(256, 8, replace=False)
    frac[out, rng.integers(0, 3, 8)] += rng.choice([-1.0, 1.0], 8)
    org = np.array([2.0, -7.5, 11.0])
    return _cutoff(frac @ tri + org, tri, org, PBC)


def _sc125():
    """perfect simple cubic, awkward lattice constant, shifted origin, the six nearest: every bond on the z axis (rxy = 0, |cos| = 1)
    or in the xy plane (cos = 0)"""
    pos, box = lattice_positions("sc", 2.87, 5, 5, 5)
    org = np.array([0.37, -1.91, 5.23])
    return _nearest(pos + org, box, org, PBC, 6, 1e9)


def _knn12_rc():
    """the twelve nearest of fcc256 with a cutoff that drops some of them: entries skipped inside a prefetched group of four"""
    pos, box = _rattled_fcc()
    return _nearest(pos, box, np.zeros(3), PBC, 12, 2.75)


def _single():
    z = np.zeros(1)
    return SimpleNamespace(x=z, y=z.copy(), z=z.copy(), box=np.eye(3) * 10.0, org=np.zeros(3), bnd=PBC, v=np.full((1, 1), -1, np.int32),
                           d=np.full((1, 1), RC + 1.0), n=np.zeros(1, np.int32), nnn=0, rc=RC, use_voronoi=False)


def _n65():  # one atom past a 64-row workgroup; the first 65 atoms of fcc256 in its box: rows of every length from 0 up
    pos, box = _rattled_fcc()
    return _cutoff(pos[:65], box, np.zeros(3), PBC)


_BUILDERS = dict(fcc256=_fcc256, fcc250_open_z=_fcc250_open_z, tri256=_tri256, sc125=_sc125, knn12_rc=_knn12_rc, single=_single, n65=_n65)
CASES = list(_BUILDERS)
# Cubic point symmetry makes the unweighted q_l of a perfect cubic lattice vanish for every odd l and for l = 2: w_l-hat is 0/0 there.  No seed
# changes that, so the cap on rows whose w_l-hat is not compared cannot hold for these degrees; instead the exact q_l is asserted
# to vanish on every row (and the library's q_l, q_lm and w_l are compared with it like any others).
ZERO_BY_SYMMETRY = {"sc125": {1, 2, 3, 5, 7, 9, 11}}


@functools.lru_cache(maxsize=None)
def case(name):
    c = _BUILDERS[name]()
    c.name = name
    c.N = len(c.x)
    c.bonds = R.Bonds(c.x, c.y, c.z, c.box, c.org, c.bnd, c.v, c.d, c.n, c.nnn, c.rc, c.use_voronoi)
    c.weight = 1.0 - np.random.default_rng(8).random(c.v.shape)  # (0, 1]
    return c


def launch_path(llist, lmax, variant, full):
    """the kernels ``mdh_get_sq`` launches for this call, from its own arithmetic: 'stage 1 + stage 3'"""
    stride = len(llist) * (2 * lmax + 1)
    special = variant != 1 and all(2 <= l <= 8 or l in (10, 12) for l in llist)
    if special and list(llist) == [4, 6]:
        one = "pair"
    elif special:
        one = "per_degree"
    else:
        bd = min(65536 // (16 * stride) // 64 * 64, 256)
        one = f"generic_lds{bd}" if bd >= 64 else "generic_global"
    if special and not full:
        return one + "+fused_ql"
    return one + ("+final_staged" if 65 * 16 * stride <= 60 * 1024 else "+final_global")


# (degrees, lmax, variant of mdh_debug_set_sq_variant).  The path of each is in its test id: with (w_l, w_l-hat, averaging) all
# on, then with all off.
LISTS = [
    ([4, 6], 6, 0),                          # both degrees in one launch
    ([6, 4], 6, 0),                          # per degree: the order of the list is the order of the slots
    ([2], 2, 0), ([3], 3, 0), ([4], 4, 0), ([5], 5, 0), ([6], 6, 0), ([7], 7, 0), ([8], 8, 0), ([10], 10, 0), ([12], 12, 0),
    ([6], 8, 0),                             # lmax above the degree: 17 slots per row, 13 used
    ([0], 0, 0), ([1], 1, 0),                # stride 1, 3: generic kernel, 256 threads
    ([9], 9, 0),                             # stride 19: 192 threads
    ([11], 11, 0),                           # stride 23: 128 threads
    ([9, 11], 11, 0),                        # stride 46: 64 threads
    ([4, 9], 9, 0),                          # a compiled and an uncompiled degree: the whole list goes generic (stride 38: 64 threads)
    ([2, 3, 5, 7, 8, 10, 12], 12, 0),        # stride 175: seven per-degree launches, stage 3 reads global memory
    ([2, 3, 5, 7, 8, 10, 12], 12, 1),        # the same through the generic kernel without LDS accumulators
]
HIGH_DEGREE = ([16], 16, 0)                  # stride 33: 64 threads; the 3j table of l = 16 takes a moment, so one case only


def list_id(entry):
    ls, lmax, variant = entry
    name = "l" + "_".join(str(l) for l in ls) + (f"_lmax{lmax}" if lmax != max(ls) else "") + ("_variant1" if variant else "")
    return f"{name}-{launch_path(ls, lmax, variant, True)}-{launch_path(ls, lmax, variant, False)}"


COMBOS = [(full, use_w) for full in (True, False) for use_w in (False, True)]


def call(backend, c, llist, lmax, full, use_w, start=None):
    """get_sq of ``backend`` (the oracle module or mdapy_amd._sbo) -> (qlm_r, qlm_i, qn)"""
    nl = len(llist)
    qr = np.zeros((c.N, nl, 2 * lmax + 1)); qi = np.zeros_like(qr); qn = np.zeros((c.N, nl * (3 if full else 1)))
    if start is not None:
        qr[...], qi[...] = start
    backend.get_sq(c.x, c.y, c.z, c.box, c.org, c.bnd, c.v, c.d, c.n, c.weight if use_w else np.zeros((2, 2)), np.array(llist, np.int32),
                   c.nnn, lmax, full, full, full, c.use_voronoi, c.rc, use_w, qr, qi, qn, 1)
    return qr, qi, qn


def measure(backend, c, entry):
    """one (case, degree list) through all four combinations of (w_l, w_l-hat, averaging) x weights against the exact values
    -> dict kind -> largest absolute error.  Asserts the NaN pattern and the cap on rows whose w_l-hat is not compared."""
    llist, lmax, _ = entry
    worst = {}
    for full, use_w in COMBOS:
        exact = R.exact_columns(c.bonds, llist, c.weight if use_w else None, full)
        if lmax != max(llist):  # wider rows than the degrees need
            wide = np.zeros((c.N, len(llist), 2 * lmax + 1), np.complex128)
            wide[:, :, :exact["qlm"].shape[2]] = exact["qlm"]
            exact["qlm"] = wide
        qr, qi, qn = call(backend, c, llist, lmax, full, use_w)
        err, left_out, finite = R.errors(exact, qr, qi, qn, full, full)
        for il, l in enumerate(llist):
            if not use_w and l in ZERO_BY_SYMMETRY.get(c.name, ()):  # (random weights break the symmetry)
                assert exact["ql"][:, il].max() < 1e-14, f"l = {l}: q_l of the perfect lattice should vanish"
            else:
                assert left_out[il] <= R.MAX_LEFT_OUT * finite[il], f"l = {l}: {left_out[il]} of {finite[il]} rows have q_l <= {R.QL_FLOOR}"
        for k, e in err.items():
            worst[k] = max(worst.get(k, 0.0), e)
    return worst


# ---- solid / liquid
def _half_molten():
    pos, box = lattice_positions("fcc", A_FCC, 4, 4, 4)
    rng = np.random.default_rng(2)
    hot = pos[:, 2] > 0.49 * box[2, 2]  # the four upper layers of eight: 128 atoms
    pos = pos + rng.normal(0.0, 0.04, pos.shape)
    pos[hot] += rng.normal(0.0, 0.5, (128, 3))
    return pos, box


@functools.lru_cache(maxsize=None)
def solid_liquid_cases():
    """the 256-atom fcc with half its atoms displaced by sigma = 0.5, on cutoff rows and on the 12 nearest with a finite cutoff
    -> [(name, case)]; c.bonds is the yardstick's view of the list"""
    pos, box = _half_molten()
    out = [("cutoff", _cutoff(pos, box, np.zeros(3), PBC)), ("nearest12_rc", _nearest(pos, box, np.zeros(3), PBC, 12, 3.0))]
    for _, c in out:
        c.N = len(c.x)
        c.bonds = R.Bonds(c.x, c.y, c.z, c.box, c.org, c.bnd, c.v, c.d, c.n, c.nnn, c.rc)
    return out


SLOTS = [(0, [6], 6), (2, [4, 5, 6], 6), (1, [4, 6, 8], 8)]  # (q6index, llist, lmax)
THRESHOLD, N_BOND = 0.7, 7


def solid_liquid_inputs(c, llist, lmax):
    """(qlm_r, qlm_i (N, nl, 2 lmax + 1), Q6, exact q_6m (N, 13)) from the exact module, for identifySolidLiquid"""
    exact = R.exact_columns(c.bonds, llist)
    wide = np.zeros((c.N, len(llist), 2 * lmax + 1), np.complex128)
    wide[:, :, :exact["qlm"].shape[2]] = exact["qlm"]
    at = llist.index(6)
    return np.ascontiguousarray(wide.real), np.ascontiguousarray(wide.imag), np.ascontiguousarray(exact["ql"][:, at]), exact["qlm"][:, at, :13]


def check_solid_liquid(backend, name, c, slot):
    q6index, llist, lmax = slot
    qr, qi, Q6, q6m = solid_liquid_inputs(c, llist, lmax)
    want_sl, want_nb, gap = c.bonds.solid_liquid(q6m, THRESHOLD, N_BOND)
    print(f"steinhardt solid/liquid {name} {llist}: rows {np.bincount(c.bonds.listed.sum(axis=1)).nonzero()[0].tolist()}, "
          f"solid {int(want_sl.sum())} of {c.N}, smallest |s_ij - threshold| {gap:.2e}")
    assert gap >= 1e-9, "a bond sits on the threshold: choose another seed"
    assert 0.25 * c.N < want_sl.sum() < 0.75 * c.N
    sl = np.zeros(c.N, np.int32); nb = np.zeros(c.N, np.int32)
    backend.identifySolidLiquid(q6index, Q6, c.v, c.d, c.n, qr, qi, THRESHOLD, N_BOND, sl, nb, False, c.nnn, c.rc, 1)
    assert np.array_equal(nb, want_nb) and np.array_equal(sl, want_sl)
