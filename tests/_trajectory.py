"""Short trajectories for the tests of everything that carries state from one call to the next: a start frame
made from a seed, steps that turn one frame into the next, and the expected answer of ONE frame computed from that frame alone
by the oracle.  TEST INFRASTRUCTURE: plain numpy, importable without torch or a device; the oracle is loaded only by
``expected_*``.

Every atom set is rattled or random, so exact ties in distance do not occur and every comparison made with these frames is
bitwise.  The perfect lattice is left out on purpose (its tie order is a subject of its own)."""
from dataclasses import dataclass, replace

import numpy as np

PBC = (1, 1, 1)


@dataclass(frozen=True)
class Frame:
    pos: np.ndarray        # (N, 3) f64, not wrapped
    box: np.ndarray        # (3, 3) f64, rows are the cell vectors
    origin: np.ndarray     # (3,) f64
    boundary: np.ndarray   # (3,) i32, 1 = periodic

    @property
    def n(self):
        return len(self.pos)

    def xyz(self):
        return tuple(np.ascontiguousarray(self.pos[:, k]) for k in range(3))

    def where(self):
        """(x, y, z, box, origin, boundary): the leading arguments of every kernel and oracle call"""
        return (*self.xyz(), self.box, self.origin, self.boundary)

    def frac(self, axis=None):
        f = (self.pos - self.origin) @ np.linalg.inv(self.box)
        return f if axis is None else f[:, axis]


def _frame(pos, box, origin=None, boundary=PBC):
    return Frame(np.ascontiguousarray(pos, dtype=np.float64), np.ascontiguousarray(box, dtype=np.float64),
                 np.zeros(3) if origin is None else np.asarray(origin, np.float64), np.asarray(boundary, np.int32))


# ---------------------------------------------------------------------------------------------------------------- start frames
def start(kind, cells, seed, a=3.615, rattle=0.07, shuffle=True):
    """kind: "fcc" / "bcc" (rattled by `rattle` A, a normal displacement per coordinate) or "gas" (uniform, at the density of the
    fcc crystal of the same cells).  cells: (nx, ny, nz) unit cells of edge a.  shuffle: atoms in no spatial order."""
    rng = np.random.default_rng(seed)
    nx, ny, nz = cells
    box = np.diag([nx * a, ny * a, nz * a])
    if kind == "gas":
        pos = rng.random((4 * nx * ny * nz, 3)) * np.diag(box)
    else:
        basis = {"fcc": [[0, 0, 0], [0.5, 0.5, 0], [0.5, 0, 0.5], [0, 0.5, 0.5]], "bcc": [[0, 0, 0], [0.5, 0.5, 0.5]]}[kind]
        grid = np.stack(np.meshgrid(np.arange(nx), np.arange(ny), np.arange(nz), indexing="ij"), -1).reshape(-1, 1, 3)
        pos = ((grid + np.asarray(basis)[None]) * a).reshape(-1, 3) + rng.normal(0.0, rattle, (len(grid) * len(basis), 3))
    if shuffle:
        pos = pos[rng.permutation(len(pos))]
    return _frame(pos, box)


def decomposed_frame():
    """(frame, rc) of the 21 952-atom system of tests/test_gpu_distributed.py: rattled fcc, some atoms outside the box, 3 % displaced
    by half an angstrom, arbitrary numbering; rc = the first-shell cutoff of the fixed-cutoff CNA"""
    from test_gpu_distributed import _system

    pos, _, boxm, a = _system()
    return _frame(pos, boxm), 0.854 * a


# ---------------------------------------------------------------------------------------------------------------- boxes
def sheared(frame, tilt=(0.10, -0.05, 0.10), origin=(2.0, -7.5, 11.0)):
    """the same fractional coordinates in a sheared box (xy, xz, yz tilts as fractions of the edge) at another origin"""
    h = frame.box.copy()
    h[1, 0], h[2, 0], h[2, 1] = tilt[0] * h[0, 0], tilt[1] * h[0, 0], tilt[2] * h[1, 1]
    org = np.asarray(origin, np.float64)
    return replace(frame, pos=np.ascontiguousarray(frame.frac() @ h + org), box=h, origin=org)


def open_along(frame, axis):
    b = frame.boundary.copy()
    b[axis] = 0
    return replace(frame, boundary=b)


# ---------------------------------------------------------------------------------------------------------------- steps
def drift(frame, rng, sigma=0.04):
    """every atom moves a fraction of a cell"""
    return replace(frame, pos=frame.pos + rng.normal(0.0, sigma, frame.pos.shape))


def jump(frame, rng, share=0.03):
    """a few per cent of the atoms move by whole box vectors along periodic axes (unwrapped coordinates)"""
    who = rng.random(frame.n) < share
    m = rng.integers(-2, 3, (frame.n, 3)) * who[:, None] * frame.boundary[None, :]
    return replace(frame, pos=frame.pos + m @ frame.box)


def renumber(frame, rng):
    """the same atoms in another permutation"""
    return replace(frame, pos=np.ascontiguousarray(frame.pos[rng.permutation(frame.n)]))


def resize(frame, rng, share=0.9):
    """N changes: a random subset of the atoms, in the order they had"""
    keep = np.sort(rng.choice(frame.n, int(frame.n * share), replace=False))
    return replace(frame, pos=np.ascontiguousarray(frame.pos[keep]))


def reshape(frame, rng, strain=(1.03, 0.98, 1.01)):
    """the same N and boundary in another box matrix (an affine strain: the atoms keep their fractional coordinates)"""
    h = frame.box * np.asarray(strain)[None, :]
    return replace(frame, pos=np.ascontiguousarray(frame.frac() @ h + frame.origin), box=np.ascontiguousarray(h))


def repbc(frame, rng, boundary=(1, 1, 0)):
    """the same N and box with another boundary"""
    return replace(frame, boundary=np.asarray(boundary, np.int32))


def nan_atom(frame, rng, coordinate=0):
    """one coordinate of one atom becomes NaN (column 0, x, is the one the neighbor builds read as "this atom is absent")"""
    pos = frame.pos.copy()
    pos[int(rng.integers(frame.n)), coordinate] = np.nan
    return replace(frame, pos=pos)


def gap(frame, axis, faces, width, shift=1.2):
    """atoms within `width` (a distance, measured along the normal of the planes) of the fractional planes `faces` of `axis` move
    away from the plane, along the cell vector of `axis`, by shift * width > width: none crosses a plane, so the slab that owns
    every atom stays the same, and nothing is left within `width` of a plane (the ghost layers of a slab decomposition with these
    faces are empty).  Planes are periodic images of each other (0 and 1 are the same plane)."""
    inv = np.linalg.inv(frame.box)
    thick = 1.0 / np.linalg.norm(inv[:, axis])      # distance between the planes f = 0 and f = 1
    f = frame.frac(axis)
    f = f - np.floor(f)
    w = width / thick
    move = np.zeros(frame.n)
    for face in faces:
        d = f - face
        d = d - np.rint(d)                            # signed fractional distance to the nearest image of the plane
        near = np.abs(d) < w
        assert not (near & (move != 0)).any(), "the planes are closer than two widths"
        move[near] = np.where(d[near] >= 0, shift * w, -shift * w)
    return replace(frame, pos=np.ascontiguousarray(frame.pos + move[:, None] * frame.box[axis][None, :]))


STEPS = {"drift": drift, "jump": jump, "renumber": renumber, "resize": resize, "reshape": reshape, "repbc": repbc, "nan_atom": nan_atom}


def sequence(first, steps, seed):
    """[first, step_1(first), step_2(...), ...]; a step is a name of STEPS or a callable (frame, rng) -> frame"""
    rng = np.random.default_rng(seed)
    out = [first]
    for s in steps:
        out.append((STEPS[s] if isinstance(s, str) else s)(out[-1], rng))
    return out


# ---------------------------------------------------------------------------------------------------------------- expected answers
def finite(frame):
    return np.isfinite(frame.pos).all(axis=1)


def _over_finite(frame):
    ok = finite(frame)
    ids = np.nonzero(ok)[0].astype(np.int32)
    return ok, ids, replace(frame, pos=np.ascontiguousarray(frame.pos[ok]))


def expected_cutoff(frame, rc, threads=8):
    """exact-width rows, distances, counts and fixed-cutoff CNA labels of this frame alone (the oracle: neighbor.cpp + cna.cpp).  An
    atom with a non-finite coordinate is left out of the search: no row (pads -1 / rc + 1, count 0, label 0) and in nobody's row."""
    from oracle import oracle as O

    ok, ids, sub = _over_finite(frame)
    v, d, nn = O.build_neighbor_without_max_neigh(*sub.where(), rc, threads)
    pat = np.zeros(sub.n, np.int32)
    O.fcna(*sub.where(), v, nn, pat, rc, threads)
    if ok.all():
        return {"rows": v, "dist": d, "counts": nn, "cna": pat}
    rows = np.full((frame.n, v.shape[1]), -1, np.int32)
    dist = np.full((frame.n, v.shape[1]), rc + 1.0)
    counts, labels = np.zeros(frame.n, np.int32), np.zeros(frame.n, np.int32)
    rows[ok] = np.where(v >= 0, ids[np.clip(v, 0, None)], -1)
    dist[ok], counts[ok], labels[ok] = d, nn, pat
    return {"rows": rows, "dist": dist, "counts": counts, "cna": labels}


def expected_knn(frame, k, threads=8, csp=None):
    """the k nearest of every finite atom among the finite atoms (the oracle's brute-force search, fast_knn.cpp); rows of the other
    atoms are not defined here (`finite` says which).  csp = m: the centro-symmetry parameter over the first m as well."""
    from oracle import oracle as O

    ok, ids, sub = _over_finite(frame)
    idx, dist = np.zeros((sub.n, k), np.int32), np.zeros((sub.n, k))
    O.knn(*sub.where(), k, idx, dist, threads)
    out = {"finite": ok, "rows": np.full((frame.n, k), -1, np.int32), "dist": np.full((frame.n, k), np.nan)}
    out["rows"][ok], out["dist"][ok] = ids[idx], dist
    if csp is not None:
        c = np.zeros(sub.n)
        O.get_csp(*sub.where(), idx, csp, c, threads)
        out["csp"] = np.full(frame.n, np.nan)
        out["csp"][ok] = c
    return out
