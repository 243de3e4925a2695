"""A numpy restatement of the reference's CHILL+ (src/chill_plus.cpp:27-179) for the CHILL+ tests: the yardstick.

Same call signature as ``mdapy_amd._chill_plus.compute_chill_plus`` (it can stand in for ``kernels.chill_plus``).  A loop over
the slot index, vectorised over atoms.  It is NOT bitwise the reference: everything is float64 (the reference and the kernel
work in float32 behind the minimum image) and e^{i phi} is (dx + i dy) / |(dx, dy)| without trigonometry.  The normalisation
constants and the three thresholds are the reference's float32 values, widened.

A label is three integer counts of comparisons of a bond's c against a threshold, so float32 and float64 can only disagree on an
atom one of whose bonds has c on a threshold to within single-precision noise.  ``analyse`` flags those atoms ``ambiguous``:
some bond's c within BAND = 5e-6 of a threshold (the largest |c32 - c64| seen over the test inputs was 8.4e-7).  The rule of the
tests: every atom that is not ambiguous carries the yardstick's label, and at most MAX_AMBIGUOUS of the atoms are ambiguous.

A row entry jj < neighbor_number[i] is a bond iff distance_list[i, jj] <= rc and verlet_list[i, jj] >= 0; a rejected entry is
passed over, the row goes on behind it."""
import numpy as np

from _bond_ref import _pbc

BAND = 5e-6
MAX_AMBIGUOUS = 0.005  # of N
_f32 = np.float32
LOW, HIGH, STAGGERED = float(_f32(-0.35)), float(_f32(0.25)), float(_f32(-0.8))
_PI = _f32(3.14159265358979323846)
N0 = float(_f32(0.25) * np.sqrt(_f32(7.0) / _PI))
N1 = float(_f32(0.125) * np.sqrt(_f32(21.0) / _PI))
N2 = float(_f32(0.25) * np.sqrt(_f32(105.0) / (_f32(2.0) * _PI)))
N3 = float(_f32(0.125) * np.sqrt(_f32(35.0) / _PI))


def _np(a):
    if hasattr(a, "numpy") and not isinstance(a, np.ndarray):
        a = a.numpy()
    return np.asarray(a.to_numpy() if hasattr(a, "to_numpy") else a)


def _y3m(dx, dy, dz):
    """(n, 7) complex: Y_3m of every bond vector, m = -3 .. 3 (Condon-Shortley); zeros for a bond of length 0"""
    r2 = dx * dx + dy * dy + dz * dz
    live = r2 > 0.0
    r = np.sqrt(np.where(live, r2, 1.0))
    ct = dz / r
    xy = np.sqrt(dx * dx + dy * dy)
    st = xy / r
    planar = xy > 0.0
    e1 = np.where(planar, (dx + 1j * dy) / np.where(planar, xy, 1.0), 1.0 + 0.0j)
    e2 = e1 * e1
    e3 = e2 * e1
    a1 = N1 * st * (5.0 * ct * ct - 1.0)
    a2 = N2 * st * st * ct
    a3 = N3 * st * st * st
    y = np.stack([a3 * np.conj(e3), a2 * np.conj(e2), a1 * np.conj(e1), N0 * (5.0 * ct * ct * ct - 3.0 * ct) + 0.0j,
                  -a1 * e1, a2 * e2, -a3 * e3], axis=1)
    return np.where(live[:, None], y, 0.0)


def _code(coordination, eclipsed, staggered):
    code = np.zeros(len(coordination), np.int32)
    open_ = coordination == 4
    for mask, value in ((eclipsed == 4, 4), (eclipsed == 3, 5), (staggered == 4, 2), ((staggered == 3) & (eclipsed == 1), 1),
                        ((staggered == 3) & (eclipsed == 0), 3), (staggered == 2, 3)):
        take = open_ & mask
        code[take] = value
        open_ = open_ & ~mask
    return code


def analyse(x, y, z, box, origin, boundary, verlet_list, distance_list, neighbor_number, rc):
    """-> (label (N,) int32, c (N, M) float64 with NaN where the entry is no bond, ambiguous (N,) bool)"""
    v = np.asarray(_np(verlet_list), np.int64)
    d = np.asarray(_np(distance_list), np.float64)
    N, M = v.shape
    nn = np.clip(np.asarray(_np(neighbor_number), np.int64), 0, M)
    pos = [np.asarray(_np(a), np.float64) for a in (x, y, z)]
    assert v.max(initial=-1) < N, "the restatement is for lists of this system"
    pbc = _pbc(_np(box), _np(boundary))
    i = np.arange(N)
    bond = (np.arange(M)[None, :] < nn[:, None]) & ~(d > float(rc)) & (v >= 0)
    j = np.where(bond, v, i[:, None])
    q = np.zeros((N, 7), np.complex128)
    for jj in range(M):
        dx, dy, dz = pbc(pos[0][j[:, jj]] - pos[0], pos[1][j[:, jj]] - pos[1], pos[2][j[:, jj]] - pos[2])
        q += np.where(bond[:, jj, None], _y3m(dx, dy, dz), 0.0)
    norm = np.sqrt((q.real * q.real + q.imag * q.imag).sum(axis=1))
    c = np.full((N, M), np.nan)
    for jj in range(M):
        qj = q[j[:, jj]]
        denom = norm * norm[j[:, jj]]
        dot = (q.real * qj.real + q.imag * qj.imag).sum(axis=1)
        value = np.where(denom > 0.0, dot / np.where(denom > 0.0, denom, 1.0), 0.0)
        c[:, jj] = np.where(bond[:, jj], value, np.nan)
    with np.errstate(invalid="ignore"):
        eclipsed = ((c > LOW) & (c < HIGH)).sum(axis=1)
        staggered = (c < STAGGERED).sum(axis=1)
        near = np.minimum(np.minimum(np.abs(c - LOW), np.abs(c - HIGH)), np.abs(c - STAGGERED)) <= BAND
    return _code(bond.sum(axis=1), eclipsed, staggered), c, near.any(axis=1)


def compute_chill_plus(x, y, z, box, origin, boundary, verlet_list, distance_list, neighbor_number, rc, pattern, num_t=1):
    labels = analyse(x, y, z, box, origin, boundary, verlet_list, distance_list, neighbor_number, rc)[0]
    if isinstance(pattern, np.ndarray):
        pattern[...] = labels
    else:  # (an output buffer in HBM, where a GPU is there)
        import torch

        pattern.dev().copy_(torch.from_numpy(np.ascontiguousarray(labels, np.int32)))
        pattern.invalidate_host()


def on_system_list(system, cutoff):
    """the yardstick on the list ``system`` remembers — ``as_numpy`` of its rows, distances and counts, in the compute view's
    numbering (the replica's for a thin box) — cut to the N real atoms"""
    from mdapy_amd.devarray import as_numpy

    cell, frame = system._get_compute_view()
    label, c, ambiguous = analyse(*(frame[k].to_numpy() for k in "xyz"), cell.box, cell.origin, cell.boundary,
                                  as_numpy(system.verlet_list), as_numpy(system.distance_list), as_numpy(system.neighbor_number), cutoff)
    n = system.N
    return label[:n], c[:n], ambiguous[:n]


def check(got, want, ambiguous, what=""):
    """the parity rule; prints the figures before it asserts"""
    got, want = np.asarray(got), np.asarray(want)
    n = len(want)
    differ = got != want
    print(f"chill {what}: N = {n}, ambiguous = {int(ambiguous.sum())}, differing = {int(differ.sum())} "
          f"(of them ambiguous {int((differ & ambiguous).sum())}), classes = {np.bincount(want, minlength=6).tolist()}")
    assert got.dtype == np.int32 and got.shape == (n,)
    assert ambiguous.sum() <= MAX_AMBIGUOUS * n, f"{int(ambiguous.sum())} of {n} atoms sit on a threshold"
    bad = np.flatnonzero(differ & ~ambiguous)
    assert bad.size == 0, f"{bad.size} unambiguous atoms differ, e.g. atom {bad[:5].tolist()}: got {got[bad[:5]].tolist()}, want {want[bad[:5]].tolist()}"
