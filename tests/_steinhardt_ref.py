"""The Steinhardt bond-orientational order parameters restated from their definition, for the Steinhardt tests: the yardstick.

Nothing here is a recurrence of the library's.  A bond's Y_lm comes from ``scipy.special.sph_harm_y``, the Wigner 3j symbols
are sympy's exact values, sums run in extended precision (``numpy.longdouble``) and are rounded to double once:

    q_lm(i)  = sum_j w_ij Y_lm(r_ij) / sum_j w_ij           over the entries of row i that ``get_sq`` selects
    averaged = (q_lm(i) + sum_j q_lm(j)) / (1 + #j)          over the listed indices of row i (Lechner-Dellago)
    q_l      = sqrt(4 pi / (2l+1) * sum_m |q_lm|^2)
    w_l      = sum_{m1+m2+m3=0} (l l l; m1 m2 m3) q_lm1 q_lm2 q_lm3
    w_l-hat  = w_l / (sum_m |q_lm|^2)^(3/2)

Which entries count (read from ``mdh_get_sq``): the first ``nnn`` entries of a row, or the first ``neighbor_number[i]`` when
``nnn`` is 0 or ``use_voronoi`` is set; of those the *listed* ones have ``0 <= j < N``; of those the *selected* ones have
``1e-15 < d <= rc``.  Stage 1 sums over the selected entries, the average over the listed ones, the solid/liquid bond count over
the listed ones with ``d <= rc``.  The bond vector is the minimum image formed here in float64 from the positions; the module
asserts that its length equals the list's distance to 1e-12 — if that fails the yardstick has the wrong image, not the kernel.

Convention: the library's q_lm carries no Condon-Shortley phase, q_lm(library) = (-1)^m q_lm(scipy).  ``Bonds.order`` returns the
library's convention; q_l, w_l and w_l-hat do not depend on it.  An atom without a selected entry has 0/0 = NaN everywhere;
``get_sq`` writes w_l-hat only where q_l > 1e-15, which is false for NaN: such a row keeps the caller's content there
(``errors`` checks that it does).

Bounds of the GPU tests.  tests/test_steinhardt_host.py measures the largest absolute error of the CPU oracle
(oracle/mdapy_oracle.c, the same recurrences as the kernels in plain C) against this module, per kind of output, over every
case and degree list of tests/_steinhardt_cases.py, and asserts that it stays within ORACLE_ERR below.  A kernel may be 64 times
as far away (device sqrt, division and FMA contraction moving each of up to about 13 x (2l+1) terms by a few ulp), and never
farther than CEILING = 1e-12, the absolute tolerance the project has always used for these columns."""
import functools

import numpy as np
from scipy.special import sph_harm_y
from sympy.physics.wigner import wigner_3j

EPS = 1e-15
QL_FLOOR = 1e-3        # w_l-hat is compared where the exact q_l exceeds this ...
MAX_LEFT_OUT = 0.02    # ... and at most this share of the finite rows may fall under it
CEILING = 1e-12

# Largest |oracle - exact| measured by tests/test_steinhardt_host.py over all cases x all degree lists x weights on/off x
# (w_l, w_l-hat, averaging) on/off.  The comment is the measurement and where it occurred, the constant is it rounded up.
ORACLE_ERR = {
    "qlm": 1.2e-14,  # 1.10e-14: perfect simple cubic, l = 12 (next: 6.0e-15, sheared box, l = 11)
    "ql": 7.5e-15,   # 6.88e-15: perfect simple cubic, l = 12 (next: 4.1e-15, sheared box, l = 7)
    "wl": 6.0e-16,   # 5.62e-16: perfect simple cubic, l = 12 (rattled cases: 7.5e-17)
    "wlh": 1.5e-14,  # 1.44e-14: simple cubic with random weights, l = 2, where q_2 is small (rattled cases: 4.5e-15, l = 2)
}
FACTOR = 64
BOUND = {kind: FACTOR * err for kind, err in ORACLE_ERR.items()}
assert all(b <= CEILING for b in BOUND.values())

_ld, _cld = np.longdouble, np.clongdouble


@functools.lru_cache(maxsize=None)
def three_j(l):
    """(2l+1, 2l+1) float64: (l l l; m1 m2 -m1-m2) at [m1 + l, m2 + l], 0 where |m1 + m2| > l — exact values, rounded once"""
    t = np.zeros((2 * l + 1, 2 * l + 1))
    for m1 in range(-l, l + 1):
        for m2 in range(max(-l, -l - m1), min(l, l - m1) + 1):
            t[m1 + l, m2 + l] = float(wigner_3j(l, l, l, m1, m2, -m1 - m2).evalf(30))
    return t


def _minimum_image(box, boundary):
    h = np.asarray(box, np.float64).reshape(3, 3)
    inverse = np.linalg.inv(h)
    periodic = np.asarray(boundary).astype(bool)

    def image(dr):  # whole lattice vectors are taken off: the bond itself is not sent through the matrix pair
        shifts = np.where(periodic, np.round(dr @ inverse), 0.0)
        return dr - shifts @ h
    return image


class Bonds:
    """the bonds of one list on one system; harmonics are computed once per degree and kept"""

    def __init__(self, x, y, z, box, origin, boundary, verlet_list, distance_list, neighbor_number, nnn, rc, use_voronoi=False):
        pos = np.stack([np.asarray(a, np.float64) for a in (x, y, z)], axis=1)
        v = np.asarray(verlet_list, np.int64)
        d = np.asarray(distance_list, np.float64)
        N, M = v.shape
        assert pos.shape == (N, 3) and d.shape == (N, M)
        count = np.asarray(neighbor_number, np.int64) if (use_voronoi or nnn <= 0) else np.full(N, int(nnn), np.int64)
        assert count.max(initial=0) <= M
        self.N, self.M, self.rc = N, M, float(rc)
        self.listed = (np.arange(M)[None, :] < count[:, None]) & (v >= 0) & (v < N)
        self.selected = self.listed & (d > EPS) & (d <= rc)
        self.near = self.listed & (d <= rc)
        self.j = np.where(self.listed, v, np.arange(N)[:, None])
        dr = _minimum_image(box, boundary)(pos[self.j] - pos[:, None, :])
        length = np.sqrt((dr * dr).sum(axis=2))
        if self.selected.any():
            off = np.abs(length - d)[self.selected].max()
            assert off <= 1e-12, f"the yardstick's bonds are not the list's: lengths differ by {off:.3g}"
        self.theta = np.arctan2(np.hypot(dr[..., 0], dr[..., 1]), dr[..., 2])
        self.phi = np.arctan2(dr[..., 1], dr[..., 0])
        self._harmonics = {}

    def harmonics(self, l):
        """(N, M, 2l+1) complex: Y_lm of every bond, m = -l .. l, scipy's (Condon-Shortley) convention"""
        if l not in self._harmonics:
            m = np.arange(-l, l + 1)
            self._harmonics[l] = sph_harm_y(l, m[None, None, :], self.theta[..., None], self.phi[..., None])
        return self._harmonics[l]

    def _mean(self, l, weight):
        w = np.where(self.selected, 1.0 if weight is None else np.asarray(weight, np.float64), 0.0).astype(_ld)
        total = (w[..., None] * self.harmonics(l).astype(_cld)).sum(axis=1)
        with np.errstate(invalid="ignore", divide="ignore"):
            return total / w.sum(axis=1)[:, None]

    def _averaged(self, q):
        """q must be finite where it is used: a NaN row spreads to every atom that lists it, as in the library"""
        total = q + np.where(self.listed[..., None], q[self.j], 0.0).sum(axis=1)
        return total / (1 + self.listed.sum(axis=1)).astype(_ld)[:, None]

    def order(self, l, weight=None, average=False):
        """-> dict(qlm (N, 2l+1) complex in the LIBRARY's convention, ql, wl, wlh (N,)), float64 / complex128"""
        q = self._mean(l, weight)
        if average:
            q = self._averaged(q)
        power = (q.real * q.real + q.imag * q.imag).sum(axis=1)
        table = three_j(l)
        w = np.zeros(self.N, _cld)
        for m1 in range(-l, l + 1):
            for m2 in range(max(-l, -l - m1), min(l, l - m1) + 1):
                w += table[m1 + l, m2 + l] * q[:, m1 + l] * q[:, m2 + l] * q[:, l - m1 - m2]
        with np.errstate(invalid="ignore", divide="ignore"):
            hat = w.real / power ** _ld(1.5)
        sign = np.where(np.arange(-l, l + 1) % 2 == 0, 1.0, -1.0)
        return dict(qlm=(q * sign).astype(np.complex128), ql=np.sqrt(4 * _ld(np.pi) / (2 * l + 1) * power).astype(np.float64),
                    wl=w.real.astype(np.float64), wlh=hat.astype(np.float64))

    def solid_liquid(self, q6m, threshold, n_bond):
        """the q6-q6 bond rule on q_6m (N, 13) complex (either convention: the phase cancels)
        -> (solidliquid, nbond (N,) int32, the smallest |s_ij - threshold| over the counted entries)"""
        q = np.asarray(q6m).astype(_cld)
        size = np.sqrt((q.real * q.real + q.imag * q.imag).sum(axis=1))
        with np.errstate(invalid="ignore", divide="ignore"):
            s = (q[:, None, :] * np.conj(q[self.j])).sum(axis=2).real / (size[:, None] * size[self.j])
            bonded = self.near & (s > threshold)
        nbond = bonded.sum(axis=1).astype(np.int32)
        first = nbond >= n_bond
        solid = first & (self.listed & first[self.j]).any(axis=1)
        gap = np.abs(np.where(self.near & np.isfinite(s), s, np.inf) - threshold).min(initial=np.inf)
        return solid.astype(np.int32), nbond, float(gap)


def exact_columns(bonds, llist, weight=None, average=False):
    """the exact values in the shapes ``get_sq`` writes for ``llist``: qlm (N, nl, 2*max(l)+1) complex, zero in the slots past a
    degree's 2l+1 (the library leaves those alone), and q_l, w_l, w_l-hat (N, nl) each"""
    llist = [int(l) for l in llist]
    out = dict(llist=llist, qlm=np.zeros((bonds.N, len(llist), 2 * max(llist) + 1), np.complex128))
    out.update({k: np.zeros((bonds.N, len(llist))) for k in ("ql", "wl", "wlh")})
    for il, l in enumerate(llist):
        got = bonds.order(l, weight, average)
        out["qlm"][:, il, :2 * l + 1] = got["qlm"]
        for k in ("ql", "wl", "wlh"):
            out[k][:, il] = got[k]
    return out


def errors(exact, qlm_r, qlm_i, qn, wl, wlhat):
    """``get_sq`` output (arrays that went in as zeros) against ``exact_columns``.  Asserts what is no matter of tolerance —
    equal NaN masks, the slots past 2l+1 still zero, w_l-hat still zero in a row whose q_l is NaN — and returns
    (dict kind -> largest absolute error, for the kinds computed; left_out (nl,) rows whose w_l-hat was not compared because
    the exact q_l is at most QL_FLOOR; finite (nl,) rows with a finite exact q_l)"""
    llist, nl = exact["llist"], len(exact["llist"])
    got = np.asarray(qlm_r) + 1j * np.asarray(qlm_i)
    qn = np.asarray(qn)
    assert got.shape == exact["qlm"].shape and qn.shape == (got.shape[0], nl * (1 + bool(wl) + bool(wlhat)))
    worst = dict(qlm=0.0, ql=0.0)
    for il, l in enumerate(llist):
        k = 2 * l + 1
        a, b = got[:, il, :k], exact["qlm"][:, il, :k]
        assert np.array_equal(np.isnan(a.real) | np.isnan(a.imag), np.isnan(b.real) | np.isnan(b.imag)), f"q_{l}m: NaN masks differ"
        assert not got[:, il, k:].any(), f"q_{l}m: a slot past 2l+1 was written"
        ok = ~np.isnan(b.real)
        worst["qlm"] = max(worst["qlm"], float(np.abs(a - b)[ok].max(initial=0.0)))
    finite = ~np.isnan(exact["ql"])
    blocks = [("ql", qn[:, :nl])] + ([("wl", qn[:, nl:2 * nl])] if wl else [])
    for kind, have in blocks:
        assert np.array_equal(np.isnan(have), ~finite), f"{kind}: NaN masks differ"
        worst[kind] = float(np.abs(have - exact[kind])[finite].max(initial=0.0))
    left_out = np.zeros(nl, np.int64)
    if wlhat:
        have = qn[:, (2 if wl else 1) * nl:]
        assert not have[~finite].any(), "w_l-hat of a row without q_l was written"
        compared = finite & (exact["ql"] > QL_FLOOR)
        assert np.isfinite(have[compared]).all(), "w_l-hat: not finite where q_l is"
        worst["wlh"] = float(np.abs(have - exact["wlh"])[compared].max(initial=0.0))
        left_out = (finite & ~compared).sum(axis=0)
    return worst, left_out, finite.sum(axis=0)
