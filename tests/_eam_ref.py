"""A numpy restatement of the reference's EAM calculator for the EAM tests: the reader's section logic
(src/mdapy/eam.py:141-219), the spline constructor and ``locate`` (src/spline.h:394-500) and the two passes of
``EAM::calculate`` (src/eam.cpp:85-182).

Class ``EAM`` has the constructor and the ``calculate`` of ``mdapy_amd._eam.EAM`` (the module can stand in for ``kernels.eam``).
The passes are a loop over the slot index, vectorised over atoms: every per-atom sum is accumulated in list order, every
floating-point expression is the reference's, operation for operation.  numpy does not fuse a product into an add, so this is the
bitwise yardstick.  A row is ``neighbor_number[i]`` entries long and ends early at an entry outside [0, N), which the library
never dereferences; an atom whose type is outside the potential contributes nothing and receives nothing."""
import gzip
import math
import os

import numpy as np

from _bond_ref import _pbc

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "eam")
# the reference's three LAMMPS cases (tests/golden/eam/README.md): potential file, fcc cells per edge, elements, ratios, noise
CASES = {1: ("CoNiFeAlCu.eam.alloy.gz", 3, ["Co", "Ni", "Fe", "Al", "Cu"], [0.25, 0.25, 0.25, 0.075, 0.175], False),
         2: ("NiCoCr.lammps.eam.gz", 4, ["Co", "Ni", "Cr"], [0.2, 0.3, 0.5], True),
         3: ("FeNiCrCoTi-heamix.setfl.gz", 4, ["Co", "Ni", "Cr"], [0.2, 0.3, 0.5], True)}
calls = {"calculate": 0}  # (how often EAM.calculate ran: the host tests count calculations)


def _np(a):
    if hasattr(a, "numpy") and not isinstance(a, np.ndarray):
        a = a.numpy()
    return np.asarray(a.to_numpy() if hasattr(a, "to_numpy") else a)


# ------------------------------------------------------------------------------------------------ the file
def read_setfl(filename):
    """-> dict(header, elements, nrho, drho, nr, dr, rc, F_rho, rho_r, rphi_r)"""
    opener = gzip.open if str(filename).endswith(".gz") else open
    with opener(filename, "rt") as f:
        lines = f.readlines()
    nelem = int(lines[3].split()[0])
    elements = lines[3].split()[1:1 + nelem]
    five = lines[4].split()
    nrho, drho, nr, dr, rc = int(five[0]), float(five[1]), int(five[2]), float(five[3]), float(five[4])
    at = 5

    def section(n):
        nonlocal at
        got = []
        while len(got) < n and at < len(lines):
            for token in lines[at].split("#")[0].split():
                if len(got) >= n:
                    break
                try:
                    got.append(float(token))
                except ValueError:
                    break
            at += 1  # (what is left on the section's last line is dropped)
        assert len(got) == n, f"{filename}: a section of {n} values ended after {len(got)}"
        return np.array(got)

    F_rho, rho_r = np.zeros((nelem, nrho)), np.zeros((nelem, nr))
    for e in range(nelem):
        at += 1
        F_rho[e] = section(nrho)
        rho_r[e] = section(nr)
    rphi_r = np.zeros((nelem, nelem, nr))
    for i in range(nelem):
        for j in range(i + 1):
            rphi_r[i, j] = section(nr)
            rphi_r[j, i] = rphi_r[i, j]
    return dict(header=lines[:3], elements=elements, nrho=nrho, drho=drho, nr=nr, dr=dr, rc=rc, F_rho=F_rho, rho_r=rho_r, rphi_r=rphi_r)


# ------------------------------------------------------------------------------------------------ the spline
class Spline:
    """UniformCubicSpline (src/spline.h:394-500) of one table, evaluated over arrays"""

    def __init__(self, h, y):
        y = [float(v) for v in y]
        n = len(y)
        assert h > 0.0 and n >= 2
        fp = [0.0] * n
        fp[0] = y[1] - y[0]
        fp[n - 1] = y[n - 1] - y[n - 2]
        if n >= 3:
            fp[1] = 0.5 * (y[2] - y[0])
            fp[n - 2] = 0.5 * (y[n - 1] - y[n - 3])
        for m in range(2, n - 2):
            fp[m] = ((y[m - 2] - y[m + 2]) + 8.0 * (y[m + 1] - y[m - 1])) / 12.0
        a, b, c, d = [0.0] * n, [0.0] * n, [0.0] * n, [0.0] * n
        inv_h = 1.0 / h
        inv_h2 = inv_h * inv_h
        inv_h3 = inv_h2 * inv_h
        for m in range(n - 1):
            dy = y[m + 1] - y[m]
            B2 = 3.0 * dy - 2.0 * fp[m] - fp[m + 1]
            B3 = fp[m] + fp[m + 1] - 2.0 * dy
            a[m], b[m], c[m], d[m] = y[m], fp[m] * inv_h, B2 * inv_h2, B3 * inv_h3
        a[n - 1], b[n - 1], c[n - 1], d[n - 1] = y[n - 1], fp[n - 1] * inv_h, 0.0, 0.0
        self.h, self.n, self.fp = float(h), n, np.array(fp)
        self.a, self.b, self.c, self.d = (np.array(v) for v in (a, b, c, d))

    def locate(self, x):
        x = np.asarray(x, np.float64)
        with np.errstate(invalid="ignore", over="ignore"):
            m = np.trunc(x / self.h)
        m = np.where(np.isnan(m), 0.0, np.clip(m, -1.0, float(self.n)))  # ((int) saturates; beyond the clamps nothing differs)
        m = m.astype(np.int64)
        below = m < 0
        m = np.minimum(np.where(below, 0, m), self.n - 1)
        dx = np.where(below, 0.0, x - m * self.h)
        return m, dx

    def evaluate(self, x):
        m, dx = self.locate(x)
        return self.a[m] + (self.b[m] + (self.c[m] + self.d[m] * dx) * dx) * dx

    def derivative(self, x):
        m, dx = self.locate(x)
        return self.b[m] + (2.0 * self.c[m] + 3.0 * self.d[m] * dx) * dx

    def evaluate_and_derivative(self, x):
        return self.evaluate(x), self.derivative(x)


# ------------------------------------------------------------------------------------------------ the calculator
class EAM:
    def __init__(self, rc, dr, drho, F_rho, rho_r, rphi_r):
        F_rho, rho_r, rphi_r = (np.asarray(a, np.float64) for a in (F_rho, rho_r, rphi_r))
        self.rc, self.nelem = float(rc), F_rho.shape[0]
        self.F = [Spline(drho, F_rho[i]) for i in range(self.nelem)]
        self.rho = [Spline(dr, rho_r[i]) for i in range(self.nelem)]
        self.rphi = [[Spline(dr, rphi_r[i, j]) for j in range(self.nelem)] for i in range(self.nelem)]

    def _by_type(self, types, splines, method, x):
        """splines[t].method(x) for every atom's t; 0.0 where t is no type of the potential"""
        out = np.zeros(len(x)) if method != "evaluate_and_derivative" else (np.zeros(len(x)), np.zeros(len(x)))
        for t in range(self.nelem):
            pick = types == t
            if pick.any():
                got = getattr(splines[t], method)(x[pick])
                if isinstance(out, tuple):
                    out[0][pick], out[1][pick] = got
                else:
                    out[pick] = got
        return out

    def calculate(self, x, y, z, type_list, box, origin, boundary, verlet_list, distance_list, neighbor_number, force, virial, energy,
                  num_t=1, accumulate=True, n_real=None, virial_sum=None):
        calls["calculate"] += 1
        v = np.asarray(_np(verlet_list), np.int64)
        N, M = v.shape
        dist = np.asarray(_np(distance_list), np.float64)
        nn = np.clip(np.asarray(_np(neighbor_number), np.int64), 0, M)
        pos = [np.asarray(_np(a), np.float64) for a in (x, y, z)]
        t = np.asarray(_np(type_list), np.int64)
        known = (t >= 0) & (t < self.nelem)
        pbc = _pbc(box, boundary)
        me = np.arange(N)

        def row_walk():
            """(slot, live rows, j) for every slot that still has a live row, in list order"""
            alive = known.copy()
            for jj in range(M):
                alive = alive & (jj < nn) & (v[:, jj] >= 0) & (v[:, jj] < N)
                if not alive.any():
                    return
                yield jj, alive, np.where(alive, v[:, jj], me)

        # pass 1 (:85-113)
        rho = np.zeros(N)
        for jj, alive, j in row_walk():
            r = dist[:, jj]
            use = alive & (r <= self.rc) & known[j]
            term = self._by_type(np.where(use, t[j], -1), self.rho, "evaluate", r)
            rho = np.where(use, rho + term, rho)
        F, dF = self._by_type(np.where(known, t, -1), self.F, "evaluate_and_derivative", rho)
        self.density = rho  # (kept for the tests that ask where in its table an atom's embedding function was read)
        # pass 2 (:115-182)
        e = np.zeros(N)
        f = [np.zeros(N) for _ in range(3)]
        w = [np.zeros(N) for _ in range(9)]
        for jj, alive, j in row_walk():
            r = dist[:, jj]
            use = alive & (r <= self.rc) & known[j]
            if not use.any():
                continue
            d = pbc(pos[0][j] - pos[0][me], pos[1][j] - pos[1][me], pos[2][j] - pos[2][me])
            tj = np.where(use, t[j], -1)
            z2, dz2 = np.zeros(N), np.zeros(N)
            for a in range(self.nelem):
                for b in range(self.nelem):
                    pick = use & (t == a) & (tj == b)
                    if pick.any():
                        z2[pick], dz2[pick] = self.rphi[a][b].evaluate_and_derivative(r[pick])
            with np.errstate(divide="ignore", invalid="ignore", over="ignore"):
                rinv = 1.0 / r
                phi = z2 * rinv
                dphi = (dz2 - phi) * rinv
                drho_j = self._by_type(tj, self.rho, "derivative", r)
                drho_i = self._by_type(np.where(use, t, -1), self.rho, "derivative", r)
                e = np.where(use, e + 0.5 * phi, e)
                pf = dphi + dF * drho_j + dF[j] * drho_i
                pf = pf * rinv
                fp = [pf * d[k] for k in range(3)]
                for k in range(3):
                    f[k] = np.where(use, f[k] + fp[k], f[k])
                for a in range(3):
                    for b in range(3):
                        w[3 * a + b] = np.where(use, w[3 * a + b] - d[a] * fp[b], w[3 * a + b])
        if not accumulate:
            energy[...] = 0.0
            force[...] = 0.0
            virial[...] = 0.0
        E0 = np.array(_np(energy), np.float64)
        F0 = np.array(_np(force), np.float64)
        V0 = np.array(_np(virial), np.float64)
        energy[...] = np.where(known, (E0 + F) + e, E0)
        for k in range(3):
            force[:, k] = np.where(known, F0[:, k] + f[k], F0[:, k])
        for k in range(9):
            virial[:, k] = np.where(known, V0[:, k] + w[k] * 0.5, V0[:, k])
        if virial_sum is not None:
            virial_sum[...] = exact_column_sums(np.asarray(_np(virial))[: N if n_real is None else int(n_real)])


def exact_column_sums(virial):
    """the correctly rounded sum of every column (math.fsum)"""
    virial = np.asarray(virial, np.float64)
    return np.array([math.fsum(virial[:, k].tolist()) for k in range(virial.shape[1])])


def stress_of(virial_sums, volume):
    """the reference's stress from the nine virial sums (src/mdapy/eam.py:487-494)"""
    v = np.asarray(virial_sums, np.float64).reshape(3, 3)
    return (-0.5 * (v + v.T) / volume).ravel()[[0, 4, 8, 5, 2, 1]]


def types_of(frame, elements_list):
    names = np.asarray(frame["element"].to_numpy()).astype(str)
    return np.array([list(elements_list).index(n) for n in names], np.int32)


def on_system_list(system, eam, detail=None):
    """what ``system.get_*`` must return with ``system.calc = eam``: this restatement run on the list the System holds —
    ``as_numpy`` of its rows, distances and counts, positions, box and types in the compute view's numbering (the replica's for a
    thin box) — cut to the N real atoms.  -> (energies, forces, virials); ``detail`` (a dict) also receives the atoms' densities"""
    from mdapy_amd.devarray import as_numpy

    cell, frame = system._get_compute_view()
    n = frame.shape[0]
    ref = EAM(eam.rc, eam.dr, eam.drho, eam.F_rho, eam.rho_r, eam._rphi_r)
    energy, force, virial = np.zeros(n), np.zeros((n, 3)), np.zeros((n, 9))
    ref.calculate(*(frame[c].to_numpy() for c in "xyz"), types_of(frame, eam.elements_list), cell.box, cell.origin, cell.boundary,
                  as_numpy(system.verlet_list), as_numpy(system.distance_list), as_numpy(system.neighbor_number), force, virial, energy)
    calls["calculate"] -= 1  # (the yardstick's own run is not one of the package's calculations)
    if detail is not None:
        detail["density"] = ref.density[: system.N]
    return energy[: system.N], force[: system.N], virial[: system.N]


def hea(n, elements, ratios, noise, a=3.6):
    """the input configurations of the fixture, regenerated (numpy's legacy generator is stable): an n x n x n fcc lattice whose
    sites carry ``elements`` in the given ratios, shuffled with seed 1; ``noise``: uniform displacements of +-0.7 A, seed 1 again.
    -> (pos, box, element names)"""
    from mdapy_amd.build_lattice import lattice_positions

    pos, box = lattice_positions("fcc", a, n, n, n)
    N = len(pos)
    ratios = np.asarray(ratios, float)
    counts = np.floor(N * ratios).astype(int)
    counts[(counts == 0) & (ratios > 1e-6)] += 1
    counts[-1] = N - counts[:-1].sum()
    names = np.repeat(np.array(elements, dtype=object), counts)
    np.random.seed(1)
    np.random.shuffle(names)
    if noise:
        np.random.seed(1)
        pos = pos + (np.random.random((N, 3)) - 0.5) * 1.4
    return pos, box, names


def fixture_case(k):
    """-> (path of the potential file, pos, box, element names) of LAMMPS case k"""
    name, n, elements, ratios, noise = CASES[k]
    return (os.path.join(GOLDEN, name),) + hea(n, elements, ratios, noise)
