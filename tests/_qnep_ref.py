"""A numpy restatement of the charge-aware NEP arithmetic of mdapy_amd/csrc/nep_charge.hip for the QNEP tests, written from the
definition; the charge-free parts (radial functions, harmonics, invariants, ZBL) are those of tests/_nep_ref.py.  ``calculate_charge``
has the shape of ``mdapy_amd._nep.calculate_charge`` and ``Model`` that of its ``Model``, so the module can stand in for
``kernels.nep``.

The model.  The network of atom i has two outputs, the energy U_i and the charge q_i = sum_n w1q[n] tanh(w0[n] . x - b0[n]); the mean
of the real atoms' charges is removed.  With alpha = pi / rc (rc the largest radial cutoff), K = 14.399645 eV A and
tap = 2 alpha / sqrt(pi) the energy gains
    k-space (modes 1, 2): K sum_k G_k |S(k)|^2,  S(k) = sum_i q_i e^{-i k.r_i},  G_k = 2 (2 pi / V) / k^2 exp(-k^2 / (4 alpha^2)),
                          k over the half space of reciprocal vectors with 0 < k^2 < (2 pi alpha)^2
    real space (mode 1):  K (1/2 sum_ij q_i q_j erfc(alpha d) / d - tap / 2 sum_i q_i^2)      over list entries with d < rc
    real space (mode 3):  K 1/2 sum_ij q_i q_j (erfc(alpha d) / d + A d + B)                  (zero with its slope at d = rc)
D_i is the derivative of that energy with respect to q_i at fixed positions; the model's forces are those of the charge-free pair
pass with Fp_E + D_i Fp_q and A_E + D_i A_q in place of Fp and A (the removal of the mean is not differentiated: the format's
convention).  The same pair pass with (Fp_q, A_q) alone gives g_ij = dq_i / dr_ij, and the Born effective charge is
    bec_i = sqrt(eps_inf) (q_i 1 + 1/2 sum_j r_ij (x) (g_ij + g_ji))."""
import math
import os

import numpy as np
from scipy.special import erfc as _erfc

import _nep_ref
from _bond_ref import _pbc
from _nep_ref import COULOMB, _np, exact_column_sums, harmonics, invariants, radial_functions, zbl_pair

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "qnep")
calls = {"calculate": 0}


class Model(_nep_ref.Model):
    """header words (the last one the charge mode), the three ZBL numbers and the f64 block of ``QNEP._model_arrays``"""

    def unpack(self):
        T, NR, KR, NA, KA, L3, L4, L5, H, mode, size, charge = (int(v) for v in self.head[:12])
        dim = NR + NA * (L3 + (L4 == 2) + (L5 == 1))
        b, at = self.block, [0]

        def take(*shape):
            n = int(np.prod(shape))
            out = b[at[0]:at[0] + n].reshape(shape)
            at[0] += n
            return out

        m = dict(T=T, NR=NR, KR=KR, NA=NA, KA=KA, L3=L3, L4=L4, L5=L5, H=H, mode=mode, dim=dim, charge=charge)
        m["rc_r"], m["rc_a"], m["z"], m["rcov"], m["scaler"] = take(T), take(T), take(T), take(T), take(dim)
        m["c_r"], m["c_a"] = take(T, T, NR, KR), take(T, T, NA, KA)
        m["w0"], m["b0"], m["w1"], m["w1q"], m["bias"] = [], [], [], [], []
        for _ in range(T):
            m["w0"].append(take(H, dim)); m["b0"].append(take(H)); m["w1"].append(take(H)); m["w1q"].append(take(H)); m["bias"].append(take(1)[0])
        m["sqrt_eps"], m["b1"] = take(1)[0], take(1)[0]
        assert at[0] == size == len(b) and charge in (1, 2, 3), "the block's length does not belong to its header"
        return m


# ---------------------------------------------------------------------------------------------- the electrostatic part
def constants(rc):
    alpha = math.pi / rc
    tap = 2.0 * alpha / math.sqrt(math.pi)
    A = math.erfc(math.pi) / (rc * rc) + tap * math.exp(-math.pi * math.pi) / rc
    B = -math.erfc(math.pi) / rc - A * rc
    return alpha, tap, A, B


def k_points(cell, alpha):
    """cell (3, 3), rows the cell vectors -> (k (nk, 3), G (nk,)): n1 b1 + n2 b2 + n3 b3 with 0 < k^2 < (2 pi alpha)^2 in the half
    space n1 > 0, or n1 = 0 and n2 > 0, or n1 = n2 = 0 and n3 > 0; |n_i| <= alpha |a_i|"""
    cell = np.asarray(cell, np.float64)
    volume = abs(np.linalg.det(cell))
    b = 2.0 * math.pi * np.linalg.inv(cell).T  # rows b_i: a_i . b_j = 2 pi delta_ij
    top = [int(alpha * np.linalg.norm(cell[i])) for i in range(3)]
    n1, n2, n3 = np.meshgrid(np.arange(0, top[0] + 1), np.arange(-top[1], top[1] + 1), np.arange(-top[2], top[2] + 1), indexing="ij")
    n = np.stack([n1.ravel(), n2.ravel(), n3.ravel()], 1)
    half = (n[:, 0] > 0) | ((n[:, 0] == 0) & (n[:, 1] > 0)) | ((n[:, 0] == 0) & (n[:, 1] == 0) & (n[:, 2] > 0))
    n = n[half]
    k = n[:, 0:1] * b[0] + n[:, 1:2] * b[1] + n[:, 2:3] * b[2]
    ksq = (k * k).sum(1)
    keep = ksq < (2.0 * math.pi * alpha) ** 2
    k, ksq = k[keep], ksq[keep]
    return k, 2.0 * (2.0 * math.pi / volume) / ksq * np.exp(-ksq / (4.0 * alpha * alpha))


def coulomb(pos, q, n_real, cell, rc, mode, slots):
    """the electrostatic part for given charges.  pos (N, 3), q (N,); the structure factor sums the first n_real rows over ``cell``;
    ``slots`` yields (use (N,) bool, j (N,), d (N,), r_ij (N, 3)) list column by list column.
    -> per-atom energy (N,), D (N,), force (N, 3), virial (N, 9)"""
    N = len(q)
    alpha, tap, A, B = constants(rc)
    E, D, F, V = np.zeros(N), np.zeros(N), np.zeros((N, 3)), np.zeros((N, 9))
    if mode in (1, 2):
        k, G = k_points(cell, alpha)
        phase = pos[:n_real] @ k.T
        S = (q[:n_real, None] * np.exp(-1j * phase)).sum(0)
        for lo in range(0, N, 256):  # (blocks of atoms: the (atoms x k-points) table stays small)
            hi = min(N, lo + 256)
            w = S[None, :] * np.exp(1j * (pos[lo:hi] @ k.T))
            gse, gim = G * w.real, G * w.imag
            E[lo:hi] = COULOMB * q[lo:hi] * gse.sum(1)
            D[lo:hi] = 2.0 * COULOMB * gse.sum(1)
            F[lo:hi] = (2.0 * COULOMB * q[lo:hi])[:, None] * (gim @ k)
            factor = 2.0 / (4.0 * alpha * alpha) + 2.0 / (k * k).sum(1)
            kk = (k[:, :, None] * k[:, None, :]).reshape(-1, 9) * factor[:, None]
            V[lo:hi] = (COULOMB * q[lo:hi])[:, None] * (gse.sum(1)[:, None] * np.eye(3).ravel() - gse @ kk)
    if mode in (1, 3):
        if mode == 1:
            E += -COULOMB * tap * 0.5 * q * q
            D += -COULOMB * tap * q
        for use, j, d, delta in slots:
            use = use & (d < rc)
            d = np.where(use, d, 1.0)
            qq = q * q[j]
            screened = _erfc(alpha * d) / d
            phi = screened + (A * d + B if mode == 3 else 0.0)
            slope = (screened + tap * np.exp(-alpha * alpha * d * d)) / (d * d) - (A / d if mode == 3 else 0.0)
            f2 = -0.5 * COULOMB * qq * slope
            E += np.where(use, 0.5 * COULOMB * qq * phi, 0.0)
            D += np.where(use, COULOMB * q[j] * phi, 0.0)
            F += np.where(use[:, None], 2.0 * f2[:, None] * delta, 0.0)
            V -= np.where(use[:, None], (delta[:, :, None] * (f2[:, None] * delta)[:, None, :]).reshape(N, 9), 0.0)
    return E, D, F, V


def electrostatics(pos, q, cell, rc, mode):
    """``coulomb`` for a periodic cell of its own (3, 3): every image within rc by brute force, no list needed"""
    pos, q, cell = np.asarray(pos, np.float64), np.asarray(q, np.float64), np.asarray(cell, np.float64)
    N = len(q)
    reach = [int(math.ceil(rc * np.linalg.norm(np.linalg.inv(cell)[:, i]))) for i in range(3)]
    slots = []
    me = np.arange(N)
    for a in range(-reach[0], reach[0] + 1):
        for b in range(-reach[1], reach[1] + 1):
            for c in range(-reach[2], reach[2] + 1):
                shift = a * cell[0] + b * cell[1] + c * cell[2]
                for step in range(N):  # j = i + step: every pair of atoms once per image
                    if step == 0 and (a, b, c) == (0, 0, 0):
                        continue
                    j = (me + step) % N
                    delta = pos[j] + shift - pos
                    d = np.linalg.norm(delta, axis=1)
                    if (d < rc).any():
                        slots.append((d < rc, j, d, delta))
    return coulomb(pos, q, N, cell, rc, mode, slots)


# ---------------------------------------------------------------------------------------------- the whole calculation
def calculate_charge(x, y, z, types, type_map, box, origin, boundary, rows, dist, counts, model, kcell, rc_coulomb, energy=None, force=None,
                     virial=None, virial_sum=None, charge=None, bec=None, descriptor=None, latent=None, n_real=None, max_kpoints=None,
                     detail=None, charge_mean=None):
    """``charge_mean``: subtract this number instead of the mean of the real atoms' charges (the energy whose gradient the format's
    forces are: see ``on_system_list``); ``detail``: a dict that receives the electrostatic part and the mean that was removed"""
    calls["calculate"] += 1
    m = model.unpack()
    v = np.asarray(_np(rows), np.int64)
    N, M = v.shape
    real = N if n_real is None else int(n_real)
    d_all = np.asarray(_np(dist), np.float64)
    nn = np.clip(np.asarray(_np(counts), np.int64), 0, M)
    pos = np.stack([np.asarray(_np(a), np.float64) for a in (x, y, z)], 1)
    lookup = np.asarray(_np(type_map), np.int64)
    raw = np.asarray(_np(types), np.int64)
    t = np.where((raw >= 0) & (raw < len(lookup)), lookup[np.clip(raw, 0, len(lookup) - 1)], -1)
    known = t >= 0
    ts = np.where(known, t, 0)
    pbc = _pbc(box, boundary)
    me = np.arange(N)
    NR, NA, dim, H = m["NR"], m["NA"], m["dim"], m["H"]

    def walk():
        for slot in range(int(nn.max()) if N else 0):
            alive = known & (slot < nn) & (v[:, slot] >= 0) & (v[:, slot] < N)
            j = np.where(alive, v[:, slot], me)
            use = alive & known[j]
            d = np.where(use, d_all[:, slot], 1.0)
            delta = pos[j] - pos
            delta = np.stack(pbc(delta[:, 0], delta[:, 1], delta[:, 2]), 1)
            yield slot, use, j, d, delta

    # pass A: the descriptor and the network's two outputs
    q_r, s, e_zbl = np.zeros((N, NR)), np.zeros((N, NA, 24)), np.zeros(N)
    for slot, use, j, d, delta in walk():
        tj = ts[j]
        rc_r, rc_a = 0.5 * (m["rc_r"][ts] + m["rc_r"][tj]), 0.5 * (m["rc_a"][ts] + m["rc_a"][tj])
        g, _ = radial_functions(d, rc_r, m["c_r"][ts, tj])
        q_r += np.where((use & (d < rc_r))[:, None], g, 0.0)
        ang = use & (d < rc_a)
        g, _ = radial_functions(d, rc_a, m["c_a"][ts, tj])
        b = harmonics(delta / d[:, None])
        s += np.where(ang[:, None, None], g[:, :, None] * b[:, None, :], 0.0)
        if m["mode"]:
            e, _ = zbl_pair(d, m["z"][ts], m["z"][tj], m["rcov"][ts], m["rcov"][tj], m["mode"], *model.zbl)
            e_zbl += np.where(ang, 0.5 * e, 0.0)
    q_a, derivative = invariants(s, m)
    q = np.concatenate([q_r, q_a.reshape(N, -1)], 1) * m["scaler"]
    E, Q, Fp, Fq, lat = np.zeros(N), np.zeros(N), np.zeros((N, dim)), np.zeros((N, dim)), np.zeros((N, H))
    for k in range(m["T"]):
        pick = known & (ts == k)
        if not pick.any():
            continue
        hidden = np.tanh(q[pick] @ m["w0"][k].T - m["b0"][k])
        lat[pick] = hidden * m["w1"][k]
        E[pick] = lat[pick].sum(1) - m["b1"] - m["bias"][k]
        Q[pick] = (hidden * m["w1q"][k]).sum(1)
        Fp[pick] = ((1.0 - hidden * hidden) * m["w1"][k]) @ m["w0"][k]
        Fq[pick] = ((1.0 - hidden * hidden) * m["w1q"][k]) @ m["w0"][k]
    Fp, Fq = Fp * m["scaler"], Fq * m["scaler"]
    A_E, A_q = derivative(Fp[:, NR:].reshape(N, -1, NA)), derivative(Fq[:, NR:].reshape(N, -1, NA))
    E = np.where(known, E + e_zbl, 0.0)
    Q = np.where(known, Q, 0.0)
    removed = (Q[:real].sum() / real if real else 0.0) if charge_mean is None else float(charge_mean)
    Q = Q - removed
    if descriptor is not None:
        descriptor[...] = np.where(known[:, None], q, 0.0)
    if latent is not None:
        latent[...] = np.where(known[:, None], lat, 0.0)
    # the electrostatic part
    e_c, D, f_c, v_c = coulomb(pos, Q, real, np.asarray(kcell, np.float64), float(rc_coulomb), m["charge"],
                               ((use, j, d, delta) for _, use, j, d, delta in walk()))
    if detail is not None:
        detail.update(coulomb_energy=e_c, D=D, coulomb_force=f_c, coulomb_virial=v_c, charge_mean=removed)
    if energy is not None:
        energy[...] = E + e_c
    if charge is not None:
        charge[...] = Q

    def pair_table(FpR, A, with_zbl):
        table = np.zeros((N, M, 3))
        for slot, use, j, d, delta in walk():
            tj = ts[j]
            u = delta / d[:, None]
            rc_r, rc_a = 0.5 * (m["rc_r"][ts] + m["rc_r"][tj]), 0.5 * (m["rc_a"][ts] + m["rc_a"][tj])
            _, dg = radial_functions(d, rc_r, m["c_r"][ts, tj])
            f = np.where((use & (d < rc_r))[:, None], np.einsum("an,an->a", FpR, dg)[:, None] * u, 0.0)
            g, dg = radial_functions(d, rc_a, m["c_a"][ts, tj])
            b, grad = harmonics(u, True)
            S = np.einsum("ank,ak->an", A, b)
            V = np.einsum("ank,akc->anc", A, grad)
            V = V - u[:, None, :] * np.einsum("anc,ac->an", V, u)[:, :, None]
            fa = np.einsum("an,an->a", dg, S)[:, None] * u + np.einsum("an,anc->ac", g, V) / d[:, None]
            if with_zbl:
                _, de = zbl_pair(d, m["z"][ts], m["z"][tj], m["rcov"][ts], m["rcov"][tj], m["mode"], *model.zbl)
                fa = fa + (0.5 * de)[:, None] * u
            table[:, slot] = f + np.where((use & (d < rc_a))[:, None], fa, 0.0)
        return table

    def back_of(table, slot, use, j):
        """f_ji: where row j names i"""
        back = (v[j] == me[:, None]) & (np.arange(M)[None, :] < nn[j][:, None])
        found = use & back.any(1)
        return np.where(found[:, None], table[j, back.argmax(1)], 0.0)

    if not (force is None and virial is None and virial_sum is None):
        table = pair_table(Fp[:, :NR] + D[:, None] * Fq[:, :NR], A_E + D[:, None, None] * A_q, bool(m["mode"]))
        F, Vir = np.zeros((N, 3)), np.zeros((N, 9))
        for slot, use, j, d, delta in walk():
            f_ji = back_of(table, slot, use, j)
            F += np.where(use[:, None], table[:, slot] - f_ji, 0.0)
            Vir += np.where(use[:, None], (delta[:, :, None] * f_ji[:, None, :]).reshape(N, 9), 0.0)
        F, Vir = F + f_c, Vir + v_c
        if force is not None:
            force[...] = F
        if virial is not None:
            virial[...] = Vir
        if virial_sum is not None:
            virial_sum[...] = exact_column_sums(Vir[:real])
    if bec is not None:
        table = pair_table(Fq[:, :NR], A_q, False)
        Z = Q[:, None] * np.eye(3).ravel()[None, :]
        for slot, use, j, d, delta in walk():
            both = table[:, slot] + back_of(table, slot, use, j)
            Z += np.where(use[:, None], 0.5 * (delta[:, :, None] * both[:, None, :]).reshape(N, 9), 0.0)
        bec[...] = Z * m["sqrt_eps"]


def on_system_list(system, qnep, want=("energy", "force", "virial", "charge", "bec"), detail=None, charge_mean=None):
    """what ``system.get_*`` must return with ``system.calc = qnep``: this restatement on the list the System holds, in the compute
    view's numbering, cut to the N real atoms.

    ``charge_mean``.  The format's forces carry D_i dq_i/dr of every atom's own network output and nothing for the mean that is
    removed from the charges: they are the gradient of the energy in which the removed number is a CONSTANT, not of the energy in
    which it follows the atoms.  A finite difference that is to meet them hands the unmoved frame's mean in here."""
    from mdapy_amd.devarray import as_numpy

    cell, frame = system._get_compute_view()
    n = frame.shape[0]
    names = np.asarray(frame["element"].to_numpy()).astype(str)
    types = np.array([qnep.element_list.index(e) for e in names], np.int32)
    present = tuple(int(k) for k in np.unique(types))
    type_map = np.full(len(qnep.element_list), -1, np.int32)
    type_map[list(present)] = np.arange(len(present))
    model = Model(*qnep._model_arrays(present))
    widths = dict(energy=(n,), force=(n, 3), virial=(n, 9), charge=(n,), bec=(n, 9))
    out = {name: np.zeros(widths[name]) for name in want}
    calculate_charge(*(frame[c].to_numpy() for c in "xyz"), types, type_map, cell.box, cell.origin, cell.boundary, as_numpy(system.verlet_list),
                     as_numpy(system.distance_list), as_numpy(system.neighbor_number), model, qnep._ewald_cell(system.box),
                     qnep.info["radial_cutoff"], n_real=system.N, detail=detail, charge_mean=charge_mean, **out)
    calls["calculate"] -= 1
    return {name: a[: system.N] for name, a in out.items()}


def gpumd_differences(calc, frames, want):
    """the reference's own comparison (its tests/test_qnep.py): the mean energy per atom, the forces, the mean virial in the order
    xx yy zz xy yz zx, the BEC, and the charges against the recorded ones with their per-frame mean removed.
    -> name -> the largest absolute difference over the frames"""
    import mdapy_amd as mp

    worst = dict(energy=0.0, force=0.0, virial=0.0, charge=0.0, bec=0.0)
    for k, s in enumerate(frames):
        s = mp.System(data=s.data, box=s.box)
        s.calc = calc
        calc.results = {}
        rows = slice(384 * k, 384 * (k + 1))
        recorded = want["charge"][rows] - want["charge"][rows].mean()
        got = dict(energy=s.get_energies().mean() - want["energy"][k], force=s.get_force() - want["force"][rows],
                   virial=s.get_virials().mean(axis=0)[[0, 4, 8, 1, 5, 6]] - want["virial"][k],
                   charge=calc.results["charges"] - recorded, bec=calc.results["bec"] - want["bec"][rows])
        assert s.N == 384 and calc.results["charges"].shape == (384,) and calc.results["bec"].shape == (384, 9)
        for name in worst:
            worst[name] = max(worst[name], float(np.abs(got[name]).max()))
    return worst


def write_model(path, charge_mode=1, elements=("Al", "Cr", "Ni"), cutoffs=(5.0, 4.0), n_max=(3, 2), basis=(5, 4), l_max=(4, 2, 1), neurons=6,
                zbl=None, seed=0):
    """a small nep4 charge model from a seeded generator, in the manner of ``_nep_ref.write_model``: per type w0, b0, then w1 of
    2 x neurons (energy row, charge row); after all types sqrt(epsilon_inf) (1.3 here), then the common bias"""
    rng = np.random.default_rng(seed)
    T = len(elements)
    orders = l_max[0] + (l_max[1] == 2) + (l_max[2] == 1)
    dim = (n_max[0] + 1) + (n_max[1] + 1) * orders
    n_ann = neurons * (dim + 3) * T + 2
    n_c = T * T * ((n_max[0] + 1) * (basis[0] + 1) + (n_max[1] + 1) * (basis[1] + 1))
    numbers = rng.normal(0.0, 0.3, n_ann + n_c)
    numbers[n_ann - 2] = 1.3
    scalers = rng.uniform(0.5, 2.0, dim)
    flat = np.ravel(cutoffs)
    lines = [f"nep4{'_zbl' if zbl else ''}_charge{charge_mode} {T} " + " ".join(elements)]
    if zbl:
        lines.append("zbl " + " ".join(repr(float(v)) for v in zbl))
    lines += ["cutoff " + " ".join(repr(float(v)) for v in flat) + " 100 80", f"n_max {n_max[0]} {n_max[1]}", f"basis_size {basis[0]} {basis[1]}",
              f"l_max {l_max[0]} {l_max[1]} {l_max[2]}", f"ANN {neurons} 0"]
    lines += [f"{v:.17e}" for v in numbers] + [f"{v:.17e}" for v in scalers]
    with open(path, "wt") as f:
        f.write("\n".join(lines) + "\n")
    return dict(numbers=numbers, scalers=scalers, dim=dim, n_ann=n_ann, elements=list(elements), neurons=neurons, cutoffs=flat.reshape(-1, 2),
                n_max=n_max, basis=basis, l_max=l_max, zbl=zbl, charge_mode=charge_mode)


def argument_error_calls(L):
    """the raw C entry ``mdh_nep_charge`` with arguments it must refuse before any device work -> (what was wrong, its return code),
    one by one.  (Null array pointers: a call that got as far as touching one would not come back with an error code.)"""
    from mdapy_amd import _lib

    box, origin, pbc = np.eye(3) * 20.0, np.zeros(3), np.ones(3, np.int32)
    good = dict(T=2, NR=3, KR=4, NA=3, KA=4, L3=4, L4=2, L5=1, H=5, mode=0, charge=1)
    zbl = np.array([1.0, 2.0, 0.0])

    def call(N=4, M=2, n_real=4, type_map=(0, 1), types=None, length=None, virial_sum=False, kcell=np.eye(3) * 20.0, rc=5.0, max_k=1 << 20, **head):
        h = dict(good, **head)
        dim = h["NR"] + h["NA"] * (h["L3"] + (h["L4"] == 2) + (h["L5"] == 1))
        size = 4 * h["T"] + dim + h["T"] ** 2 * (h["NR"] * h["KR"] + h["NA"] * h["KA"]) + h["T"] * (h["H"] * (dim + 3) + 1) + 2
        words = np.array([h[k] for k in ("T", "NR", "KR", "NA", "KA", "L3", "L4", "L5", "H", "mode")] + [size if length is None else length, h["charge"]],
                         np.int32)
        tm = np.array(type_map, np.int32)
        ty = None if types is None else np.array(types, np.int32)
        nine = np.zeros(9)
        cell = None if kcell is None else np.ascontiguousarray(kcell, np.float64)
        return L.mdh_nep_charge(None, None, None, None if ty is None else ty.ctypes.data, N, tm.ctypes.data, len(tm), box.ctypes.data,
                                origin.ctypes.data, pbc.ctypes.data, None, None, None, M, None, words.ctypes.data, zbl.ctypes.data,
                                None if cell is None else cell.ctypes.data, rc, max_k, n_real, None, None, None,
                                nine.ctypes.data if virial_sum else None, None, None, None, None, _lib.HOST, None)

    charge_free = 4 * 2 + 27 + 4 * 24 + 2 * (5 * 29 + 1) + 1  # the block's length without the charge's weights and sqrt(epsilon_inf)
    # a 20 A cell with rc = 5 has 544 k-points in the half space; a cell of 10^5 A has more integer triples than the host walks; a
    # cell 8000 A long has 10 053 phase-table entries along that axis, more than LDS holds for one atom
    for bad in (dict(charge=0), dict(charge=4), dict(charge=-1), dict(length=charge_free), dict(length=7), dict(max_k=100), dict(max_k=-1),
                dict(kcell=np.eye(3) * 1e5), dict(kcell=np.diag([20.0, 20.0, 8000.0]), max_k=1 << 24), dict(kcell=np.zeros((3, 3))), dict(kcell=None), dict(rc=0.0), dict(rc=-1.0), dict(rc=float("nan")),
                dict(NA=17), dict(H=129), dict(T=0), dict(L3=5), dict(L4=1), dict(L3=1, L4=2), dict(mode=3), dict(mode=1, length=7),
                dict(type_map=(0, 2)), dict(types=(0, 1, 2, 0)), dict(M=1 << 23), dict(N=-1), dict(n_real=5), dict(virial_sum=True)):
        yield bad, call(**bad)
