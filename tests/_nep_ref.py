"""A numpy restatement of the NEP arithmetic of mdapy_amd/csrc/nep.hip for the NEP tests, written from the model's definition
(Fan et al., Phys. Rev. B 104, 104309; J. Chem. Phys. 157, 114801): ``calculate`` has the shape of ``mdapy_amd._nep.calculate`` and
``Model`` that of its ``Model``, so the module can stand in for ``kernels.nep``.  It walks the list slot by slot, vectorised over
the atoms, so every per-atom sum is accumulated in list order, as the kernels do.

Notation.  u = r_ij / d is the unit vector to a neighbour; the 24 real harmonics b_k(u), l = 1..4, are p_lm(z) Re (x + i y)^m and
p_lm(z) Im (x + i y)^m with p_lm proportional to the m-th derivative of the Legendre polynomial P_l (``P_LM``); s_nk = sum_j
g_n(d_j) b_k(u_j); the 3-body invariant is q_n^l = sum_k W_k s_nk^2, and W follows from the addition theorem (``weights``).
Forces: with A_nk = dE_i / ds_nk the derivative of E_i with respect to r_ij is
    f_ij = sum_n [ g_n'(d) (A_n . b) u + g_n(d) / d (1 - u u^T) (A_n . grad b) ]
(grad b the gradient of b as a polynomial in x, y, z), plus the radial part sum_n Fp_n g_n'(d) u and half the ZBL pair force.
The force on i is sum_j (f_ij - f_ji), its virial sum_j r_ij (x) f_ji."""
import gzip
import math
import os

import numpy as np

from _bond_ref import _pbc

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "nep")
UNEP = os.path.join(GOLDEN, "UNEP-v1.txt.gz")
calls = {"calculate": 0}
# the small models the tests write themselves (write_model): every branch of the format that UNEP-v1 (nep4_zbl, one pair of cutoffs,
# l_max 4 2 1, n_max 4 4) does not take; 'wide' has more than 8 radial functions, which the kernels give 16 lanes an atom
VARIANTS = {"nep3": dict(version=3),
            "nep5_zbl": dict(version=5, zbl=(1.0, 2.0), neurons=10),
            "typewise_cutoffs": dict(version=4, cutoffs=((5.0, 4.0), (4.5, 3.5), (4.8, 4.2)), neurons=4),
            "zbl_factor": dict(version=4, zbl=(1.0, 2.0, 0.7)),
            "l_max_200": dict(version=4, l_max=(2, 0, 0)),
            "wide": dict(version=4, elements=("Al", "Ni"), n_max=(9, 8), basis=(10, 9), neurons=5)}

# p_lm(z) as coefficient lists in rising powers of z, l = 1..4, m = 0..l
P_LM = {1: [[0, 1], [1]],
        2: [[-1, 0, 3], [0, 1], [1]],
        3: [[0, -3, 0, 5], [-1, 0, 5], [0, 1], [1]],
        4: [[3, 0, -30, 0, 35], [0, -3, 0, 7], [-1, 0, 7], [0, 1], [1]]}
# the 4-body (l = 2) and 5-body (l = 1) invariants' coefficients: tables of the NEP format (GPUMD, J. Chem. Phys. 157, 114801)
C4 = (-0.007499480826664, -0.134990654879954, 0.067495327439977, 0.404971964639861, -0.809943929279723)
C5 = (0.026596810706114, 0.053193621412227, 0.026596810706114)
ZBL_A = (0.18175, 0.50986, 0.28022, 0.02817)  # the universal screening function (Ziegler, Biersack, Littmark)
ZBL_B = (3.1998, 0.94229, 0.4029, 0.20162)
ZBL_LENGTH_INV, COULOMB = 2.134563, 14.399645  # 1 / 0.46850 A; e^2 / (4 pi eps0) in eV A


def weights():
    """W_k, k = 0..23.  Addition theorem: P_l(cos g) = sum_m (2 - d_m0) (l-m)!/(l+m)! P_l^m(z) P_l^m(z') cos m(phi - phi'), and
    P_l^m(z) cos m phi = (d^m P_l / dz^m) Re (x + i y)^m.  With p_lm = a_lm d^m P_l / dz^m:
    W_lm = (2l+1)/(4 pi) (2 - d_m0) (l-m)!/(l+m)! / a_lm^2, so that q^l = (2l+1)/(4 pi) sum_jk g_j g_k P_l(cos theta_jk)."""
    out = []
    for l in range(1, 5):
        legendre = np.polynomial.legendre.leg2poly([0] * l + [1])
        for m in range(l + 1):
            derived = np.polynomial.polynomial.polyder(legendre, m) if m else legendre
            a = P_LM[l][m][-1] / derived[-1]
            w = (2 * l + 1) / (4.0 * math.pi) * math.factorial(l - m) / math.factorial(l + m) / (a * a)
            out += [w] if m == 0 else [2.0 * w, 2.0 * w]
    return np.array(out)


W = weights()
L_OF_K = np.array([l for l in range(1, 5) for _ in range(2 * l + 1)])


def _np(a):
    if hasattr(a, "numpy") and not isinstance(a, np.ndarray):
        a = a.numpy()
    return np.asarray(a.to_numpy() if hasattr(a, "to_numpy") else a)


def harmonics(u, gradient=False):
    """u (..., 3) -> b (..., 24) [and grad b (..., 24, 3)]"""
    x, y, z = u[..., 0], u[..., 1], u[..., 2]
    c, s = [np.ones_like(x), x], [np.zeros_like(x), y]
    for m in range(2, 5):
        c.append(x * c[m - 1] - y * s[m - 1])
        s.append(x * s[m - 1] + y * c[m - 1])
    b, g = [], []
    for l in range(1, 5):
        for m in range(l + 1):
            p = np.polynomial.polynomial.polyval(z, P_LM[l][m])
            dp = np.polynomial.polynomial.polyval(z, np.polynomial.polynomial.polyder(P_LM[l][m])) if len(P_LM[l][m]) > 1 else 0.0 * z
            if m == 0:
                b.append(p)
                g.append(np.stack([0.0 * z, 0.0 * z, dp], -1))
            else:
                b += [p * c[m], p * s[m]]
                g.append(np.stack([p * m * c[m - 1], -p * m * s[m - 1], dp * c[m]], -1))
                g.append(np.stack([p * m * s[m - 1], p * m * c[m - 1], dp * s[m]], -1))
    b = np.stack(b, -1)
    return (b, np.stack(g, -2)) if gradient else b


def radial_functions(d, rc, c):
    """g_n(d) and g_n'(d) for coefficient rows c (..., n, k): f_k = (T_k(x) + 1) / 2 * fc, x = 2 (d / rc - 1)^2 - 1,
    fc = (1 + cos(pi d / rc)) / 2 below rc and 0 from there on"""
    inside = d < rc
    t = d / rc
    fc = np.where(inside, 0.5 * np.cos(math.pi * t) + 0.5, 0.0)
    dfc = np.where(inside, -0.5 * math.pi * np.sin(math.pi * t) / rc, 0.0)
    x = 2.0 * (t - 1.0) ** 2 - 1.0
    dx = 4.0 * (t - 1.0) / rc
    K = c.shape[-1]
    T, dT = [np.ones_like(x), x], [np.zeros_like(x), np.ones_like(x)]
    for k in range(2, K):
        T.append(2.0 * x * T[k - 1] - T[k - 2])
        dT.append(2.0 * T[k - 1] + 2.0 * x * dT[k - 1] - dT[k - 2])
    f = np.stack([(T[k] + 1.0) * 0.5 * fc for k in range(K)], -1)
    df = np.stack([0.5 * dT[k] * dx * fc + (T[k] + 1.0) * 0.5 * dfc for k in range(K)], -1)
    return np.einsum("...nk,...k->...n", c, f), np.einsum("...nk,...k->...n", c, df)


def zbl_pair(d, zi, zj, ri, rj, mode, inner, outer, factor):
    """the pair's ZBL energy and its derivative with respect to d"""
    a_inv = (zi ** 0.23 + zj ** 0.23) * ZBL_LENGTH_INV
    xs = d * a_inv
    phi = sum(a * np.exp(-b * xs) for a, b in zip(ZBL_A, ZBL_B))
    dphi = sum(-a * b * np.exp(-b * xs) for a, b in zip(ZBL_A, ZBL_B)) * a_inv
    k = COULOMB * zi * zj
    e, de = k * phi / d, k * (dphi / d - phi / (d * d))
    if mode == 2:
        lo, hi = np.zeros_like(d), np.minimum(factor * (ri + rj), outer)
    else:
        lo, hi = np.full_like(d, inner), np.full_like(d, outer)
    span = math.pi / np.where(hi > lo, hi - lo, 1.0)
    mid = (d >= lo) & (d < hi)
    fc = np.where(d < lo, 1.0, np.where(mid, 0.5 * np.cos(span * (d - lo)) + 0.5, 0.0))
    dfc = np.where(mid, -0.5 * span * np.sin(span * (d - lo)), 0.0)
    return e * fc, de * fc + e * dfc


class Model:
    """header words, the three ZBL numbers and the f64 block, as ``mdapy_amd._nep.Model`` takes them"""

    def __init__(self, head, zbl, block):
        self.head, self.zbl, self.block = np.asarray(head, np.int32), np.asarray(zbl, np.float64), np.asarray(block, np.float64)

    def unpack(self):
        T, NR, KR, NA, KA, L3, L4, L5, H, mode, size = (int(v) for v in self.head[:11])
        orders = L3 + (L4 == 2) + (L5 == 1)
        dim = NR + NA * orders
        b, at = self.block, [0]

        def take(*shape):
            n = int(np.prod(shape))
            out = b[at[0]:at[0] + n].reshape(shape)
            at[0] += n
            return out

        m = dict(T=T, NR=NR, KR=KR, NA=NA, KA=KA, L3=L3, L4=L4, L5=L5, H=H, mode=mode, dim=dim)
        m["rc_r"], m["rc_a"], m["z"], m["rcov"], m["scaler"] = take(T), take(T), take(T), take(T), take(dim)
        m["c_r"], m["c_a"] = take(T, T, NR, KR), take(T, T, NA, KA)
        m["w0"], m["b0"], m["w1"], m["bias"] = [], [], [], []
        for _ in range(T):
            m["w0"].append(take(H, dim)); m["b0"].append(take(H)); m["w1"].append(take(H)); m["bias"].append(take(1)[0])
        m["b1"] = take(1)[0]
        assert at[0] == size == len(b), "the block's length does not belong to its header"
        return m


def invariants(s, m):
    """s (N, NA, 24) -> (q_angular (N, orders, NA), dq/ds contracted later: a function Fp_angular (N, orders, NA) -> A (N, NA, 24))"""
    L3 = m["L3"]
    q = [np.einsum("k,ank->an", W * (L_OF_K == l), s * s) for l in range(1, L3 + 1)]
    t = [s[..., 3 + k] for k in range(5)]
    p = [s[..., k] for k in range(3)]
    pp = p[1] ** 2 + p[2] ** 2
    if m["L4"] == 2:
        q.append(C4[0] * t[0] ** 3 + C4[1] * t[0] * (t[1] ** 2 + t[2] ** 2) + C4[2] * t[0] * (t[3] ** 2 + t[4] ** 2)
                 + C4[3] * t[3] * (t[2] ** 2 - t[1] ** 2) + C4[4] * t[1] * t[2] * t[4])
    if m["L5"] == 1:
        q.append(C5[0] * p[0] ** 4 + C5[1] * p[0] ** 2 * pp + C5[2] * pp * pp)

    def derivative(Fp):
        A = np.zeros_like(s)
        for l in range(1, L3 + 1):
            A += 2.0 * (W * (L_OF_K == l)) * s * Fp[:, l - 1, :, None]
        at = L3
        if m["L4"] == 2:
            F = Fp[:, at]
            A[..., 3] += F * (3.0 * C4[0] * t[0] ** 2 + C4[1] * (t[1] ** 2 + t[2] ** 2) + C4[2] * (t[3] ** 2 + t[4] ** 2))
            A[..., 4] += F * (2.0 * C4[1] * t[0] * t[1] - 2.0 * C4[3] * t[3] * t[1] + C4[4] * t[2] * t[4])
            A[..., 5] += F * (2.0 * C4[1] * t[0] * t[2] + 2.0 * C4[3] * t[3] * t[2] + C4[4] * t[1] * t[4])
            A[..., 6] += F * (2.0 * C4[2] * t[0] * t[3] + C4[3] * (t[2] ** 2 - t[1] ** 2))
            A[..., 7] += F * (2.0 * C4[2] * t[0] * t[4] + C4[4] * t[1] * t[2])
            at += 1
        if m["L5"] == 1:
            F = Fp[:, at]
            A[..., 0] += F * (4.0 * C5[0] * p[0] ** 3 + 2.0 * C5[1] * p[0] * pp)
            A[..., 1] += F * (2.0 * C5[1] * p[0] ** 2 * p[1] + 4.0 * C5[2] * pp * p[1])
            A[..., 2] += F * (2.0 * C5[1] * p[0] ** 2 * p[2] + 4.0 * C5[2] * pp * p[2])
        return A

    return np.stack(q, 1), derivative


def calculate(x, y, z, types, type_map, box, origin, boundary, rows, dist, counts, model, energy=None, force=None, virial=None,
              virial_sum=None, descriptor=None, latent=None, n_real=None, rows_of_interest=None):
    calls["calculate"] += 1
    m = model.unpack()
    v = np.asarray(_np(rows), np.int64)
    N, M = v.shape
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

    def walk(R=N):
        """the rows 0 .. R-1, slot by slot: (slot, which rows use it, j, d, r_ij)"""
        for slot in range(int(nn[:R].max()) if R else 0):
            alive = known[:R] & (slot < nn[:R]) & (v[:R, slot] >= 0) & (v[:R, slot] < N)
            j = np.where(alive, v[:R, slot], me[:R])
            use = alive & known[j]
            d = np.where(use, d_all[:R, slot], 1.0)
            delta = pos[j] - pos[:R]
            delta = np.stack(pbc(delta[:, 0], delta[:, 1], delta[:, 2]), 1)
            yield slot, use, j, d, delta

    # pass A: the descriptor and the network
    pairs = not (force is None and virial is None and virial_sum is None)
    R = N if pairs or rows_of_interest is None else int(rows_of_interest)  # (energies alone: only these rows are worked out)
    known_r, ts_r = known[:R], ts[:R]
    q_r, s, e_zbl = np.zeros((R, NR)), np.zeros((R, NA, 24)), np.zeros(R)
    for slot, use, j, d, delta in walk(R):
        tj = ts[j]
        rc_r, rc_a = 0.5 * (m["rc_r"][ts_r] + m["rc_r"][tj]), 0.5 * (m["rc_a"][ts_r] + m["rc_a"][tj])
        g, _ = radial_functions(d, rc_r, m["c_r"][ts_r, tj])
        q_r += np.where((use & (d < rc_r))[:, None], g, 0.0)
        ang = use & (d < rc_a)
        g, _ = radial_functions(d, rc_a, m["c_a"][ts_r, tj])
        b = harmonics(delta / d[:, None])
        s += np.where(ang[:, None, None], g[:, :, None] * b[:, None, :], 0.0)
        if m["mode"]:
            e, _ = zbl_pair(d, m["z"][ts_r], m["z"][tj], m["rcov"][ts_r], m["rcov"][tj], m["mode"], *model.zbl)
            e_zbl += np.where(ang, 0.5 * e, 0.0)
    q_a, derivative = invariants(s, m)
    q = np.concatenate([q_r, q_a.reshape(R, -1)], 1) * m["scaler"]
    E, Fp, lat = np.zeros(R), np.zeros((R, dim)), np.zeros((R, H))
    for k in range(m["T"]):
        pick = known_r & (ts_r == k)
        if not pick.any():
            continue
        hidden = np.tanh(q[pick] @ m["w0"][k].T - m["b0"][k])
        lat[pick] = hidden * m["w1"][k]
        E[pick] = lat[pick].sum(1) - m["b1"] - m["bias"][k]
        Fp[pick] = ((1.0 - hidden * hidden) * m["w1"][k]) @ m["w0"][k]
    Fp = Fp * m["scaler"]
    A = derivative(Fp[:, NR:].reshape(R, -1, NA))
    E = np.where(known_r, E + e_zbl, 0.0)
    if descriptor is not None:
        descriptor[:R] = np.where(known_r[:, None], q, 0.0)
    if latent is not None:
        latent[:R] = np.where(known_r[:, None], lat, 0.0)
    if energy is not None:
        energy[:R] = E
    if not pairs:
        return
    # pass B: every pair's f_ij, then the gather
    table = np.zeros((N, M, 3))
    for slot, use, j, d, delta in walk():
        tj = ts[j]
        u = delta / d[:, None]
        rc_r, rc_a = 0.5 * (m["rc_r"][ts] + m["rc_r"][tj]), 0.5 * (m["rc_a"][ts] + m["rc_a"][tj])
        _, dg = radial_functions(d, rc_r, m["c_r"][ts, tj])
        f = np.where((use & (d < rc_r))[:, None], np.einsum("an,an->a", Fp[:, :NR], dg)[:, None] * u, 0.0)
        g, dg = radial_functions(d, rc_a, m["c_a"][ts, tj])
        b, grad = harmonics(u, True)
        S = np.einsum("ank,ak->an", A, b)
        V = np.einsum("ank,akc->anc", A, grad)
        V = V - u[:, None, :] * np.einsum("anc,ac->an", V, u)[:, :, None]
        fa = np.einsum("an,an->a", dg, S)[:, None] * u + np.einsum("an,anc->ac", g, V) / d[:, None]
        if m["mode"]:
            _, de = zbl_pair(d, m["z"][ts], m["z"][tj], m["rcov"][ts], m["rcov"][tj], m["mode"], *model.zbl)
            fa = fa + (0.5 * de)[:, None] * u
        f = f + np.where((use & (d < rc_a))[:, None], fa, 0.0)
        table[:, slot] = f
    F, Vir = np.zeros((N, 3)), np.zeros((N, 9))
    for slot, use, j, d, delta in walk():
        back = (v[j] == me[:, None]) & (np.arange(M)[None, :] < nn[j][:, None])
        found = use & back.any(1)
        f_ji = np.where(found[:, None], table[j, back.argmax(1)], 0.0)
        F += np.where(use[:, None], table[:, slot] - f_ji, 0.0)
        Vir += np.where(use[:, None], (delta[:, :, None] * f_ji[:, None, :]).reshape(N, 9), 0.0)
    if force is not None:
        force[...] = F
    if virial is not None:
        virial[...] = Vir
    if virial_sum is not None:
        virial_sum[...] = exact_column_sums(Vir[: N if n_real is None else int(n_real)])


def exact_column_sums(virial):
    virial = np.asarray(virial, np.float64)
    return np.array([math.fsum(virial[:, k].tolist()) for k in range(virial.shape[1])])


def on_system_list(system, nep, want=("energy", "force", "virial")):
    """what ``system.get_*`` must return with ``system.calc = nep``: this restatement on the list the System holds, in the compute
    view's numbering, cut to the N real atoms.  -> dict of the arrays named in ``want`` (also 'descriptor', 'latent')"""
    from mdapy_amd.devarray import as_numpy

    cell, frame = system._get_compute_view()
    n = frame.shape[0]
    names = np.asarray(frame["element"].to_numpy()).astype(str)
    types = np.array([nep.element_list.index(e) for e in names], np.int32)
    present = tuple(int(k) for k in np.unique(types))
    type_map = np.full(len(nep.element_list), -1, np.int32)
    type_map[list(present)] = np.arange(len(present))
    model = Model(*nep._model_arrays(present))
    widths = dict(energy=(n,), force=(n, 3), virial=(n, 9), descriptor=(n, nep.info["num_ndim"]), latent=(n, nep.info["num_nlatent"]))
    out = {name: np.zeros(widths[name]) for name in want}
    calculate(*(frame[c].to_numpy() for c in "xyz"), types, type_map, cell.box, cell.origin, cell.boundary, as_numpy(system.verlet_list),
              as_numpy(system.distance_list), as_numpy(system.neighbor_number), model, rows_of_interest=system.N, **out)
    calls["calculate"] -= 1
    return {name: a[: system.N] for name, a in out.items()}


def write_model(path, version=4, elements=("Al", "Cr", "Ni"), cutoffs=(5.0, 4.0), n_max=(3, 2), basis=(5, 4), l_max=(4, 2, 1), neurons=6,
                zbl=None, seed=0):
    """a small model from a seeded generator: weights of order 0.3, scalers of order 1.  cutoffs: one pair, or one pair per element;
    zbl: None, (inner, outer) or (inner, outer, factor).  -> the dict of what was written"""
    rng = np.random.default_rng(seed)
    T = len(elements)
    orders = l_max[0] + (l_max[1] == 2) + (l_max[2] == 1)
    dim = (n_max[0] + 1) + (n_max[1] + 1) * orders
    per_net = neurons * (dim + 2) + (version == 5)
    n_ann = per_net * (1 if version == 3 else T) + 1
    n_c = T * T * ((n_max[0] + 1) * (basis[0] + 1) + (n_max[1] + 1) * (basis[1] + 1))
    numbers = rng.normal(0.0, 0.3, n_ann + n_c)
    scalers = rng.uniform(0.5, 2.0, dim)
    flat = np.ravel(cutoffs)
    lines = [f"nep{version}{'_zbl' if zbl else ''} {T} " + " ".join(elements)]
    if zbl:
        lines.append("zbl " + " ".join(repr(float(v)) for v in zbl))
    lines += ["cutoff " + " ".join(repr(float(v)) for v in flat) + " 100 80", f"n_max {n_max[0]} {n_max[1]}", f"basis_size {basis[0]} {basis[1]}",
              f"l_max {l_max[0]} {l_max[1]} {l_max[2]}", f"ANN {neurons} 0"]
    lines += [f"{v:.17e}" for v in numbers] + [f"{v:.17e}" for v in scalers]
    opener = gzip.open if str(path).endswith(".gz") else open
    with opener(path, "wt") as f:
        f.write("\n".join(lines) + "\n")
    return dict(numbers=numbers, scalers=scalers, dim=dim, n_ann=n_ann, version=version, elements=list(elements), neurons=neurons,
                cutoffs=flat.reshape(-1, 2), n_max=n_max, basis=basis, l_max=l_max, zbl=zbl)


def argument_error_calls(L):
    """the raw C entry with arguments it must refuse before any device work -> (what was wrong, its return code), one by one.
    (Null array pointers: a call that got as far as touching one would not come back with an error code.)"""
    from mdapy_amd import _lib

    box, origin, pbc = np.eye(3) * 20.0, np.zeros(3), np.ones(3, np.int32)
    good = dict(T=2, NR=3, KR=4, NA=3, KA=4, L3=4, L4=2, L5=1, H=5, mode=0)
    zbl = np.array([1.0, 2.0, 0.0])

    def call(N=4, M=2, n_real=4, type_map=(0, 1), types=None, length=None, virial_sum=False, **head):
        h = dict(good, **head)
        dim = h["NR"] + h["NA"] * (h["L3"] + (h["L4"] == 2) + (h["L5"] == 1))
        size = 4 * h["T"] + dim + h["T"] ** 2 * (h["NR"] * h["KR"] + h["NA"] * h["KA"]) + h["T"] * (h["H"] * (dim + 2) + 1) + 1
        words = np.array([h[k] for k in ("T", "NR", "KR", "NA", "KA", "L3", "L4", "L5", "H", "mode")] + [size if length is None else length, 0], np.int32)
        tm = np.array(type_map, np.int32)
        ty = None if types is None else np.array(types, np.int32)
        nine = np.zeros(9)
        return L.mdh_nep(None, None, None, None if ty is None else ty.ctypes.data, N, tm.ctypes.data, len(tm), box.ctypes.data,
                         origin.ctypes.data, pbc.ctypes.data, None, None, None, M, None, words.ctypes.data, zbl.ctypes.data, n_real, None, None,
                         None, nine.ctypes.data if virial_sum else None, None, None, _lib.HOST, None)

    # NA = 17: a descriptor of 17 x 6 + 3 numbers, above the compiled maximum; types (0, 1, 2, 0): a type outside the type map
    for bad in (dict(NA=17), dict(NR=17), dict(KR=18), dict(H=129), dict(T=0), dict(NA=0), dict(L3=5), dict(L3=0), dict(L4=1), dict(L5=2),
                dict(L3=1, L4=2), dict(mode=3), dict(mode=1, length=7), dict(length=7), dict(type_map=(0, 2)), dict(type_map=(0, -2)),
                dict(types=(0, 1, 2, 0)), dict(types=(0, -1, 1, 0)), dict(M=1 << 23), dict(N=-1), dict(n_real=5), dict(virial_sum=True)):
        yield bad, call(**bad)
