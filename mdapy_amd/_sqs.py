"""Drop-in for ``mdapy._sqs`` (src/sqs.cpp:514-550): ``SQSEngine`` with the reference's attributes and methods.

Construction — channels, targets, tables — runs on the host; ``correlations``, ``per_channel_delta``, ``objective`` and ``run_mc``
run on the device (csrc/sqs.hip, whose header pins the arithmetic) and raise without one.  The chains are the library's own: the
reference's ``std::mt19937_64`` stream is not reproduced, everything deterministic is.  Extensions: ``replica_objectives``,
``winner`` and (on request) ``replica_best_types`` after ``run_mc``; ``run_mc(..., launch_steps=0, return_replicas=False)``;
``evaluate(types)`` for many type vectors at once."""
import itertools
import math

import numpy as np

from . import _lib

f64, i32, i64 = np.float64, np.int32, np.int64

MAX_ATOMS, MAX_SPECIES, MAX_GROUPS, LDS_CAP = 4096, 8, 1024, 65536
_TWO_PI = 6.283185307179586476925286766559


def trigo_basis(m):
    """phi[k][s], src/sqs.cpp:49-64: phi_{2t-1}(s) = -cos(2 pi t s / m), phi_{2t}(s) = -sin(2 pi t s / m)"""
    table = [[0.0] * m for _ in range(m - 1)]
    for s in range(m):
        for t in range(1, m // 2 + 1):
            table[2 * t - 2][s] = -math.cos(_TWO_PI * s * t / m)
        for t in range(1, (m + 1) // 2):
            table[2 * t - 1][s] = -math.sin(_TWO_PI * s * t / m)
    return table


def symmetrised_products(phi, m, n):
    """(function tuples, multisets, tab): tab[c][k] = the mean over the n! assignments of prod_p phi[f_p][s_q(p)] for function tuple
    c and species multiset k — products left to right, assignments q in lexicographic order, summed sequentially, one division"""
    funcs = list(itertools.combinations_with_replacement(range(m - 1), n))
    multisets = list(itertools.combinations_with_replacement(range(m), n))
    orders = list(itertools.permutations(range(n)))
    tab = np.zeros((len(funcs), len(multisets)), f64)
    for c, f in enumerate(funcs):
        for k, s in enumerate(multisets):
            total = 0.0
            for q in orders:
                term = 1.0
                for p in range(n):
                    term *= phi[f[p]][s[q[p]]]
                total += term
            tab[c, k] = total / float(len(orders))
    return funcs, multisets, tab


def multiset_index(m, n, multisets):
    """index of the multiset of every ordered species tuple, the tuple read as a base-m number"""
    where = {s: k for k, s in enumerate(multisets)}
    return np.array([where[tuple(sorted(t))] for t in itertools.product(range(m), repeat=n)], i32)


class SQSEngine:
    def __init__(self):
        self.n_atoms = 0
        self.n_species = 0
        self.n_func = 0
        self.point_corr = []
        self.shell_weight = []
        self.shell_diameter = []
        self.objective_mode = 1  # 0 = "abs", 1 = "atat"
        self.atat_tol = 1e-3
        self.atat_w_dist = 1.0
        self.atat_w_npts = 1.0
        self.replica_objectives = None
        self.replica_best_types = None
        self.winner = None
        self._phi = None
        self._bodies = []
        self._model = None

    # ---- construction (src/sqs.cpp:114-237)
    def set_species(self, m, conc):
        m = int(m)
        if m < 2:
            raise ValueError("n_species must be >= 2")
        if m > MAX_SPECIES:
            raise ValueError(f"n_species must be <= {MAX_SPECIES} (got {m})")
        if len(conc) != m:
            raise ValueError("conc size mismatch")
        self.n_species, self.n_func = m, m - 1
        self.concentrations = [float(c) for c in conc]
        self._phi = trigo_basis(m)
        self.point_corr = []
        for k in range(self.n_func):
            v = 0.0
            for s in range(m):
                v += self.concentrations[s] * self._phi[k][s]
            self.point_corr.append(v)
        self._model = None

    def add_cluster_body(self, n_pts, tuples_flat, shell_ids):
        n_pts = int(n_pts)
        if n_pts < 2 or n_pts > 4:
            raise ValueError("n_pts must be 2..4")
        shells = np.asarray(shell_ids, i64).reshape(-1)
        atoms = np.asarray(tuples_flat, i64).reshape(-1)
        if atoms.size != shells.size * n_pts:
            raise ValueError("tuples_flat size mismatch")
        if self.n_func == 0:
            raise RuntimeError("set_species() must be called first")
        if shells.size:
            self._bodies.append((n_pts, atoms.reshape(-1, n_pts), shells))
        self._model = None

    def finalize(self):
        N, m = int(self.n_atoms), self.n_species
        if N <= 0:
            raise RuntimeError("n_atoms must be set")
        if len(self.shell_diameter) == 0:
            raise RuntimeError("shell_diameter must be set before finalize()")
        if N < 2 or N > MAX_ATOMS:
            raise ValueError(f"n_atoms must be between 2 and {MAX_ATOMS} (got {N})")
        if not self._bodies:
            raise RuntimeError("add_cluster_body() must be called before finalize()")
        groups, per_group = {}, []  # (n_pts, shell) -> index, first come first served; [atoms arrays]
        for n, atoms, shells in self._bodies:
            if atoms.min() < 0 or atoms.max() >= N:
                raise RuntimeError("atom index out of range in instance")
            if shells.min() < 0 or shells.max() >= len(self.shell_diameter):
                raise RuntimeError("shell index out of range in instance")
            _, first = np.unique(shells, return_index=True)
            for sh in shells[np.sort(first)]:
                if (n, int(sh)) not in groups:
                    groups[(n, int(sh))] = len(groups)
                    per_group.append([])
                per_group[groups[(n, int(sh))]].append(atoms[shells == sh])
        G = len(groups)
        if G > MAX_GROUPS:
            raise ValueError(f"more than {MAX_GROUPS} (body, shell) groups (got {G})")
        by_body = {n: symmetrised_products(self._phi, m, n) for n in sorted({n for n, _ in groups})}
        tab_off, off = {}, 0
        for n, (_, _, tab) in by_body.items():
            tab_off[n] = off
            off += tab.size
        tab = np.concatenate([by_body[n][2].reshape(-1) for n in by_body])
        inst_atoms, inst_group, group_i, chan_i, channels = [], [], [], [], []
        hist_off = 0
        for (n, sh), g in groups.items():
            atoms = np.concatenate(per_group[g])
            funcs, multisets, _ = by_body[n]
            K = len(multisets)
            group_i.append((n, hist_off, len(channels), len(funcs), len(atoms), K))
            padded = np.full((len(atoms), 4), -1, i32)
            padded[:, :n] = atoms
            inst_atoms.append(padded)
            inst_group.append(np.full(len(atoms), g, i32))
            for c, f in enumerate(funcs):
                target = 1.0
                for p in range(n):
                    target *= self.point_corr[f[p]]
                chan_i.append((g, n - 2, tab_off[n] + c * K))
                channels.append((n, sh, list(f), len(atoms), target))
            hist_off += K
        inst_atoms, inst_group = np.concatenate(inst_atoms), np.concatenate(inst_group)
        C, H, I = len(channels), hist_off, len(inst_atoms)
        lds = 16 * C + 4 * H + 4 * ((G + 31) // 32) + 2 * ((N + 7) & ~7)
        if lds > LDS_CAP:
            raise ValueError(f"one replica's state needs {lds} bytes of LDS ({C} channels, {H} histogram bins, {N} atoms): the limit is {LDS_CAP}")
        # atom -> the instances that hold it, each once
        pairs = []
        for p in range(4):
            col = inst_atoms[:, p]
            fresh = col >= 0
            for q in range(p):
                fresh &= inst_atoms[:, q] != col
            pairs.append(np.column_stack([col[fresh], np.nonzero(fresh)[0]]))
        pairs = np.concatenate(pairs)
        pairs = pairs[np.lexsort((pairs[:, 1], pairs[:, 0]))]
        a2i_off = np.zeros(N + 1, i32)
        a2i_off[1:] = np.cumsum(np.bincount(pairs[:, 0], minlength=N))
        msidx = np.concatenate([multiset_index(m, n, by_body[n][1]) if n in by_body else np.zeros(m ** n, i32) for n in (2, 3, 4)])
        self._channels = channels
        self._model = dict(
            dims=np.array([N, m, I, G, C, H, tab.size, len(pairs)], i64), inst_atoms=np.ascontiguousarray(inst_atoms, i32),
            inst_group=np.ascontiguousarray(inst_group, i32), a2i_off=a2i_off, a2i=np.ascontiguousarray(pairs[:, 1], i32),
            group_i=np.array(group_i, i32), chan_i=np.array(chan_i, i32), tab=np.ascontiguousarray(tab, f64), msidx=msidx)

    # ---- what the reference reports
    def num_channels(self):
        return len(self._channels)

    def num_instances(self):
        return int(sum(ch[3] for ch in self._channels))  # (the reference holds one instance per channel, src/sqs.cpp:188-193)

    def channel_info(self, i):
        return self._channels[i]

    # ---- the device side
    def _tables(self):
        """the pointers of the model in the C ABI's order; objective settings are read now (they may change after finalize)"""
        if self._model is None:
            raise RuntimeError("finalize() must be called first")
        M = self._model
        weight, diam = [float(w) for w in self.shell_weight], [float(d) for d in self.shell_diameter]
        chan_d = np.zeros((len(self._channels), 4), f64)
        d_min, max_n = math.inf, 2
        for c, (n, sh, _, _, target) in enumerate(self._channels):
            chan_d[c] = (target, diam[sh], weight[sh], weight[sh] * math.pow(self.atat_w_npts, n - 2))
            d_min = min(d_min, diam[sh])
            max_n = max(max_n, n)
        if not math.isfinite(d_min) or d_min <= 0.0:
            d_min = 1.0
        n_body = max_n - 1
        maxdist0, reward = [0.0] * 3, [0.0] * 3
        for n, sh, _, _, _ in self._channels:
            if diam[sh] > maxdist0[n - 2]:
                maxdist0[n - 2] = diam[sh]
        for p in range(n_body):
            maxdist0[p] += d_min
            reward[p] = self.atat_w_dist * math.pow(self.atat_w_npts, p)
        if int(self.objective_mode) not in (0, 1):
            raise ValueError("objective_mode must be 0 (abs) or 1 (atat)")
        objp = np.array([int(self.objective_mode), self.atat_tol, d_min, n_body] + maxdist0 + reward, f64)
        keep = [M["dims"], M["inst_atoms"], M["inst_group"], M["a2i_off"], M["a2i"], M["group_i"], M["chan_i"], chan_d, M["tab"],
                M["msidx"], objp]
        return keep, [a.ctypes.data for a in keep]

    def _types(self, types, rows):
        if self._model is None:
            raise RuntimeError("finalize() must be called first")
        t = np.asarray(types, i64)
        if t.size == 0 or t.size % int(self.n_atoms) or (rows > 0 and t.size != rows * int(self.n_atoms)):
            raise ValueError("types size != n_atoms")
        t = np.ascontiguousarray(t.reshape(-1, int(self.n_atoms)), i32)
        if t.size and (t.min() < 0 or t.max() >= self.n_species):
            raise ValueError(f"species must lie in [0, {self.n_species})")
        return t

    def evaluate(self, types):
        """(hist (R, H) i32, corr (R, C), delta (R, C), objective (R)) of R type vectors (R, N)"""
        t = self._types(types, -1)
        keep, ptrs = self._tables()
        R, C, H = len(t), len(self._channels), int(self._model["dims"][5])
        if R < 1:
            raise ValueError("needs at least one type vector")
        hist, corr, delta, obj = np.zeros((R, H), i32), np.zeros((R, C)), np.zeros((R, C)), np.zeros(R)
        _lib.check(_lib.lib().mdh_sqs_count(*ptrs, t.ctypes.data, R, hist.ctypes.data, corr.ctypes.data, delta.ctypes.data,
                                            obj.ctypes.data, _lib.HOST, None))
        return hist, corr, delta, obj

    def correlations(self, types):
        return self.evaluate(self._types(types, 1))[1][0].tolist()

    def per_channel_delta(self, types):
        return self.evaluate(self._types(types, 1))[2][0].tolist()

    def objective(self, types):
        return float(self.evaluate(self._types(types, 1))[3][0])

    def run_mc(self, init_types, max_steps, T, n_replicas, seed, num_t=1, launch_steps=0, return_replicas=False):
        """src/sqs.cpp:379-509 -> (best types, best objective, its correlations); every chain's best objective is left in
        ``replica_objectives``, the winner's index in ``winner``"""
        if len(init_types) != int(self.n_atoms):
            raise RuntimeError("init_types size != n_atoms")
        t = self._types(init_types, 1)
        R, steps, T = int(n_replicas), int(max_steps), float(T)
        if R < 1:
            raise ValueError("n_replicas must be >= 1")
        if not T > 0.0:
            raise ValueError("T must be > 0")
        if steps < 0:
            raise ValueError("max_steps must be >= 0")
        if int(launch_steps) < 0:
            raise ValueError("launch_steps must be >= 0 (0: the library chooses)")
        keep, ptrs = self._tables()
        N, C = int(self.n_atoms), len(self._channels)
        winner, best_types, best_corr, objectives = np.zeros(1, i32), np.zeros(N, i32), np.zeros(C), np.zeros(R)
        every = np.zeros((R, N), np.uint8) if return_replicas else None
        _lib.check(_lib.lib().mdh_sqs_run(*ptrs, t.ctypes.data, steps, T, R, int(seed) & 0xFFFFFFFFFFFFFFFF, int(launch_steps),
                                          winner.ctypes.data, best_types.ctypes.data, best_corr.ctypes.data, objectives.ctypes.data,
                                          None if every is None else every.ctypes.data, _lib.HOST, None))
        self.replica_objectives, self.replica_best_types, self.winner = objectives, every, int(winner[0])
        return best_types.tolist(), float(objectives[self.winner]), best_corr.tolist()
