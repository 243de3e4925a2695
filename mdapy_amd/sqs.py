"""Special quasirandom structures — the drop-in for ``mdapy.sqs.SQS`` (src/mdapy/sqs.py), an ATAT-mcsqs-style search
(van de Walle et al., CALPHAD 42, 13-18 (2013)).

Take a ``System`` holding a random alloy (``build_hea``), enumerate pair / triplet / quadruplet clusters over every periodic
image direction, and let many independent Monte-Carlo chains swap species until the cluster correlations match those of the
fully random alloy; the best chain wins.  The chains run on the GPU, one wavefront each (csrc/sqs.hip), so ``n_replicas`` in
the thousands costs what a handful does.  The chains draw the library's own counter-based random numbers: a seed gives the
same structure on every run here, not the reference's.

>>> hea = mp.build_hea(("Cr", "Co", "Ni"), (1/3,) * 3, "fcc", 3.53, nx=3, ny=3, nz=3, random_seed=1)
>>> sqs = mp.SQS(hea, cutoffs={2: 4.0, 3: 3.0}, n_replicas=1024).compute()
>>> sqs.is_sqs()

``cutoffs`` maps a body order (2 required; 3, 4 optional) to its cutoff: "just past the shell you want to constrain"."""
from collections import Counter

import numpy as np

from . import kernels

_OBJECTIVE_MODE_ATAT = 1
_ATAT_TOL = 1e-3
_SHELL_TOL = 0.05
_WEIGHT_DECAY = 0.0
_WEIGHT_NPTS = 1.0


def _bin_first_come(values):
    """src/mdapy/sqs.py:360-374 without the loop over members: a member joins the first bin — bins in order of creation — whose
    founder it matches within ``_SHELL_TOL`` in every component, else founds one.  -> (bin of every member, founders)"""
    values = np.asarray(values, np.float64).reshape(len(values), -1)
    bins = np.full(len(values), -1, np.int64)
    founders = []
    while True:
        open_ = np.nonzero(bins < 0)[0]
        if not len(open_):
            return bins, founders
        # whoever is still open matched no earlier bin, and the bins founded after this one come later in the list
        founder = values[open_[0]]
        joins = open_[np.all(np.abs(values[open_] - founder) < _SHELL_TOL, axis=1)]
        bins[joins] = len(founders)
        founders.append(founder)


def image_neighbors(pos, box, rc_max):
    """src/mdapy/sqs.py:208-264 -> per atom (j, position of that image of j, distance), every image direction on its own, in the
    reference's order: image offsets (nx, ny, nz)-lexicographic, j ascending within an image"""
    pos, box = np.asarray(pos, np.float64), np.asarray(box, np.float64)
    N = len(pos)
    nmax = [max(1, int(np.ceil(rc_max / length)) + 1) for length in np.linalg.norm(box, axis=1)]
    found = []
    number = 0
    rows = max(1, min(N, (1 << 22) // max(N, 1)))
    for nx in range(-nmax[0], nmax[0] + 1):
        for ny in range(-nmax[1], nmax[1] + 1):
            for nz in range(-nmax[2], nmax[2] + 1):
                img = nx * box[0] + ny * box[1] + nz * box[2]
                for i0 in range(0, N, rows):  # (blocks of origin atoms: the N x N x 3 differences of 4096 atoms are 400 MB)
                    delta = pos[None, :, :] + img[None, None, :] - pos[i0:i0 + rows, None, :]
                    dist = np.linalg.norm(delta, axis=2)
                    mask = dist <= rc_max + 1e-9
                    if nx == 0 and ny == 0 and nz == 0:
                        mask[np.arange(len(mask)), i0 + np.arange(len(mask))] = False
                    ii, jj = np.nonzero(mask)
                    if len(ii):
                        found.append((ii + i0, np.full(len(ii), number), jj, pos[jj] + img, dist[ii, jj]))
                number += 1
    ii, nn, jj, where, dist = (np.concatenate(c) for c in zip(*found)) if found else (np.zeros(0, np.int64),) * 3 + (np.zeros((0, 3)), np.zeros(0))
    order = np.lexsort((jj, nn, ii))
    ii, jj, where, dist = ii[order], jj[order], where[order], dist[order]
    start = np.searchsorted(ii, np.arange(N + 1))
    return [(jj[start[i]:start[i + 1]], where[start[i]:start[i + 1]], dist[start[i]:start[i + 1]]) for i in range(N)]


def enumerate_clusters(pos, box, cutoffs):
    """src/mdapy/sqs.py:266-358 -> (per_body, all_diams, global_map); per_body = [(n_pts, {local shell: (k, n_pts) atoms}, shell
    diameters)], one instance per (origin atom, image direction), in the reference's order"""
    nbrs = image_neighbors(pos, box, max(cutoffs.values()))
    N = len(nbrs)
    per_body = []
    for n in (2, 3, 4):
        if n not in cutoffs:
            continue
        rc = float(cutoffs[n]) + 1e-9
        atoms, sigs = [], []
        for i in range(N):
            j, where, d = nbrs[i]
            ok = d <= rc
            j, where, d = j[ok], where[ok], d[ok]
            if n == 2:
                atoms.append(np.column_stack([np.full(len(j), i), j]))
                sigs.append(d[:, None])
                continue
            between = np.linalg.norm(where[:, None, :] - where[None, :, :], axis=2)
            near = np.triu(between <= rc, 1)
            if n == 3:
                a, b = np.nonzero(near)
                atoms.append(np.column_stack([np.full(len(a), i), j[a], j[b]]))
                sigs.append(np.sort(np.column_stack([d[a], d[b], between[a, b]]), axis=1))
            else:
                a, b, c = np.nonzero(near[:, :, None] & near[:, None, :] & near[None, :, :])
                atoms.append(np.column_stack([np.full(len(a), i), j[a], j[b], j[c]]))
                sigs.append(np.sort(np.column_stack([d[a], d[b], d[c], between[a, b], between[a, c], between[b, c]]), axis=1))
        atoms, sigs = np.concatenate(atoms).astype(np.int32), np.concatenate(sigs)
        shell, founders = _bin_first_come(sigs)
        per_shell = {s: atoms[shell == s] for s in range(len(founders))}
        per_body.append((n, per_shell, [float(f[-1]) for f in founders]))
    all_diams, global_map = [], []
    for _, _, diams in per_body:
        mapping = []
        for d in diams:
            hit = next((k for k, known in enumerate(all_diams) if abs(known - d) < _SHELL_TOL), -1)
            if hit < 0:
                all_diams.append(d)
                hit = len(all_diams) - 1
            mapping.append(hit)
        global_map.append(mapping)
    return per_body, all_diams, global_map


class SQS:
    """``SQS(system, cutoffs, n_replicas=4, max_steps=100000, T=0.05, seed=0).compute()`` -> ``system`` (the input's atoms and
    cell, species reshuffled), ``objective``, ``correlations`` (n_channels), ``channel_info`` (per channel: n_pts, shell, diameter,
    funcs, n_instances, target, corr) and ``replica_objectives`` (n_replicas: every chain's best objective).  ``max_steps <= 0``
    evaluates the input as it stands."""

    _BODIES = ((2, "pair"), (3, "triplet"), (4, "quad"))

    def __init__(self, system, cutoffs, n_replicas=4, max_steps=100000, T=0.05, seed=0):
        if 2 not in cutoffs:
            raise ValueError("cutoffs must include key 2 (pair cutoff in Å)")
        strange = [k for k in cutoffs if k not in (2, 3, 4)]
        if strange:
            raise ValueError(f"only 2-, 3- and 4-body cutoffs are supported (got {strange[0]})")
        self._sys_in, self.cutoffs = system, dict(cutoffs)
        self.n_replicas, self.max_steps, self.T, self.seed = int(n_replicas), int(max_steps), float(T), int(seed)
        self.system = self.objective = self.correlations = self.channel_info = self.replica_objectives = None
        self._engine = self._best_types = self._species_labels = None

    def _species(self):
        """(0-based species per atom, labels, the column that carries them): element names in sorted order, else ``type - 1``"""
        data = self._sys_in.data
        if "element" in data.columns:
            labels, codes = np.unique(data["element"].to_numpy().astype(str), return_inverse=True)
            return codes.astype(np.int64), labels.tolist(), "element"
        if "type" not in data.columns:
            raise ValueError("System must have an 'element' or 'type' column")
        codes = np.asarray(data["type"].to_numpy(), np.int64) - 1
        return codes, list(range(int(codes.max()) + 1)), "type"

    def _make_engine(self, species, kinds):
        """the engine with every cluster of the cell in it -> (engine, diameter of every shell)"""
        frame = self._sys_in.data
        pos = np.column_stack([frame[c].to_numpy() for c in "xyz"]).astype(np.float64)
        per_body, diameters, shell_of = enumerate_clusters(pos, np.array(self._sys_in.box.box, np.float64), self.cutoffs)
        engine = kernels.sqs.SQSEngine()
        engine.n_atoms = len(pos)
        engine.set_species(kinds, (np.bincount(species, minlength=kinds).astype(np.float64) / len(pos)).tolist())
        engine.objective_mode, engine.atat_tol = _OBJECTIVE_MODE_ATAT, _ATAT_TOL
        engine.atat_w_dist, engine.atat_w_npts = 1.0, _WEIGHT_NPTS
        for (n_pts, shells, _), to_global in zip(per_body, shell_of):
            for local, atoms in shells.items():
                engine.add_cluster_body(n_pts, np.asarray(atoms, np.int32).reshape(-1), [int(to_global[local])] * len(atoms))
        nearest = min(diameters)
        engine.shell_weight = [float(np.exp(-_WEIGHT_DECAY * (d - nearest))) for d in diameters]
        engine.shell_diameter = list(diameters)
        engine.finalize()
        return engine, diameters

    def compute(self):
        """run the search (src/mdapy/sqs.py:377-455); returns ``self``"""
        from .system import System

        species, labels, column = self._species()
        engine, diameters = self._make_engine(species, len(labels))
        if self.max_steps > 0:
            best, objective, corr = engine.run_mc(species.tolist(), self.max_steps, self.T, self.n_replicas, self.seed, 1)
            self.replica_objectives = np.array(engine.replica_objectives, np.float64)
        else:  # the input as it stands, unshuffled
            best = species.tolist()
            corr, objective = engine.correlations(best), engine.objective(best)
            self.replica_objectives = np.full(self.n_replicas, float(objective))
        columns = {"type": np.asarray(best, np.int32) + 1}
        if column == "element":
            columns["element"] = np.array([labels[t] for t in best], dtype=object)
        self.system = System(data=self._sys_in.data.with_columns(**columns), box=self._sys_in.box)
        self.objective, self.correlations = float(objective), np.array(corr, np.float64)
        self._engine, self._best_types, self._species_labels = engine, np.array(best, np.int64), labels
        keys = ("n_pts", "shell", "funcs", "n_instances", "target")
        self.channel_info = []
        for c in range(engine.num_channels()):
            entry = dict(zip(keys, engine.channel_info(c)))
            self.channel_info.append({"n_pts": int(entry["n_pts"]), "shell": int(entry["shell"]), "diameter": float(diameters[entry["shell"]]),
                                      "funcs": list(entry["funcs"]), "n_instances": int(entry["n_instances"]),
                                      "target": float(entry["target"]), "corr": float(self.correlations[c])})
        return self

    def _warren_cowley(self):
        """per pair shell, nearest first: the Warren-Cowley matrix of the result over a list that ends just past the shell"""
        rows = []
        for diameter in sorted({c["diameter"] for c in self.channel_info if c["n_pts"] == 2}):
            rc = diameter + _SHELL_TOL
            self.system.build_neighbor(rc=rc)
            alpha = self.system.cal_warren_cowley_parameter(rc=rc).WCP
            rows.append({"shell": f"NN{len(rows) + 1}", "diameter": float(diameter), "rc": float(rc), "max_abs": float(np.abs(alpha).max()),
                         "max_off_diag": float(np.abs(alpha - np.diag(np.diag(alpha))).max()), "matrix": alpha})
        return rows

    def is_sqs(self, tol=0.03, verbose=True):
        """src/mdapy/sqs.py:458-588 -> (verdict, info): the verdict is ``max |pi - target| < tol`` over every channel; the
        Warren-Cowley parameters of each pair shell are reported beside it and do not enter it"""
        if self._engine is None:
            raise RuntimeError("call compute() before is_sqs()")
        residual = np.asarray(self._engine.per_channel_delta(self._best_types.tolist()), np.float64)
        worst = float(residual.max()) if residual.size else 0.0
        verdict = worst < tol
        shells = self._warren_cowley()
        info = {"verdict": verdict, "absolute": {"pass": verdict, "max_delta": worst, "tol": tol},
                "warren_cowley": {"tol": tol, "per_shell": shells}}
        if verbose:
            print(self._report(tol, worst, verdict, shells))
        return verdict, info

    def _report(self, tol, worst, verdict, shells):
        held = Counter(self._best_types.tolist())
        comp_str = ", ".join(f"{self._species_labels[t]}({held[t]})" for t in sorted(held))
        per_body = Counter(c["n_pts"] for c in self.channel_info)
        body_str = "  ".join(f"{name}={per_body[n]}" for n, name in self._BODIES if per_body[n] > 0)
        lines = [f"SQS verification ({self._sys_in.N} atoms; species: {comp_str})", "-" * 60,
                 f"correlations    : {len(self.channel_info)} channels  ({body_str})", f"objective       : {self.objective:.5f}", "",
                 f"absolute residual   max|pi - target| = {worst:.4f}   tol={tol:.3f}   {'PASS' if verdict else 'FAIL'}    <- decides verdict"]
        lines += [f"WCP {s['shell']:>3s}  d={s['diameter']:.3f} A    max|alpha|={s['max_abs']:.4f}   tol={tol:.3f}   INFO" for s in shells]
        return "\n".join(lines + ["", f"Verdict: {'SQS' if verdict else 'NOT YET'}"])
