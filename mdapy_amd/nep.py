"""Neuroevolution-potential calculator — the drop-in for ``mdapy.nep.NEP`` (src/mdapy/nep.py, which wraps the NEP_CPU library
through src/neppy.cpp): reads a GPUMD ``nep.txt`` model and computes per-atom energies, forces and virials, the stress, the
descriptors and the latent space of a frame on the GPU.

    system.calc = NEP("nep.txt")
    system.get_energies(); system.get_force(); system.get_virials(); system.get_stress(); system.get_energy()
    system.calc.get_descriptor(system.data, system.box); system.calc.get_latentspace(system.data, system.box)

The model (Fan et al., Phys. Rev. B 104, 104309; J. Chem. Phys. 157, 114801; Song et al., Nat. Commun. 15, 10208 — PAPERS.md): the
energy of atom i is a one-hidden-layer tanh network of its descriptor, radial sums of Chebyshev radial functions and angular
invariants of real-harmonic sums over the neighbours, plus half of every pair's universal ZBL energy.  The arithmetic is written
from that definition (csrc/nep.hip; tests/_nep_ref.py restates it in numpy); of NEP_CPU only the conventions of the FILE are
followed: the order of the parameters, the sign of the biases, the tables of the format.

In scope: ``nep3``, ``nep4``, ``nep5`` potential models, each with or without ``_zbl`` (universal ZBL, with its optional typewise
factor), global or per-type cutoffs, ``l_max`` 3-body up to 4, 4-body 0 or 2, 5-body 0 or 1.  The constructor raises
``NotImplementedError`` for flexible ZBL, the dipole and polarizability models and ``l_max`` above 4.  The charge models
(``nep4_charge1/2/3``) are read by ``QNEP``, a subclass; ``NEP`` refuses them and says so, and ``load(filename)`` returns the class
the head line asks for.

What differs from the reference:

* **the list** is the System's own (``_list_calculator.py``): the one it remembers when it reaches ``rc``, the replica of a thin
  box, the cell-sorted twin.  NEP_CPU builds lists of its own, and sums in the order of those.
* **open boundaries** are the System's: no images along an open axis.  The reference pads the box by ``3 rc`` there instead and
  keeps it periodic — the same neighbours.
* **the sums run in a fixed order** and every atom GATHERS its forces and virials; the reference scatters ``+=`` into the
  neighbours' rows from CPU threads.  Two runs give the same bits here.
* **the stress** divides the REAL atoms' virial sum by the real box's volume, as ``EAM`` does.
* a malformed file raises ``ValueError`` with the line; NEP_CPU ends the process.
* **charge models have a class of their own**, ``QNEP``; the reference's one ``NEP`` reads both kinds.
* **the exact 2 pi** in the reciprocal vectors of the Ewald sum; NEP_CPU truncates it to 6.2831853 (phases differ by less than 1e-7).
* **the BEC with per-type cutoffs**: dq_i/dr_ij uses the pair's own cutoff, the one the charge was computed with; NEP_CPU takes the
  largest cutoff there."""
import gzip
import os
import re

import numpy as np

from . import kernels
from ._list_calculator import ListCalculator
from .devarray import empty

# the periodic table as far as the format knows it: Z = place + 1
SYMBOLS = ("H He Li Be B C N O F Ne Na Mg Al Si P S Cl Ar K Ca Sc Ti V Cr Mn Fe Co Ni Cu Zn Ga Ge As Se Br Kr Rb Sr Y Zr Nb Mo Tc Ru Rh "
           "Pd Ag Cd In Sn Sb Te I Xe Cs Ba La Ce Pr Nd Pm Sm Eu Gd Tb Dy Ho Er Tm Yb Lu Hf Ta W Re Os Ir Pt Au Hg Tl Pb Bi Po At Rn "
           "Fr Ra Ac Th Pa U Np Pu").split()
# covalent radii in A by Z - 1: a table of the NEP format (GPUMD's typewise ZBL cutoff, `zbl rc_inner rc_outer factor`)
COVALENT_RADIUS = (
    0.426667, 0.613333, 1.6, 1.25333, 1.02667, 1.0, 0.946667, 0.84, 0.853333, 0.893333, 1.86667, 1.66667, 1.50667, 1.38667, 1.46667, 1.36,
    1.32, 1.28, 2.34667, 2.05333, 1.77333, 1.62667, 1.61333, 1.46667, 1.42667, 1.38667, 1.33333, 1.32, 1.34667, 1.45333, 1.49333,
    1.45333, 1.53333, 1.46667, 1.52, 1.56, 2.52, 2.22667, 1.96, 1.85333, 1.76, 1.65333, 1.53333, 1.50667, 1.50667, 1.44, 1.53333, 1.64,
    1.70667, 1.68, 1.68, 1.64, 1.76, 1.74667, 2.78667, 2.34667, 2.16, 1.96, 2.10667, 2.09333, 2.08, 2.06667, 2.01333, 2.02667, 2.01333,
    2.0, 1.98667, 1.98667, 1.97333, 2.04, 1.94667, 1.82667, 1.74667, 1.64, 1.57333, 1.54667, 1.48, 1.49333, 1.50667, 1.76, 1.73333,
    1.73333, 1.81333, 1.74667, 1.84, 1.89333, 2.68, 2.41333, 2.22667, 2.10667, 2.02667, 2.04, 2.05333, 2.06667)
_HEAD = re.compile(r"^nep(\d+)(_zbl)?(_[a-z]+\d*)?$")
_OTHER_MODELS = {"_dipole": "dipole models", "_polarizability": "polarizability models", "_temperature": "temperature-dependent models",
                 "_charge1": "charge models", "_charge2": "charge models", "_charge3": "charge models"}


class NEP(ListCalculator):
    _charge_heads = False  # (QNEP: True — which of the two kinds of head this class reads)

    def __init__(self, filename):
        if not os.path.exists(filename):
            raise FileNotFoundError(f"{filename} does not exist.")
        self.filename = filename
        self.results = {}
        self._read()
        self.rc = max(self.info["radial_cutoff"], self.info["angular_cutoff"])
        self._types = None
        self._present = None  # (an element column, the file types its atoms have)
        self._models = {}  # the types present in a frame -> (kernels.nep as it was, its Model of the compacted block)

    # ------------------------------------------------------------------ the file
    def _read(self):
        """the text format: the head line ``nepV[_zbl] T symbols..``, ``zbl inner outer [factor]`` when the head says so, ``cutoff``
        (two numbers, or two per type, then the two list widths), ``n_max``, ``basis_size``, ``l_max``, ``ANN neurons 0``, then one
        number per line: the networks — nep3 one for all types, nep4 one per type, nep5 one per type with a bias of its own after
        ``w1`` — each ``w0`` (neurons x dim), ``b0``, ``w1``; the common bias; the descriptor coefficients c[n][k][t1][t2], radial
        block then angular block; the ``dim`` descriptor scalers."""
        source = gzip.open if str(self.filename).endswith(".gz") else open
        with source(self.filename, "rt") as f:
            lines = f.read().split("\n")
        at = [0]

        def words(first=None, counts=None):
            while at[0] < len(lines) and not lines[at[0]].split():
                at[0] += 1
            if at[0] >= len(lines):
                raise ValueError(f"NEP file '{self.filename}' ended at line {at[0] + 1} while expecting '{first or 'a number'}'.")
            line = lines[at[0]]
            at[0] += 1
            got = line.split()
            if first is not None and (got[0] != first or (counts is not None and len(got) not in counts)):
                raise ValueError(f"NEP file '{self.filename}', line {at[0]}: expected '{first}' with {counts} words, got: {line.strip()!r}")
            return got, line

        head, line = words()
        match = _HEAD.match(head[0])
        if match is None or match.group(3) not in (None,) + tuple(_OTHER_MODELS) or match.group(1) not in "345":
            raise ValueError(f"NEP file '{self.filename}', line 1: '{head[0]}' is no NEP model this reader knows: {line.strip()!r}")
        charge = int(match.group(3)[-1]) if (match.group(3) or "").startswith("_charge") else 0
        if charge and self._charge_heads and match.group(1) != "4":
            raise ValueError(f"NEP file '{self.filename}', line 1: '{head[0]}' is no NEP model this reader knows: {line.strip()!r}")
        if match.group(3) is not None and not (charge and self._charge_heads):
            hint = "; use mdapy_amd.QNEP" if charge else ""
            raise NotImplementedError(f"NEP: {_OTHER_MODELS[match.group(3)]} ('{head[0]}') are not supported, only potential models{hint}.")
        if self._charge_heads and not charge:
            raise ValueError(f"QNEP: '{head[0]}' ('{self.filename}') is no charge model; use mdapy_amd.NEP.")
        version, zbl = int(match.group(1)), match.group(2) is not None
        try:
            count = int(head[1])
        except (IndexError, ValueError):
            raise ValueError(f"NEP file '{self.filename}', line 1: no number of types: {line.strip()!r}") from None
        if len(head) != 2 + count:
            raise ValueError(f"NEP file '{self.filename}', line 1: {count} element symbols expected, {len(head) - 2} found: {line.strip()!r}")
        self.element_list = head[2:]
        for name in self.element_list:
            if name not in SYMBOLS:
                raise ValueError(f"NEP file '{self.filename}', line 1: '{name}' is no element symbol: {line.strip()!r}")
        self.zbl_inner = self.zbl_outer = self.zbl_factor = 0.0
        self.zbl_mode = 0  # 0: none, 1: universal between inner and outer, 2: typewise outer radius
        try:
            if zbl:
                got, line = words("zbl", (3, 4))
                self.zbl_inner, self.zbl_outer = float(got[1]), float(got[2])
                if self.zbl_inner == 0.0 and self.zbl_outer == 0.0:
                    raise NotImplementedError("NEP: flexible ZBL ('zbl 0 0') is not supported.")
                self.zbl_mode = 1
                if len(got) == 4:
                    self.zbl_factor, self.zbl_mode = float(got[3]), 2
            got, line = words("cutoff", (5, 2 * count + 3))
            pairs = np.array([float(w) for w in got[1:-2]]).reshape(-1, 2)
            self.rc_radial = np.ascontiguousarray(np.broadcast_to(pairs[:, 0], (count,)) if len(pairs) == 1 else pairs[:, 0])
            self.rc_angular = np.ascontiguousarray(np.broadcast_to(pairs[:, 1], (count,)) if len(pairs) == 1 else pairs[:, 1])
            got, line = words("n_max", (3,))
            n_rad, n_ang = int(got[1]) + 1, int(got[2]) + 1
            got, line = words("basis_size", (3,))
            k_rad, k_ang = int(got[1]) + 1, int(got[2]) + 1
            got, line = words("l_max", (4,))
            l3, l4, l5 = int(got[1]), int(got[2]), int(got[3])
            got, line = words("ANN", (3,))
            neurons = int(got[1])
        except ValueError as e:
            if "NEP file" in str(e):
                raise
            raise ValueError(f"NEP file '{self.filename}', line {at[0]}: {e}: {line.strip()!r}") from None
        if l3 > 4:
            raise NotImplementedError(f"NEP: l_max {l3} is not supported (3-body l_max up to 4).")
        if l3 < 1 or l4 not in (0, 2) or l5 not in (0, 1) or (l4 == 2 and l3 < 2):
            raise ValueError(f"NEP file '{self.filename}', line {at[0] - 1}: l_max {l3} {l4} {l5} is outside the format")
        orders = l3 + (l4 == 2) + (l5 == 1)
        dim = n_rad + n_ang * orders
        per_net = neurons * (dim + 2) + (version == 5) + (neurons if charge else 0)
        nets = 1 if version == 3 else count
        n_ann = per_net * nets + 1 + (charge > 0)
        n_c_rad, n_c_ang = count * count * n_rad * k_rad, count * count * n_ang * k_ang
        total = n_ann + n_c_rad + n_c_ang
        numbers = np.empty(total + dim)
        for k in range(total + dim):
            got, line = words()
            try:
                numbers[k] = float(got[0])
            except ValueError:
                raise ValueError(f"NEP file '{self.filename}', line {at[0]}: not a number: {line.strip()!r}") from None
        self.w0, self.b0, self.w1, self.bias, self.w1_charge = [], [], [], [], []
        for t in range(count):
            p = numbers[(t if nets > 1 else 0) * per_net:][:per_net]
            self.w0.append(p[:neurons * dim].reshape(neurons, dim))
            self.b0.append(p[neurons * dim:neurons * (dim + 1)])
            self.w1.append(p[neurons * (dim + 1):neurons * (dim + 2)])
            self.bias.append(float(p[-1]) if version == 5 else 0.0)
            if charge:  # the second output row of w1: the charge's weights
                self.w1_charge.append(p[neurons * (dim + 2):neurons * (dim + 3)])
        self.b1 = float(numbers[n_ann - 1])
        self.sqrt_epsilon_inf = float(numbers[n_ann - 2]) if charge else 1.0
        # c[n][k][t1][t2] of the file -> [t1][t2][n][k]: the coefficients of one pair of types and one n lie together
        self.c_radial = np.ascontiguousarray(numbers[n_ann:n_ann + n_c_rad].reshape(n_rad, k_rad, count, count).transpose(2, 3, 0, 1))
        self.c_angular = np.ascontiguousarray(numbers[n_ann + n_c_rad:total].reshape(n_ang, k_ang, count, count).transpose(2, 3, 0, 1))
        self.q_scaler = numbers[total:].copy()
        self.info = {"model_type": 0, "version": version, "charge_mode": charge, "zbl": zbl, "radial_cutoff": float(self.rc_radial.max()),
                     "angular_cutoff": float(self.rc_angular.max()), "n_max_radial": n_rad - 1, "n_max_angular": n_ang - 1,
                     "basis_size_radial": k_rad - 1, "basis_size_angular": k_ang - 1, "l_max_3body": l3, "l_max_4body": l4,
                     "l_max_5body": l5, "num_ndim": dim, "num_nlatent": neurons, "num_para": total, "element_list": list(self.element_list)}

    # ------------------------------------------------------------------ the model block of the types a frame holds
    def _model(self, present):
        """the kernels' model for the file types ``present`` (sorted): header words and one f64 block in the order
        include/mdapy_amd.h states — cutoffs, atomic numbers and covalent radii per type, the scalers, the descriptor coefficients of
        the present pairs, the present types' networks, the common bias"""
        held = self._models.get(present)
        if held is None or held[0] is not kernels.nep:
            held = self._models[present] = (kernels.nep, kernels.nep.Model(*self._model_arrays(present)))
        return held[1]

    def _model_arrays(self, present):
        """-> (header words i32, the three ZBL numbers, the f64 block)"""
        info, pick = self.info, list(present)
        z = np.array([SYMBOLS.index(self.element_list[t]) + 1 for t in pick], np.float64)
        parts = [self.rc_radial[pick], self.rc_angular[pick], z, np.array([COVALENT_RADIUS[int(v) - 1] for v in z]), self.q_scaler,
                 self.c_radial[np.ix_(pick, pick)].ravel(), self.c_angular[np.ix_(pick, pick)].ravel()]
        for t in pick:
            parts += [self.w0[t].ravel(), self.b0[t], self.w1[t], [self.bias[t]]]
        parts.append([self.b1])
        block = np.ascontiguousarray(np.concatenate([np.asarray(p, np.float64).ravel() for p in parts]))
        head = np.array([len(pick), info["n_max_radial"] + 1, info["basis_size_radial"] + 1, info["n_max_angular"] + 1,
                         info["basis_size_angular"] + 1, info["l_max_3body"], info["l_max_4body"], info["l_max_5body"], info["num_nlatent"],
                         self.zbl_mode, len(block), 0], np.int32)
        return head, np.array([self.zbl_inner, self.zbl_outer, self.zbl_factor]), block

    # ------------------------------------------------------------------ the calculation (_list_calculator.py)
    def _element_list(self):
        return self.element_list

    def _missing_column(self, name):
        return f"data must contain {name} property."

    def _unknown_element(self, name):
        return f"NEP model did not include {name}."

    def _present_types(self):
        """-> ((an element column, the file types its atoms have), the map from a file type to the compacted model's, -1: absent)"""
        held = self._types  # (types of the System's own column: what is present there is present in its replica and its twin)
        present = self._present
        if present is None or present[0] is not held[0]:
            present = self._present = (held[0], tuple(int(t) for t in np.unique(held[1])))
        local = np.full(len(self.element_list), -1, np.int32)
        local[list(present[1])] = np.arange(len(present[1]), dtype=np.int32)
        return present, local

    def _extra_outputs(self, more, atoms):
        """the arrays for the further outputs ``more`` names ('descriptor', 'latent'), put into ``more`` and returned as keywords"""
        extra = {}
        if more is not None:
            widths = {"descriptor": self.info["num_ndim"], "latent": self.info["num_nlatent"]}
            for name in more:
                extra[name] = more[name] = empty((atoms, widths[name]), np.float64)
        return extra

    def _launch(self, cols, types, cell, rows, dist, counts, energy, force, virial, real, total, threads, more):
        present, local = self._present_types()
        extra = self._extra_outputs(more, int(rows.shape[0]))
        kernels.nep.calculate(*cols, types, local, cell.box, cell.origin, cell.boundary, rows, dist, counts, self._model(present[1]),
                              energy=energy, force=force, virial=virial, virial_sum=total, n_real=real, **extra)

    def _extra(self, name, data, box):
        more = {name: None}
        raw = self._run_kernels(self._system_of(data, box), None, more)
        return self._rows_back((more[name],), raw[4], raw[5])[0]

    def get_descriptor(self, data, box):
        """(N, num_ndim): every atom's descriptor, times the model's scalers"""
        return self._extra("descriptor", data, box)

    def get_latentspace(self, data, box):
        """(N, num_nlatent): the hidden layer's contributions w1[n] * tanh(..) to every atom's energy"""
        return self._extra("latent", data, box)

    def get_charges(self, data, box):
        raise ValueError("Charges is only available for qNEP.")

    def get_bec(self, data, box):
        raise ValueError("bec is only available for qNEP.")


class QNEP(NEP):
    """The charge-aware models of GPUMD (``nep4_charge1/2/3`` and their ``_zbl`` forms): the network has a second output, the atom's
    charge q_i; the mean charge of the frame is removed; and the energy gains the electrostatic energy of the charges — mode 1: the
    Ewald sum (k-space plus real space), mode 2: its k-space part alone, mode 3: a real-space sum that is shifted to vanish with its
    derivative at the cutoff.  The Ewald parameter is fixed by the format, alpha = pi / rc_radial.  ``results`` gains ``"charges"``
    (N,) and ``"bec"`` (N, 9): the Born effective charges q_i 1 + sum_j r_ij (x) dq/dr, times the model's sqrt(epsilon_inf).

    The k-space part sums over every k-point below 2 pi alpha for every atom: the number of k-points grows with the volume, so this
    part is O(N^2) — the reference's method; particle-mesh Ewald is out of scope.  Every calculation works out charges and BEC as
    well, and makes and uploads the k-points anew, whether or not the cell has changed."""
    _charge_heads = True

    def _model_arrays(self, present):
        """NEP's block with the charge's weights after every type's ``w1`` and sqrt(epsilon_inf) before the common bias; the last
        header word is the charge mode"""
        info, pick = self.info, list(present)
        z = np.array([SYMBOLS.index(self.element_list[t]) + 1 for t in pick], np.float64)
        parts = [self.rc_radial[pick], self.rc_angular[pick], z, np.array([COVALENT_RADIUS[int(v) - 1] for v in z]), self.q_scaler,
                 self.c_radial[np.ix_(pick, pick)].ravel(), self.c_angular[np.ix_(pick, pick)].ravel()]
        for t in pick:
            parts += [self.w0[t].ravel(), self.b0[t], self.w1[t], self.w1_charge[t], [self.bias[t]]]
        parts += [[self.sqrt_epsilon_inf], [self.b1]]
        block = np.ascontiguousarray(np.concatenate([np.asarray(p, np.float64).ravel() for p in parts]))
        head = np.array([len(pick), info["n_max_radial"] + 1, info["basis_size_radial"] + 1, info["n_max_angular"] + 1,
                         info["basis_size_angular"] + 1, info["l_max_3body"], info["l_max_4body"], info["l_max_5body"], info["num_nlatent"],
                         self.zbl_mode, len(block), info["charge_mode"]], np.int32)
        return head, np.array([self.zbl_inner, self.zbl_outer, self.zbl_factor]), block

    def _ewald_cell(self, box):
        """the cell whose reciprocal vectors the k-space sum runs over: the real cell, an open axis lengthened by 3 rc (the
        reference keeps such an axis periodic in a box padded by that much)"""
        cell = np.array(box.box, np.float64)
        for axis in range(3):
            if not box.boundary[axis]:
                cell[axis] *= 1.0 + 3.0 * self.rc / np.linalg.norm(cell[axis])
        return cell

    def _run_kernels(self, system, total=None, more=None):
        self._cell = self._ewald_cell(system.box)  # (a replica's passes run in the replicated cell; the k-points are the real cell's)
        return super()._run_kernels(system, total, more)

    def _launch(self, cols, types, cell, rows, dist, counts, energy, force, virial, real, total, threads, more):
        present, local = self._present_types()
        atoms = int(rows.shape[0])
        extra = self._extra_outputs(more, atoms)
        charge, bec = empty(atoms, np.float64), empty((atoms, 9), np.float64)
        kernels.nep.calculate_charge(*cols, types, local, cell.box, cell.origin, cell.boundary, rows, dist, counts, self._model(present[1]),
                                     self._cell, self.info["radial_cutoff"], energy=energy, force=force, virial=virial, virial_sum=total,
                                     charge=charge, bec=bec, n_real=real, **extra)
        self._last = (charge, bec)

    def _to_results(self, system, energy, force, virial, total, perm, real):
        super()._to_results(system, energy, force, virial, total, perm, real)
        self.results["charges"], self.results["bec"] = self._rows_back(self._last, perm, real)

    def get_charges(self, data, box):
        """(N,): every atom's charge, the frame's mean removed"""
        return self._result("charges", data, box)

    def get_bec(self, data, box):
        """(N, 9): every atom's Born effective charge tensor, row-major"""
        return self._result("bec", data, box)


def load(filename):
    """``NEP`` or ``QNEP`` by the file's head line"""
    if not os.path.exists(filename):
        raise FileNotFoundError(f"{filename} does not exist.")
    source = gzip.open if str(filename).endswith(".gz") else open
    with source(filename, "rt") as f:
        for line in f:
            if line.split():
                match = _HEAD.match(line.split()[0])
                if match is not None and (match.group(3) or "").startswith("_charge"):
                    return QNEP(filename)
                break
    return NEP(filename)
