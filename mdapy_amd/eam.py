"""Embedded-atom-method calculator — the drop-in for ``mdapy.eam.EAM`` (src/mdapy/eam.py:70-494): reads a LAMMPS ``eam/alloy``
(setfl) file and computes per-atom energies, forces and virials and the stress of a frame on the GPU.

    system.calc = EAM("Cu.eam.alloy")
    system.get_energies(); system.get_force(); system.get_virials(); system.get_stress(); system.get_energy()

The calculation runs over a cutoff list of reach ``rc`` from the System's own machinery: the list the System remembers when it
reaches at least that far (the kernels skip entries with ``dist > rc``), a new one otherwise; the replica of a box thinner than
two cutoffs, with the results cut to the N real atoms; the cell-sorted twin of a frame that came in no spatial order, with the
results back in the caller's order.  One calculation fills all four entries of ``results``, numpy f64 in the caller's atom order:
``energies`` (N,), ``forces`` (N, 3), ``virials`` (N, 9) and ``stress`` (6,), Voigt order [xx, yy, zz, yz, xz, xy] in eV/A^3.

Two things differ from the reference:

* **the list's width.**  The reference builds its list with ``max_neigh=200``; here the library chooses the width.  The results
  are the same whenever no atom has more than 200 neighbours within ``rc`` (where one has, the reference's build raises).
* **the stress** is ``-(V + V^T) / (2 volume)`` with V the sum of the REAL atoms' virials — added on the device in a fixed
  two-level order, no atomics, so two runs give the same bits — over the real box's volume.  The reference sums the replica's
  virials and divides by the replica's volume: the same number to rounding.

``EAMAverage``, ``EAMGenerator`` and ``plot`` of the reference are not here."""
import gzip

import numpy as np

from . import kernels, policy
from .atomic_temperature import STANDARD_ATOMIC_WEIGHT
from .calculator import CalculatorMP
from .devarray import HArray, as_numpy, empty, mark_frozen
from .parallel import get_num_threads


class EAM(CalculatorMP):
    def __init__(self, filename, mass_list=None):
        self.filename = filename
        self.results = {}
        self._read_eam_alloy()
        if mass_list is None:
            mass_list = [STANDARD_ATOMIC_WEIGHT.get(name, 0.0) for name in self.elements_list]
        else:
            assert len(mass_list) == len(self.elements_list)
        self.mass_list = mass_list
        self._types = None  # (an element column, its atoms' types)
        self._shim = None  # (kernels.eam as it was, its EAM object): the spline tables are made once, at the first calculation

    def _read_eam_alloy(self):
        """the setfl layout as the reference reads it (src/mdapy/eam.py:141-219): three comment lines, the element line, the grid
        line, then per element one line of its own and the tables F(rho) and rho(r), then r phi(r) for every pair j <= i.  Every table
        starts on a line of its own, and what is left on the line a table ends on is discarded, as the LAMMPS reader does; ``#``
        starts a comment.  A name ending in ``.gz`` is read through gzip."""
        source = gzip.open if str(self.filename).endswith(".gz") else open
        with source(self.filename, "rt") as f:
            lines = f.readlines()
        self.header = lines[:3]
        words = lines[3].split()
        self.Nelements = count = int(words[0])
        self.elements_list = words[1:count + 1]
        nrho, drho, nr, dr, rc = lines[4].split()[:5]
        self.nrho, self.nr = int(nrho), int(nr)
        self.drho, self.dr, self.rc = float(drho), float(dr), float(rc)
        self.r, self.rho = self.dr * np.arange(self.nr), self.drho * np.arange(self.nrho)
        cursor = [5]  # the line the next table starts on

        def table(size):
            values = []
            while len(values) < size:
                if cursor[0] >= len(lines):
                    raise ValueError(f"EAM file '{self.filename}' ended while expecting {size} values (got {len(values)}).")
                for word in lines[cursor[0]].partition("#")[0].split():
                    try:
                        values.append(float(word))
                    except ValueError:
                        break
                    if len(values) == size:
                        break
                cursor[0] += 1
            return values

        self.F_rho, self.rho_r = np.zeros((count, self.nrho)), np.zeros((count, self.nr))
        for k in range(count):
            cursor[0] += 1  # (the element's own line: atomic number, mass, lattice)
            self.F_rho[k] = table(self.nrho)
            self.rho_r[k] = table(self.nr)
        self._rphi_r = np.zeros((count, count, self.nr))  # r phi, stored for j <= i and mirrored
        for i in range(count):
            for j in range(i + 1):
                self._rphi_r[i, j] = self._rphi_r[j, i] = table(self.nr)
        self.phi_r = np.empty_like(self._rphi_r)
        self.phi_r[..., 1:] = self._rphi_r[..., 1:] / self.r[1:]
        self.phi_r[..., 0] = self.phi_r[..., 1]

    def write_eam_alloy(self, output_name=None):
        """the reference's layout (src/mdapy/eam.py:221-289): its five head lines, then every table as ``.16E`` numbers, five to a
        line.  Every table starts a line of its own.  (The reference lets one pair's table run on in the line the last one ended in;
        when ``nr`` is no multiple of five its own reader, which drops what is left on a section's last line, then loses values.
        With a multiple of five the two files hold the same numbers in the same lines.)"""
        if output_name is None:
            output_name = "".join(self.elements_list) + ".new.eam.alloy"

        def table(values):
            rows = (values[k:k + 5] for k in range(0, len(values), 5))
            return "".join(" " + "".join(f"{v:.16E} " for v in row) + "\n" for row in rows)

        names = " ".join(self.elements_list)
        parts = [f" eam/alloy {self.Nelements} {names}\n", " Generated by mdapy!\n", "\n", f"    {self.Nelements} {names} \n",
                 f" {self.nrho} {self.drho} {self.nr} {self.dr} {self.rc}\n"]
        for i in range(self.Nelements):
            parts += [f" 0 {self.mass_list[i]} 0 dummy\n", table(self.F_rho[i]), table(self.rho_r[i])]
        for i in range(self.Nelements):
            for j in range(i + 1):
                parts.append(table(self._rphi_r[i, j]))
        with open(output_name, "w") as f:
            f.write("".join(parts))

    # ------------------------------------------------------------------ results, cached (src/mdapy/eam.py:291-395)
    def _result(self, name, data, box):
        """one of the four results: from ``results`` when it is there, after one ``_calculate`` (which fills all four) otherwise"""
        if name not in self.results:
            self._calculate(data, box)
        return self.results[name]

    def get_energies(self, data, box):
        return self._result("energies", data, box)

    def get_energy(self, data, box):
        return self._result("energies", data, box).sum()

    def get_forces(self, data, box):
        return self._result("forces", data, box)

    def get_stress(self, data, box):
        return self._result("stress", data, box)

    def get_virials(self, data, box):
        return self._result("virials", data, box)

    # ------------------------------------------------------------------ the calculation
    def _checked(self, data):
        """the reference's assertions (src/mdapy/eam.py:435-448), and every atom's type: its element's place in the FILE's list, not in
        the sorted one.  The types of a frame's element column are kept while that column lives (frame columns never change), read-only,
        so that their copy in HBM is kept too: the next calculation on the same atoms codes nothing and uploads nothing"""
        for name in ("x", "y", "z", "element"):
            assert name in data.columns, f"Required column '{name}' not found in data."
        column = data["element"]
        held = self._types
        if held is not None and held[0] is column:
            return held[1]
        names, codes = policy.label_codes(column.to_numpy())
        for name in names:
            assert name in self.elements_list, f"{name} not in current EAM potential supported elements: {self.elements_list}."
        types = np.array([self.elements_list.index(name) for name in names], np.int32)[as_numpy(codes)]
        types.setflags(write=False)
        self._types = (column, mark_frozen(types))
        return types

    def _calculate(self, data, box):
        """(data, box) of nobody's System: one is made for the list (``System.get_*`` hand themselves to ``_calculate_on``)"""
        from .frame import Frame
        from .system import System

        data = Frame.from_any(data)
        self._checked(data)
        self._calculate_on(System(data=data, box=box))

    def _calculate_on(self, system):
        """fill ``results`` for ``system``'s frame, over the list it remembers or builds"""
        self._to_results(system, *self._run_kernels(system))

    def _calculate_device(self, system, virial_sum=None):
        """the array-level door (what ``FIRE`` looks for): the kernels run as for ``_calculate_on`` and everything stays where they
        left it.  -> (forces (N, 3) in the caller's atom order, cut to the N real atoms; the nine virial sums — ``virial_sum`` itself
        when one is handed in; what ``_to_results`` turns into ``results``).  A replica's real atoms are its leading rows; a twin's rows
        go back through its permutation where they are."""
        raw = self._run_kernels(system, virial_sum)
        force, perm, real = raw[1], raw[4], raw[5]
        if perm is not None:
            back = empty((real, 3), np.float64)
            kernels.fire.scatter_rows(force, perm, back)
            force = back
        elif int(force.shape[0]) != real:
            force = force.head(real) if isinstance(force, HArray) else force[:real]
        return force, raw[3], raw

    def _run_kernels(self, system, total=None):
        """the first half of a calculation: the list, the replica or the twin, and the kernels.  -> (energies, forces, virials — one row
        per atom the list was built on, in its order —, the nine virial sums of the real atoms, the twin's permutation or None, N)"""
        types = self._checked(system.data)
        shim = self._shim
        if shim is None or shim[0] is not kernels.eam:
            shim = self._shim = (kernels.eam, kernels.eam.EAM(self.rc, self.dr, self.drho, self.F_rho, self.rho_r, self._rphi_r))
        system._require_cutoff_list(self.rc, None)
        real = system.N
        twin = system._listed_on_twin()
        if twin is not None:  # the list lives on the cell-sorted twin: its rows, its positions, the types through its permutation
            perm = twin._perm
            rows, dist, counts = twin.verlet_list, twin.distance_list, twin.neighbor_number
            cell, cols = system.box, policy.positions(twin.data)
            types = kernels.order.permute(types, perm)
        else:
            perm = None
            rows, dist, counts = system.verlet_list, system.distance_list, system.neighbor_number
            cell, frame = system._get_compute_view()
            cols = policy.positions(frame)
            if frame.shape[0] != real:  # the replica of a thin box: its atoms carry their originals' elements
                types = self._checked(frame)
        atoms = int(rows.shape[0])
        energy, force, virial = empty(atoms, np.float64), empty((atoms, 3), np.float64), empty((atoms, 9), np.float64)
        if total is None:
            total = empty(9, np.float64)
        shim[1].calculate(*cols, types, cell.box, cell.origin, cell.boundary, rows, dist, counts, force, virial, energy, get_num_threads(),
                          accumulate=False, n_real=real, virial_sum=total)
        return energy, force, virial, total, perm, real

    def _to_results(self, system, energy, force, virial, total, perm, real):
        """the second half: what the kernels left, as ``results`` — numpy, the caller's atom order, the N real atoms"""
        atoms = int(energy.shape[0])
        # (the host copies the arrays in HBM hand out are read-only; only a replica's are cut, and so copied)
        out = [as_numpy(a) if atoms == real else np.array(as_numpy(a)[:real]) for a in (energy, force, virial)]
        if perm is not None:  # row p of the twin is atom perm[p] of the caller
            where = as_numpy(perm)
            for k, a in enumerate(out):
                back = np.empty_like(a)
                back[where] = a
                out[k] = back
        self.results["energies"], self.results["forces"], self.results["virials"] = out
        self.results["stress"] = self._stress_of_sums(as_numpy(total), system.box.volume)

    @staticmethod
    def _stress_of_sums(total, volume):
        """the Voigt stress from the nine virial sums of the real atoms and the real box's volume"""
        v = np.array(total, np.float64).reshape(3, 3)
        stress = (-0.5 * (v + v.T) / volume).ravel()
        return stress[[0, 4, 8, 5, 2, 1]]
