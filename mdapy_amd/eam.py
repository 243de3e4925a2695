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

from . import kernels
from .atomic_temperature import STANDARD_ATOMIC_WEIGHT
from ._list_calculator import ListCalculator


class EAM(ListCalculator):
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

    # ------------------------------------------------------------------ the calculation (the getters, the list, the replica and the
    # twin, ``results``: _list_calculator.py; src/mdapy/eam.py:291-494)
    def _element_list(self):
        return self.elements_list

    def _unknown_element(self, name):
        return f"{name} not in current EAM potential supported elements: {self.elements_list}."

    def _launch(self, cols, types, cell, rows, dist, counts, energy, force, virial, real, total, threads, more):
        shim = self._shim
        if shim is None or shim[0] is not kernels.eam:
            shim = self._shim = (kernels.eam, kernels.eam.EAM(self.rc, self.dr, self.drho, self.F_rho, self.rho_r, self._rphi_r))
        shim[1].calculate(*cols, types, cell.box, cell.origin, cell.boundary, rows, dist, counts, force, virial, energy, threads,
                          accumulate=False, n_real=real, virial_sum=total)
