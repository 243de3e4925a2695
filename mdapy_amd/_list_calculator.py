"""What the calculators that run over a cutoff list (``EAM``, ``NEP``) share: the cached getters, the element checks and the types
cached per element column, and the two halves of a calculation — the list the System remembers or builds, its replica or its
cell-sorted twin and the kernels (``_run_kernels``), then ``results`` in the caller's atom order (``_to_results``) — with the
array-level door ``_calculate_device`` that ``FIRE``'s HBM path looks for.

A subclass sets ``rc`` and ``results``, names its elements (``_element_list``), words the two assertions of its reference
(``_missing_column``, ``_unknown_element``) and runs its kernels in ``_launch``."""
import numpy as np

from . import kernels, policy
from .calculator import CalculatorMP
from .devarray import HArray, as_numpy, empty, mark_frozen
from .parallel import get_num_threads


class ListCalculator(CalculatorMP):
    _types = None  # (an element column, its atoms' types)

    # ------------------------------------------------------------------ what a subclass says
    def _element_list(self):
        raise NotImplementedError

    def _missing_column(self, name):
        return f"Required column '{name}' not found in data."

    def _unknown_element(self, name):
        raise NotImplementedError

    def _launch(self, cols, types, cell, rows, dist, counts, energy, force, virial, real, total, threads, more):
        """run the kernels: positions ``cols`` (x, y, z), ``types``, the box ``cell``, the list, the three per-atom outputs (one row
        per atom of the list), the nine virial sums of the first ``real`` rows into ``total``; ``more``: None, or a dict whose keys
        name further outputs the subclass knows and whose values it fills"""
        raise NotImplementedError

    # ------------------------------------------------------------------ results, cached
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
        """the reference's assertions, and every atom's type: its element's place in the FILE's list, not in the sorted one.  The
        types of a frame's element column are kept while that column lives (frame columns never change), read-only, so that their
        copy in HBM is kept too: the next calculation on the same atoms codes nothing and uploads nothing"""
        for name in ("x", "y", "z", "element"):
            assert name in data.columns, self._missing_column(name)
        column = data["element"]
        held = self._types
        if held is not None and held[0] is column:
            return held[1]
        elements = self._element_list()
        names, codes = policy.label_codes(column.to_numpy())
        for name in names:
            assert name in elements, self._unknown_element(name)
        types = np.array([elements.index(name) for name in names], np.int32)[as_numpy(codes)]
        types.setflags(write=False)
        self._types = (column, mark_frozen(types))
        return types

    def _system_of(self, data, box):
        """(data, box) of nobody's System: one is made for the list"""
        from .frame import Frame
        from .system import System

        data = Frame.from_any(data)
        self._checked(data)
        return System(data=data, box=box)

    def _calculate(self, data, box):
        """(``System.get_*`` hand themselves to ``_calculate_on``)"""
        self._calculate_on(self._system_of(data, box))

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

    def _run_kernels(self, system, total=None, more=None):
        """the first half of a calculation: the list, the replica or the twin, and the kernels.  -> (energies, forces, virials — one row
        per atom the list was built on, in its order —, the nine virial sums of the real atoms, the twin's permutation or None, N)"""
        types = self._checked(system.data)
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
        self._launch(cols, types, cell, rows, dist, counts, energy, force, virial, real, total, get_num_threads(), more)
        return energy, force, virial, total, perm, real

    @staticmethod
    def _rows_back(arrays, perm, real):
        """per-atom arrays as the kernels left them -> numpy, the caller's atom order, the N real atoms"""
        # (the host copies the arrays in HBM hand out are read-only; only a replica's are cut, and so copied)
        out = [as_numpy(a) if int(a.shape[0]) == real else np.array(as_numpy(a)[:real]) for a in arrays]
        if perm is not None:  # row p of the twin is atom perm[p] of the caller
            where = as_numpy(perm)
            for k, a in enumerate(out):
                back = np.empty_like(a)
                back[where] = a
                out[k] = back
        return out

    def _to_results(self, system, energy, force, virial, total, perm, real):
        """the second half: what the kernels left, as ``results``"""
        self.results["energies"], self.results["forces"], self.results["virials"] = self._rows_back((energy, force, virial), perm, real)
        self.results["stress"] = self._stress_of_sums(as_numpy(total), system.box.volume)

    @staticmethod
    def _stress_of_sums(total, volume):
        """the Voigt stress from the nine virial sums of the real atoms and the real box's volume"""
        v = np.array(total, np.float64).reshape(3, 3)
        stress = (-0.5 * (v + v.T) / volume).ravel()
        return stress[[0, 4, 8, 5, 2, 1]]
