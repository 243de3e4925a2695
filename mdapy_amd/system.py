"""``System`` — the user-facing object of the hot path, with the surface of ``mdapy.System`` (src/mdapy/system.py) above
the neighbor list and the per-atom structural analyses.

A system is a frame of per-atom columns plus a box.  It remembers ONE neighbor list at a time — ``verlet_list``,
``distance_list``, ``neighbor_number`` and, for a cutoff list, its ``rc`` (system.py:1155-1166) — and, when that list
was built on a replica of a thin periodic box, the replica (``_enlarge_data`` / ``_enlarge_box``) its indices refer to.
Assigning a box or replacing the data with ``reset_neighbor=True`` forgets the list (system.py:232-245, 748-763).

Every ``cal_*`` method first makes sure a suitable list exists, following the reference's reuse rules (SURVEY.md 3,
Appendix C), then runs its analysis class and stores the first N rows of the result as columns of ``data`` or returns
the result object.  The reuse rules are three helpers here — ``_require_cutoff_list``, ``_nearest_prefix`` and
``_borrow_nearest`` — instead of being restated in every method.

The lists stay in HBM between calls (:class:`mdapy_amd.devarray.HArray`) and turn into numpy on first host access.
"""
import functools
import os
import re
import warnings
import weakref

import numpy as np

from . import kernels
from . import policy
from . import tool_function as tool
from .ackland_jones_analysis import AcklandJonesAnalysis
from .angular_distribution_function import AngularDistributionFunction
from .atomic_temperature import AtomicTemperature
from .bond_analysis import BondAnalysis
from .box import Box
from .calculator import CalculatorMP
from .centro_symmetry_parameter import CentroSymmetryParameter
from .chill_plus import ChillPlus
from .cluster_analysis import ClusterAnalysis
from .common_neighbor_analysis import CommonNeighborAnalysis
from .common_neighbor_parameter import CommonNeighborParameter
from .devarray import HArray, as_numpy, full, have_gpu, torch
from .frame import Frame
from .identify_diamond_structure import IdentifyDiamondStructure
from .identify_fcc_planar_faults import IdentifyFccPlanarFaults
from .knn import NearestNeighbor
from .neighbor import Neighbor
from .parallel import get_num_threads
from .polyhedral_template_matching import PolyhedralTemplateMatching
from .radial_distribution_function import RadialDistributionFunction
from .steinhardt_bond_orientation import SteinhardtBondOrientation
from .structure_entropy import StructureEntropy
from .structure_factor import StructureFactor
from ._twin import SORT_FAR_FRACTION, Twin, adf_reach  # noqa: F401 (the threshold stays importable from here)
from .vdw_radii import vdw_radius
from .voronoi import Voronoi
from .warren_cowley_parameter import WarrenCowleyParameter

_REPLICA = ("_enlarge_box", "_enlarge_data")
# ("bond": indices into the atoms the list was built on — whatever forgets the list forgets the bonds)
_LIST = ("verlet_list", "neighbor_number", "distance_list", "rc", "_sorted_columns", "_list_cutoff", "bond") + _REPLICA
_NAMES = {}  # method -> its positional parameter names (filled by _on_twin; what System._twin_for reads a call's arguments by)


def _on_twin(method):
    """run a System method on the cell-sorted twin (_twin.py) when there is one and the call's arguments allow it"""
    name, code = method.__name__, method.__code__
    _NAMES[name] = code.co_varnames[1:code.co_argcount]  # (taken from the function, once)

    @functools.wraps(method)
    def call(self, *args, **kwargs):
        twin = self._twin_for(name, args, kwargs)
        return method(self, *args, **kwargs) if twin is None else self._run_on_twin(twin, name, args, kwargs)

    return call


def _parse_formula(formula):
    """{element: count} of a molecular formula: the reference's pattern, an element symbol and an optional count, as often as
    it occurs (system.py:2668-2679) — "CH3OH" is {"C": 1, "H": 4, "O": 1}; what does not match the pattern is skipped"""
    parts = {}
    for name, count in re.findall(r"([A-Z][a-z]?)(\d*)", formula):
        parts[name] = parts.get(name, 0) + (int(count) if count else 1)
    return parts


def _normalize_bond_cutoff(rc, data):
    """(largest cutoff, compact type of every atom (int32, 0 .. ntype - 1), (ntype, ntype) cutoff matrix) of a bond cutoff
    given as one number, as a dict per pair of types or of elements, or as a matrix over the sorted distinct types
    (system.py:1266-1331)"""
    if np.isscalar(rc):
        rc = float(rc)
        assert rc > 0, "rc should be larger than 0."
        return rc, np.zeros(data.shape[0], np.int32), np.array([[rc]], float)
    if isinstance(rc, dict):
        assert len(rc) > 0, "pairwise rc should not be empty."
        first = next(iter(rc))
        assert len(first) == 2, "pairwise rc key should have two entries."
        by_element = isinstance(first[0], str)
        if by_element:
            assert "element" in data.columns, "Data must contain element column for element-pair bond cutoff."
        else:
            assert "type" in data.columns, "Data must contain type column for type-pair bond cutoff."
        # (np.unique + searchsorted: the sorted distinct labels and every atom's place among them — cached per column)
        present, compact = policy.label_codes(data["element" if by_element else "type"].to_numpy())
        ntype = len(present)
        where = {label: k for k, label in enumerate(present)}
        matrix = np.full((ntype, ntype), -1.0, float)
        for pair, cutoff in rc.items():
            assert len(pair) == 2, "pairwise rc key should have two type indices."
            a, b = pair
            assert a in where and b in where, f"type/element pair {(a, b)} is not in current system."
            cutoff = float(cutoff)
            assert cutoff > 0, "pairwise rc should be larger than 0."
            matrix[where[a], where[b]] = matrix[where[b], where[a]] = cutoff
        if np.any(matrix < 0):
            missing = [(present[a], present[b]) for a in range(ntype) for b in range(a, ntype) if matrix[a, b] < 0]
            raise ValueError(f"Missing rc for type pairs: {missing}")
    else:
        assert "type" in data.columns, "Data must contain type column for matrix bond cutoff."
        present, compact = policy.label_codes(data["type"].to_numpy())
        ntype = len(present)
        matrix = np.asarray(rc, float)
        assert matrix.ndim == 2, "pairwise rc should be a 2D array."
        assert matrix.shape == (ntype, ntype), f"pairwise rc shape should be {(ntype, ntype)}."
        assert np.all(matrix > 0), "pairwise rc should be larger than 0."
    return float(matrix.max()), compact, matrix


def _group_rows(rows):
    """``np.unique(rows, axis=0, return_counts=True)`` of a table of non-negative ints.  A row is first folded into one int64
    (its entries as digits, the first the most significant: the same order) where that fits, because numpy sorts the rows of a
    2-D array as records — 0.6 s for the 1.3 M molecules of 4 M water atoms, 40 ms as one column of integers."""
    span = [int(v) + 1 for v in rows.max(axis=0)]
    weight, total = [], 1
    for v in reversed(span):
        weight.append(total)
        total *= v
    if rows.min() < 0 or total >= (1 << 62):
        return np.unique(rows, axis=0, return_counts=True)
    folded = rows.astype(np.int64) @ np.array(weight[::-1], np.int64)
    _, first, counts = np.unique(folded, return_index=True, return_counts=True)
    return rows[first], counts


def _position_columns(xyz):
    """x, y, z columns of an (N, 3) array.  With a GPU the array crosses PCIe once, as it is, and is split into columns in HBM
    (the columns' host copies are made if somebody asks for them): the three strided host copies of the reference's
    pos[:, k] pattern were 70 of the 90 ms a 10 M-atom numpy-in / labels-out call took."""
    if have_gpu() and xyz.shape[0] >= (1 << 16):
        t = torch()
        with warnings.catch_warnings():
            warnings.simplefilter("ignore")  # (a read-only source array: the tensor is only read)
            dev = t.from_numpy(np.ascontiguousarray(xyz)).to("cuda")
        cols = dev.t().contiguous()  # one transposing pass on the device
        return {name: HArray(cols[k]) for k, name in enumerate("xyz")}
    return dict(zip("xyz", xyz.T))


def _from_ase(atoms):
    """frame and box of an ASE ``Atoms`` (load_save.py:508-545): cell rows, ``pbc``, positions, chemical symbols.  Duck-typed:
    ase itself is not needed, only the four getters the reference calls."""
    for needed in ("get_cell", "get_pbc", "get_positions", "get_chemical_symbols"):
        if not hasattr(atoms, needed):
            raise TypeError("Only accept an ASE Atoms object")
    cell = Box(np.array(atoms.get_cell(), dtype=np.float64), [1 if p else 0 for p in atoms.get_pbc()])
    xyz = np.asarray(atoms.get_positions(), dtype=np.float64)
    cols = _position_columns(xyz)
    cols["element"] = np.array(atoms.get_chemical_symbols())
    return Frame(cols), cell


def _from_ovito(collection):
    """frame, box and attributes of an OVITO ``DataCollection`` (load_save.py:413-505): the 3x4 cell transposed (vectors + origin),
    ``Position`` -> x y z, ``Particle Type`` -> type, ``Particle Identifier`` -> id, ``Velocity`` / ``Force`` -> three columns,
    ``Velocity Magnitude`` dropped, every other property under its name without blanks (vectors as name_0, name_1, ...);
    an ``element`` column when every particle type carries a name.  Duck-typed: ``.cell`` (array-like with ``.pbc``),
    ``.particles`` (mapping), ``.attributes`` (mapping)."""
    for needed in ("cell", "particles", "attributes"):
        if not hasattr(collection, needed):
            raise TypeError("Only accept an Ovito DataCollection object")
    # the whole 3x4 cell transposed: rows 0-2 the vectors, row 3 the origin (load_save.py:443-444)
    cell = Box(np.array(collection.cell[...], dtype=np.float64).T, [1 if p else 0 for p in collection.cell.pbc])
    info = {key: value for key, value in collection.attributes.items()}
    three = {"Position": ("x", "y", "z"), "Velocity": ("vx", "vy", "vz"), "Force": ("fx", "fy", "fz")}
    one = {"Particle Type": "type", "Particle Identifier": "id"}
    cols = {}
    for key in collection.particles.keys():
        values = np.array(collection.particles[key][...])
        if key in three:
            for k, name in enumerate(three[key]):
                cols[name] = np.ascontiguousarray(values[:, k])
        elif key in one:
            cols[one[key]] = values
        elif key == "Velocity Magnitude":
            continue
        else:
            name = "".join(key.split())
            if values.ndim == 1:
                cols[name] = values
            else:
                for k in range(values.shape[1]):
                    cols[f"{name}_{k}"] = np.ascontiguousarray(values[:, k])
    table = getattr(collection.particles, "particle_type", None)
    if table is not None and "type" in cols:
        names = {t.id: t.name for t in table.types}
        if names and all(isinstance(n, str) and len(n) > 0 for n in names.values()):
            cols["element"] = np.array([names[t] for t in cols["type"].tolist()])
    return Frame(cols), cell, info


class System:
    def __init__(self, filename=None, data=None, pos=None, box=None, ase_atom=None, ovito_atom=None, format=None,
                 global_info=None):
        self._info = {}
        self._sort_mode = os.environ.get("MDAPY_SPATIAL_SORT", "")  # (fixed when the system is made: see _spatial)
        if isinstance(filename, str):
            from .load_save import read_file

            self._frame, self.box, self._info = read_file(filename, format)
        elif box is not None and data is not None:
            self._frame = Frame.from_any(data)
            for name in ("x", "y", "z"):
                if name not in self._frame.columns:
                    raise AssertionError(f"data must contain column {name!r}.")
            self.box = box
        elif box is not None and pos is not None:
            xyz = np.asarray(pos, dtype=np.float64)
            if xyz.ndim != 2 or xyz.shape[1] != 3:
                raise AssertionError("pos must have shape (N, 3).")
            self._frame = Frame(_position_columns(xyz))
            self.box = box
        elif ase_atom is not None:
            self._frame, self.box = _from_ase(ase_atom)
        elif ovito_atom is not None:
            self._frame, self.box, self._info = _from_ovito(ovito_atom)
        else:
            raise RuntimeError("One must at least provide filename or [data, box] or [pos, box] or ase_atom or ovito_atom.")
        if global_info is not None and not self._info:
            self._info = dict(global_info)

    # ---------------------------------------------------------------- state
    def _forget(self, names):
        for name in names:
            self.__dict__.pop(name, None)
        if "verlet_list" in names and self._twin is not None:  # the list is gone: the twin's too, and what mirrored it
            self._twin.forget_lists()

    def _forget_list(self):
        self._forget(_LIST)

    # ------------------------------------------------------- the cell-sorted twin: all but these doors is in _twin.py
    _twin = None     # not decided yet; then a Twin — whose `system` is None where these columns and this box get none
    _twin_of = None  # on the sorted System of a Twin (which gets no twin of its own): a weak reference back to it
    _perm = property(lambda self: self._twin_of and self._twin_of().perm)  # (of a sorted System: its row p is atom perm[p] of the owner)

    def _spatial(self):
        """the twin — the sorted System of `_twin` — made on first use; None: this system is analysed in the order it has"""
        if self._twin_of is not None or self._sort_mode == "0":
            return None
        twin, mine = self._twin, (self._frame["x"], self._frame["y"], self._frame["z"], self._cell)
        if twin is None or any(a is not b for a, b in zip(twin.made_from, mine)):
            twin = self._twin = Twin(self)
        return twin.system

    def _mirrors_twin(self):
        """whether the list this system remembers is the twin's list, translated, rows in the twin's order (Twin.mirrors)"""
        return self._twin is not None and self._twin.mirrors(self)

    def _listed_on_twin(self):
        """the twin, when the list this system remembers is the twin's list, translated and in step, and the twin still has it"""
        return self._twin.system if self._twin is not None and self._twin.listed(self) else None

    def _twin_for(self, name, args, kwargs):
        """the twin if method ``name`` may run on it with these arguments (only what the caller passed is bound: no defaults)"""
        twin = self._spatial()
        return twin if twin is not None and self._twin.may_run(self, name, dict(zip(_NAMES.get(name, ()), args), **kwargs)) else None

    def _run_on_twin(self, twin, name, args, kwargs):
        """the one path every call on the twin takes"""
        return self._twin.run(self, name, args, kwargs)

    @property
    def box(self):
        return self._cell

    @box.setter
    def box(self, value):
        # Cartesian coordinates stay as they are; everything computed with the old box is gone
        self._cell = value if isinstance(value, Box) else Box(value)
        self._forget_list()

    data = property(lambda self: self._frame)
    global_info = property(lambda self: self._info)
    N = property(lambda self: self._frame.shape[0])

    def __repr__(self):
        return f"Atom Number: {self.N}\n{self.box}\nParticle Information:\n{self.data}"

    def update_data(self, data, reset_calculator=False, reset_neighbor=False, reset_calcolator=None):
        """replace the per-atom frame; ``reset_neighbor`` also forgets the neighbor list, ``reset_calculator`` clears what the
        attached calculator has cached (system.py:746-747).  ``reset_calcolator`` is the reference's deprecated misspelling of
        ``reset_calculator`` (system.py:686-744), accepted with the same warning."""
        if reset_calcolator is not None:
            warnings.warn("`reset_calcolator` is a misspelling and is deprecated; use `reset_calculator` instead.",
                          DeprecationWarning, stacklevel=2)
            reset_calculator = reset_calculator or reset_calcolator
        self._frame = Frame.from_any(data)
        if reset_calculator and isinstance(self.calc, CalculatorMP):
            self.calc.results = {}
        if reset_neighbor:
            self._forget_list()

    # ------------------------------------------------------- the calculator (src/mdapy/system.py:247-258, 560-684)
    _calc = None

    @property
    def calc(self):
        return self._calc

    @calc.setter
    def calc(self, value):
        assert isinstance(value, CalculatorMP), f"calc must be CalculatorMP, instead of {type(value).__name__}"
        value.results = {}
        self._calc = value

    def _calculated(self, getter):
        """what the calculator's ``getter`` says of this frame.  A calculator that works over a neighbour list (``_calculate_on``:
        EAM) is handed the System itself first, so that it uses the list the System remembers or builds — its replica, its twin."""
        assert isinstance(self.calc, CalculatorMP), "Must assign a calc first."
        if not self.calc.results and hasattr(self.calc, "_calculate_on"):
            self.calc._calculate_on(self)
        return getattr(self.calc, getter)(self.data, self.box)

    def get_energy(self):
        return self._calculated("get_energy")

    def get_energies(self):
        return self._calculated("get_energies")

    def get_force(self):
        return self._calculated("get_forces")

    def get_stress(self):
        return self._calculated("get_stress")

    def get_virials(self):
        return self._calculated("get_virials")

    def _get_compute_view(self):
        """(box, frame) the remembered list's indices refer to: the replica if there is one"""
        if "_enlarge_data" in self.__dict__:
            return self._enlarge_box, self._enlarge_data
        return self.box, self.data

    def _store(self, **columns):
        """results of an analysis over the compute view -> columns of the N real atoms"""
        n = self.N
        kept = {name: (values.head(n) if isinstance(values, HArray) and values.ndim == 1 else as_numpy(values)[:n])
                for name, values in columns.items()}  # results that are in HBM stay there until somebody reads them
        self.update_data(self._frame.with_columns(**kept))

    def wrap_pos(self):
        self.update_data(tool.wrap_pos(self._frame, self.box), reset_neighbor=True)

    # ---- small host helpers of the reference's System (src/mdapy/system.py:333-500, 786-850, 1414-1490): no kernel behind them
    def set_element(self, element):
        """element names: one string for every atom, or one name per atom (system.py:333-364)"""
        if isinstance(element, str):
            names = np.full(self.N, element, dtype=object)
        else:
            assert len(element) == self.N, f"Length of element ({len(element)}) must equal the atom number ({self.N})."
            names = np.array(element, dtype=object)
        self.update_data(self._frame.with_columns(element=names), True)

    def set_type_by_element(self, element_list):
        """column ``type`` = 1-based position of an atom's element in ``element_list`` (system.py:379-431)"""
        assert "element" in self.data.columns, "Data must contain element column."
        names = self.data["element"].to_numpy()
        order = {name: k for k, name in enumerate(element_list, start=1)}
        for name in np.unique(names):
            assert name in order, f"element_list must include element {name!r} (seen in data['element'])."
        present, codes = policy.label_codes(names)
        lut = np.array([order[name] for name in present], dtype=np.int32)
        self.update_data(self._frame.with_columns(type=lut[np.asarray(codes)]), True)

    def get_positions(self, reduced=False):
        """frame of x, y, z — or, reduced, of r_x, r_y, r_z = positions @ inverse box (system.py:433-477; like the reference the
        origin is not subtracted)"""
        if not reduced:
            return self.data.select("x", "y", "z")
        inv = self.box.inverse_box
        x, y, z = (self.data[c].to_numpy() for c in ("x", "y", "z"))
        return Frame({"r_x": x * inv[0, 0] + y * inv[1, 0] + z * inv[2, 0], "r_y": x * inv[0, 1] + y * inv[1, 1] + z * inv[2, 1],
                      "r_z": x * inv[0, 2] + y * inv[1, 2] + z * inv[2, 2]})

    def get_velocities(self):
        for name in ("vx", "vy", "vz"):
            assert name in self.data.columns
        return self.data.select("vx", "vy", "vz")

    def update_box(self, box, scale_pos=False):
        """a new box; ``scale_pos`` moves the atoms affinely with it (system.py:786-846: all three axes periodic)"""
        new_box = box if isinstance(box, Box) else Box(box)
        if scale_pos:
            assert sum(new_box.boundary) == 3, "only support all periodic boundary condition."
            m = np.linalg.solve(self.box.box, new_box.box)
            x, y, z = (self.data[c].to_numpy() - self.box.origin[k] for k, c in enumerate(("x", "y", "z")))
            self._frame = self._frame.with_columns(x=x * m[0, 0] + y * m[1, 0] + z * m[2, 0] + new_box.origin[0],
                                                   y=x * m[0, 1] + y * m[1, 1] + z * m[2, 1] + new_box.origin[1],
                                                   z=x * m[0, 2] + y * m[1, 2] + z * m[2, 2] + new_box.origin[2])
        self.box = new_box  # (the setter forgets the neighbor list)

    # ---- the writers (src/mdapy/system.py:939-1107): headers on the host, the atom table formatted where its columns live
    def write_mp(self, output_name):
        from .load_save import write_mp

        write_mp(output_name, self.data, self.box, self.global_info)

    def write_xyz(self, output_name, classical=False, compress=False):
        from .load_save import write_xyz

        write_xyz(output_name, self.data, self.box, classical, compress, **self.global_info)

    def write_poscar(self, output_name, reduced_pos=False, selective_dynamics=False, compress=False):
        from .load_save import write_poscar

        write_poscar(output_name, self.data, self.box, reduced_pos=reduced_pos, selective_dynamics=selective_dynamics, compress=compress)

    def write_data(self, output_name, element_list=None, num_type=None, data_format="atomic", compress=False):
        """with ``element_list`` and an ``element`` column, ``type`` is derived from the list's order for this file alone"""
        from .load_save import write_data

        data = self.data
        if element_list is not None and "element" in data.columns:
            names = data["element"].to_numpy()
            present, codes = policy.label_codes(names)
            for name in present:
                assert name in element_list, f"element_list must include element {name!r}."
            order = {name: k for k, name in enumerate(element_list, start=1)}
            lut = np.array([order[name] for name in present], dtype=np.int32)
            data = data.with_columns(type=lut[np.asarray(codes)])
        write_data(output_name, data, self.box, element_list=element_list, num_type=num_type, data_format=data_format, compress=compress)

    def write_dump(self, output_name, timestep=0, compress=False):
        from .load_save import write_dump

        write_dump(output_name, self.data, self.box, timestep=timestep, compress=compress)

    def delete_overlap(self, rc, max_neigh=None):
        """remove every atom that has a SURVIVING neighbour of smaller index closer than ``rc``; returns how many went
        (system.py:1414-1490: a sweep in index order).  The sweep's answer is the unique solution of
        gone[j] = any(not gone[i] for the neighbours i < j within rc); it is reached here by repeating that rule over all
        atoms at once until nothing changes (a chain of k overlapping atoms takes k rounds)."""
        rc = float(rc)
        assert rc > 0, "rc should be larger than 0."
        n = self.N
        if not (hasattr(self, "rc") and self.rc >= rc):
            self.build_neighbor(rc, max_neigh)
        rows, dist = as_numpy(self.verlet_list), as_numpy(self.distance_list)
        if "_enlarge_data" in self.__dict__:
            rows = np.where(rows >= 0, rows % n, -1)  # replica indices back to the atoms they copy
        rows, dist = rows[:n], dist[:n]
        own = np.arange(n)[:, None]
        smaller = (rows >= 0) & (rows < own) & (dist < rc)
        gone = np.zeros(n, dtype=bool)
        cols = np.where(smaller, rows, 0)
        while True:
            nxt = (smaller & ~gone[cols]).any(axis=1)
            if np.array_equal(nxt, gone):
                break
            gone = nxt
        removed = int(gone.sum())
        if removed:
            self.update_data(self.data.filter(~gone), reset_calculator=True, reset_neighbor=True)
        return removed

    def replicate(self, nx, ny, nz):
        self._frame, self.box = tool.replicate(self._frame, self.box, nx, ny, nz)

    # ------------------------------------------------------- neighbor lists
    def _remember(self, search, rows, distances, counts, front=0):
        """take over the list a search object built, and its replica if it made one (the replica always belongs to the
        list that is current: one left behind by an earlier search would be paired with rows it does not describe)"""
        self._forget(_REPLICA + ("bond",))  # (and the bonds that were read from the list this one replaces)
        for name in _REPLICA:
            if name in search.__dict__:
                setattr(self, name, getattr(search, name))
        self.verlet_list, self.distance_list, self.neighbor_number = rows, distances, counts
        self._sorted_columns = (weakref.ref(rows), front)  # (THIS list object, weakly; its leading columns known to hold the nearest in order)

    def _front(self):
        """how many leading columns of the CURRENT list are known to hold the nearest neighbours, in order; -1: nothing known"""
        which, done = self.__dict__.get("_sorted_columns", (None, -1))
        rows = which() if which is not None else None
        return done if rows is not None and rows is self.__dict__.get("verlet_list") else -1

    def _sort_front(self, k):
        """the k nearest of every row to the front, nearest first — once: a row prefix that is already in order (the rows of a
        k-nearest search, or an earlier call) is not touched again"""
        if self._front() < k:
            twin = self._listed_on_twin()
            if twin is not None:
                # the list is the twin's, translated: sort the twin's rows and mirror them again, so that the two stay in step and
                # later analyses keep running on the twin (the selection looks at distances and slots, not at what the entries
                # are called: the twin's sorted rows, translated, are this system's rows, sorted)
                twin._sort_front(k)
                self._twin.mirror_lists(self)
                return
            tool.sort_neighbor(self.verlet_list, self.distance_list, self.neighbor_number, k)
            self._sorted_columns = (weakref.ref(self.verlet_list), k)

    @_on_twin
    def build_neighbor(self, rc, max_neigh=None, _label=False):
        # _label (internal): the fixed-cutoff common-neighbour labels of this cutoff in the same pass; returned, not stored
        search = Neighbor(rc, self.box, self.data, max_neigh, key=self._twin_of().order_key if self._twin_of is not None else None)
        search.compute(label=_label)
        self.rc = rc
        self._remember(search, search.verlet_list, search.distance_list, search.neighbor_number)
        # provenance of the CURRENT list: a cutoff list of exactly this reach, complete (an overflow of max_neigh raises).
        # `rc` alone does not say so — like the reference's, it survives build_nearest_neighbor (system.py:1256-1263)
        self._list_cutoff = float(rc)
        return search.pattern if _label else None

    @_on_twin
    def build_nearest_neighbor(self, k):
        """k nearest neighbours as the current list (no ``rc``; every count is k)"""
        search = NearestNeighbor(self.data, self.box, k)
        search.compute()
        # (the counts live where the rows live: a host array here was 40 MB over PCIe in front of every analysis that takes the list)
        self._remember(search, search.indices_py, search.distances_py, full((search.indices_py.shape[0],), k, np.int32), front=k)
        self._forget(("_list_cutoff",))  # the current list is no cutoff list any more (`rc` stays, as in the reference)

    def _require_cutoff_list(self, rc, max_neigh):
        """a cutoff list reaching at least rc: the remembered one if it does, a new one otherwise"""
        if not ("rc" in self.__dict__ and self.rc >= rc):
            self.build_neighbor(rc, max_neigh)

    def _deep_enough(self, k):
        return "neighbor_number" in self.__dict__ and self.neighbor_number.min() >= k

    def _nearest_prefix(self, k, cutoff_lists_only=False):
        """make the first k columns of the current list the k nearest neighbours, nearest first: by sorting the remembered
        list when every atom has k entries, by a k-nearest search otherwise"""
        if self._deep_enough(k) and (not cutoff_lists_only or "rc" in self.__dict__):
            self._sort_front(k)
        else:
            self.build_nearest_neighbor(k)

    def _safe_repeat(self, safe_L=15):
        return policy.axis_copies(self.box, safe_L)

    def _borrow_nearest(self, k):
        """rows to lend to an analysis that otherwise searches its k nearest neighbours itself: the remembered list,
        sorted, if it is deep enough — but never for a box so thin that the analysis would replicate it (the list of the
        unreplicated system would miss images)"""
        if policy.is_single(self._safe_repeat()) and self._deep_enough(k):
            self._sort_front(k)
            return self.verlet_list
        return None

    # ------------------------------------------------------------- analyses
    @_on_twin
    def cal_common_neighbor_analysis(self, rc=None, max_neigh=None):
        """column ``cna``: 0 other, 1 fcc, 2 hcp, 3 bcc, 4 ico; fixed cutoff ``rc`` or adaptive (None)"""
        rows = counts = None
        if rc is None:
            if "rc" in self.__dict__:  # (only a cutoff list is lent to the adaptive variant)
                rows = self._borrow_nearest(14)
        elif policy.is_single(self._safe_repeat()) and not ("rc" in self.__dict__ and self.rc >= rc):
            # no list that reaches: the reference builds one (it stays the system's list) and labels from it; here the labels
            # are made in the pass that builds the list (mdh_build_neighbor_fcna / _exact_fcna), bit for bit the same
            labels = self.build_neighbor(rc, max_neigh, _label=True)
            if labels is not None:
                self._store(cna=labels)
                return
            rows, counts = self.verlet_list, self.neighbor_number
        elif policy.is_single(self._safe_repeat()) and self.__dict__.get("_list_cutoff") == float(rc):
            # the reference lends nothing here and the analysis builds a list of its own with this very cutoff: the same
            # rows and counts as the CURRENT list when that is a cutoff list of exactly this reach, which is lent instead
            # (one neighbour build less per call).  A stale `rc` beside a k-nearest list lends nothing.
            rows, counts = self.verlet_list, self.neighbor_number
        cell, frame = self._get_compute_view()
        job = CommonNeighborAnalysis(frame, cell, rows, counts, rc)
        job.compute()
        self._store(cna=job.pattern)

    def cal_polyhedral_template_matching(self, structure="fcc-hcp-bcc", rmsd_threshold=0.1, return_ordering=False,
                                         return_rmsd=False, return_atomic_distance=False, return_orientation=False,
                                         identify_fcc_planar_faults=False, identify_esf=True):
        """column ``ptm`` and, on request, ``ordering``, ``rmsd``, ``interatomic_distance``, ``qx qy qz qw``, ``pft``"""
        # the two calls of `_on_twin`, the twin's without the planar-fault sweep (its answer depends on the atom numbering: an index-
        # ordered sweep, identify_fcc_planar_faults.cpp:139-180): that runs here, on the translated labels and template-ordered neighbours
        matching = (structure, rmsd_threshold, return_ordering, return_rmsd, return_atomic_distance, return_orientation, False, identify_esf)
        twin = self._twin_for("cal_polyhedral_template_matching", matching, {})
        if twin is not None:
            self._run_on_twin(twin, "cal_polyhedral_template_matching", matching, {})
            if identify_fcc_planar_faults:
                shell = np.ascontiguousarray(as_numpy(self.ptm_indices)[:, 1:13])
                faults = IdentifyFccPlanarFaults(np.array(self.data["ptm"].to_numpy(), np.int32), shell, identify_esf)
                faults.compute()
                self._store(pft=faults.fault_types)
            return
        rows = self._borrow_nearest(18)
        cell, frame = self._get_compute_view()
        job = PolyhedralTemplateMatching(structure, frame, cell, rmsd_threshold, rows)
        job.compute()
        table = job.output
        if isinstance(table, HArray):  # columns are cut out in HBM; nothing crosses PCIe before it is asked for
            take = table.column
        else:
            take = lambda col, dtype=None: table[:, col] if dtype is None else table[:, col].astype(dtype)
        found = {"ptm": take(0, np.int32)}
        for wanted, name, col in ((return_ordering, "ordering", 1), (return_rmsd, "rmsd", 2),
                                  (return_atomic_distance, "interatomic_distance", 3)):
            if wanted:
                found[name] = take(col)
        if return_orientation:  # stored x, y, z, w; the kernel's quaternion is w, x, y, z
            found.update(qx=take(5), qy=take(6), qz=take(7), qw=take(4))
        self.ptm_indices = job.ptm_indices
        if identify_fcc_planar_faults:
            shell = np.ascontiguousarray(as_numpy(job.ptm_indices)[:, 1:13])  # the 12 neighbours in template order
            faults = IdentifyFccPlanarFaults(np.array(as_numpy(found["ptm"]), np.int32), shell, identify_esf)
            faults.compute()
            found["pft"] = faults.fault_types
        self._store(**found)

    @_on_twin
    def cal_common_neighbor_parameter(self, rc, max_neigh=None):
        """column ``cnp``"""
        self._require_cutoff_list(rc, max_neigh)
        cell, frame = self._get_compute_view()
        job = CommonNeighborParameter(frame, cell, rc, self.verlet_list, self.distance_list, self.neighbor_number)
        job.compute()
        self._store(cnp=job.cnp)

    @_on_twin
    def cal_ackland_jones_analysis(self):
        """column ``aja``: 0 other, 1 fcc, 2 hcp, 3 bcc, 4 ico"""
        depth = 14
        if self.N < depth and int(np.sum(self.box.boundary)) == 0:
            self._store(aja=np.zeros(self.N, np.int32))
            return
        self._nearest_prefix(depth)
        cell, frame = self._get_compute_view()
        job = AcklandJonesAnalysis(frame, cell, self.verlet_list, self.distance_list)
        job.compute()
        self._store(aja=job.aja)

    @_on_twin
    def cal_structure_entropy(self, rc, sigma, use_local_density=False, average_rc=0.0, max_neigh=None):
        """column ``entropy`` (and ``entropy_ave`` when average_rc > 0)"""
        self._require_cutoff_list(rc, max_neigh)
        cell, _ = self._get_compute_view()
        job = StructureEntropy(cell, self.verlet_list, self.distance_list, self.neighbor_number, rc, sigma,
                               use_local_density, average_rc)
        job.compute()
        found = {"entropy": job.entropy}
        if average_rc > 0:
            found["entropy_ave"] = job.entropy_ave
        self._store(**found)

    @_on_twin
    def cal_atomic_temperature(self, rc, factor=1.0, max_neigh=None):
        """column ``atomic_temp`` (K); velocities are A/fs times ``factor``"""
        self._require_cutoff_list(rc, max_neigh)
        job = AtomicTemperature(self._get_compute_view()[1], self.verlet_list, self.distance_list, rc, factor)
        job.compute()
        self._store(atomic_temp=job.T)

    @_on_twin
    def cal_chill_plus(self, cutoff=3.5):
        """column ``chill_plus``: 0 other, 1 hexagonal ice, 2 cubic ice, 3 interfacial ice, 4 gas hydrate, 5 interfacial gas
        hydrate (CHILL+); the system holds the molecule centres only (oxygens or water beads, no hydrogens)"""
        self._require_cutoff_list(cutoff, None)
        cell, frame = self._get_compute_view()
        job = ChillPlus(frame, cell, cutoff, self.verlet_list, self.distance_list, self.neighbor_number)
        job.compute()
        self._store(chill_plus=job.pattern)

    def cal_cluster_analysis(self, rc=5.0, max_neigh=None):
        """column ``cluster_id`` and attribute ``cluster_number``; ``rc`` one number or a dict per type pair"""
        per_pair = isinstance(rc, dict)
        if per_pair:
            reach = max(rc.values())
        elif isinstance(rc, (int, float, np.integer, np.floating)):
            reach = float(rc)
        else:
            raise TypeError("rc should be a positive number, or a dict like {'1-1':1.5, '1-2':1.3}")
        self._require_cutoff_list(reach, max_neigh)
        types = None
        if per_pair:
            if "type" not in self.data.columns:
                raise AssertionError("Must have type for multi rc cluster calculation.")
            # types of the atoms the list indexes, i.e. of the replica when there is one
            types = np.ascontiguousarray(self._get_compute_view()[1]["type"].to_numpy(), dtype=np.int32)
        job = ClusterAnalysis(rc, self.verlet_list, self.distance_list, self.neighbor_number, types)
        job.compute()
        self.cluster_number = job.cluster_number
        self._store(cluster_id=job.particleClusters)

    def create_bonds(self, rc, max_neigh=None):
        """attribute ``bond`` (also returned): the (Nbond, 2) int32 list of bonded pairs i < j, 0-based, in lexicographic order
        (system.py:1333-1412).  ``rc`` is one cutoff, a ``{(type_i, type_j): rc}`` or ``{(element_i, element_j): rc}`` dict, or
        an (ntype, ntype) matrix over the sorted distinct types.  Runs on the remembered list in the caller's atom order (the
        result is indices); a list built on the replica of a thin periodic box names every neighbour by the atom it copies."""
        if np.isscalar(rc):
            reach = float(rc)
        elif isinstance(rc, dict):
            reach = float(np.max(np.asarray(list(rc.values()), float)))
        else:
            assert "type" in self.data.columns, "Data must contain type column for matrix bond cutoff."
            reach = float(np.max(np.asarray(rc, float)))
        assert reach > 0, "rc should be larger than 0."
        self._require_cutoff_list(reach, max_neigh)
        frame = self._get_compute_view()[1]
        _, compact, matrix = _normalize_bond_cutoff(rc, frame)
        if matrix.shape[0] == 1:
            compact = None  # (one type: the kernel needs no type array, and none crosses PCIe)
        bond = kernels.build_bond.build_bond(self.verlet_list, self.distance_list, self.neighbor_number, compact, matrix,
                                             get_num_threads(), self.N if "_enlarge_data" in self.__dict__ else 0)
        self.bond = bond if int(bond.shape[0]) else np.empty((0, 2), np.int32)
        return self.bond

    def cal_chemical_species(self, search_species=None, element_list=None, check_most=10, add_mol_id=False, scale=0.6):
        """``{formula: count}`` of the molecules (system.py:2575-2740).  Two atoms are bonded when their distance is at most
        ``(r_i + r_j) * scale`` with the van der Waals radii of ``vdw_radii``; a molecule is a connected cluster
        (``cal_cluster_analysis``: columns ``type`` — from the sorted distinct elements when there is an ``element`` column —
        and ``cluster_id``).  Without an ``element`` column, ``element_list`` names the elements of types 1, 2, ...

        ``search_species`` (``["H2O", "CO2"]``): the count of each formula, under the caller's spelling and in the caller's
        order, 0 for a formula with an element the system does not have; ``add_mol_id`` adds the column ``mol_id``, the index
        of an atom's molecule in ``search_species`` (the last one where two formulas mean the same), -1 for none.  Counting and
        ``mol_id`` happen on the device (mdh_cluster_composition, mdh_species_match).

        ``search_species=None``: the ``check_most`` most frequent compositions, spelled as the sorted element names, each
        repeated (``"HHO"``).  The (cluster_number, ntype) composition table is brought to the host and grouped there with
        ``np.unique`` — a deliberate host step over a table far smaller than the atoms.  Equal counts go by ascending key (the
        reference leaves that order to polars)."""
        if "element" in self.data.columns:
            present, codes = policy.label_codes(self.data["element"].to_numpy())
            element_list = [str(name) for name in present]
            compact = np.asarray(codes)  # (0-based place among the sorted elements: what the composition kernel reads)
            self.update_data(self._frame.with_columns(type=(compact + 1).astype(np.int32)))
        else:
            assert element_list is not None, "'element_list' must be provided because no 'element' column is present in the data."
            assert "type" in self.data.columns, "'type' column is required when 'element' column is not available."
            most = self.data["type"].max()
            assert len(element_list) >= most, (f"'element_list' must contain at least {most} elements to match "
                                               f"the maximum atom type index ({most}).")
            element_list = [str(name) for name in element_list]
            compact = np.asarray(self.data["type"].to_numpy(), dtype=np.int32) - 1
        radii = [vdw_radius(name) for name in element_list]
        ntype = len(element_list)
        self.cal_cluster_analysis({f"{a + 1}-{b + 1}": (radii[a] + radii[b]) * scale for a in range(ntype) for b in range(a, ntype)},
                                  max_neigh=None)
        cluster_id = self.data["cluster_id"]
        if have_gpu():  # (the column where the kernels read it)
            cluster_id = cluster_id.device_array()
        table = kernels.build_bond.cluster_composition(cluster_id, compact, self.cluster_number, ntype)
        if search_species is not None:
            want = np.full((len(search_species), ntype), -1, np.int32)  # (-1: equals no composition)
            for s, formula in enumerate(search_species):
                parts = _parse_formula(formula)
                if parts and all(name in element_list for name in parts):
                    want[s] = [parts.get(name, 0) for name in element_list]
            counts, mol_id = kernels.build_bond.species_match(table, want, cluster_id if add_mol_id else None)
            if add_mol_id:
                self._store(mol_id=mol_id)
            return {formula: int(counts[s]) for s, formula in enumerate(search_species)}
        rows = as_numpy(table)  # the deliberate host step: (cluster_number, ntype) ints
        rows = rows[rows.any(axis=1)]  # (a list built on a replica has clusters of copies only)
        if rows.shape[0] == 0:
            return {}
        kinds, counts = _group_rows(rows)
        found = sorted((-int(n), "".join(sorted(name for name, k in zip(element_list, kind) for _ in range(int(k)))))
                       for kind, n in zip(kinds, counts))
        return {key: -n for n, key in found[:int(check_most)]}

    def build_voronoi_neighbor(self, a_face_area_threshold=-1.0, r_face_area_threshold=-1.0):
        """``voro_verlet_list``, ``voro_distance_list``, ``voro_face_area``, ``voro_neighbor_number``"""
        cells = Voronoi(self.box, self.data)
        lists = cells.get_neighbor(a_face_area_threshold, r_face_area_threshold)
        self.voro_verlet_list, self.voro_distance_list, self.voro_face_area, self.voro_neighbor_number = lists
        for name in _REPLICA:
            if name in cells.__dict__:
                setattr(self, name, getattr(cells, name))

    def cal_structure_factor(self, k_min, k_max, nbins, cal_partial=False, atomic_form_factors=False, mode="direct",
                             rc=None, nbin_rdf=200, window=False):
        """-> StructureFactor with ``k``, ``Sk``, ``Sk_partial``"""
        job = StructureFactor(self.data, self.box, k_min, k_max, nbins, cal_partial, atomic_form_factors, mode, rc,
                              nbin_rdf, window)
        job.compute()
        return job

    def cal_voronoi_volume(self):
        """columns ``volume``, ``neighbor_number`` (faces of the cell), ``cavity_radius``"""
        volume, faces, radius = Voronoi(self.box, self.data).get_volume()
        self.update_data(self.data.with_columns(volume=volume, neighbor_number=faces, cavity_radius=radius))

    @_on_twin
    def cal_centro_symmetry_parameter(self, N):
        """column ``csp`` from the N nearest neighbours (N even)"""
        if not (N > 0 and N % 2 == 0):
            raise AssertionError(f"N must be a positive even number: {N}.")
        if self.N <= N and int(np.sum(self.box.boundary)) == 0:
            self._store(csp=np.full(self.N, 10000, float))  # an open system with too few atoms: "as asymmetric as it gets"
            return
        self._nearest_prefix(N, cutoff_lists_only=True)
        cell, frame = self._get_compute_view()
        job = CentroSymmetryParameter(frame, cell, N, self.verlet_list)
        job.compute()
        self._store(csp=job.csp)

    def cal_identify_diamond_structure(self):
        """column ``ids``: 0 other, 1 cubic diamond (2, 3 its shells), 4 hexagonal diamond (5, 6 its shells)"""
        rows = self._borrow_nearest(4)
        cell, frame = self._get_compute_view()
        job = IdentifyDiamondStructure(frame, cell, rows)
        job.compute()
        self._store(ids=job.pattern)

    @_on_twin
    def cal_steinhardt_bond_orientation(self, llist, use_voronoi=False, nnn=0, rc=-1.0, average=False, use_weight=False,
                                        weight=None, wl=False, wlhat=False, a_face_area_threshold=-1,
                                        r_face_area_threshold=-1, identify_liquid=False, threshold=0.7, n_bond=7,
                                        max_neigh=None):
        """columns ``ql{l}`` (and ``wl{l}``, ``wlh{l}``, ``solidliquid``, ``nbond`` on request)"""
        if use_voronoi:
            self.build_voronoi_neighbor(a_face_area_threshold, r_face_area_threshold)
            lists = (self.voro_verlet_list, self.voro_distance_list, self.voro_neighbor_number)
            if use_weight and weight is None:
                weight = self.voro_face_area
        else:
            if nnn > 0:
                self._nearest_prefix(nnn)
            else:
                assert rc > 0, "At least use voronoi, or set positive nnn, or positive rc."
                self._require_cutoff_list(rc, max_neigh)
            lists = (self.verlet_list, self.distance_list, self.neighbor_number)
        cell, frame = self._get_compute_view()
        job = SteinhardtBondOrientation(cell, frame, np.asarray(llist, int), nnn, rc, average, use_voronoi, use_weight,
                                        weight, *lists, wl, wlhat, identify_liquid, threshold, n_bond)
        job.compute()
        values = job.qnarray
        take = values.column if isinstance(values, HArray) else (lambda col: values[:, col])
        if values.shape[1] == 1:
            found = {f"ql{llist[0]}": take(0)}
        else:
            names = [f"ql{l}" for l in llist]
            names += [f"wl{l}" for l in llist] if wl else []
            names += [f"wlh{l}" for l in llist] if wlhat else []
            found = {name: take(col) for col, name in enumerate(names)}
        if identify_liquid:
            found.update(solidliquid=job.solidliquid, nbond=job.nbond)
        self._store(**found)

    @_on_twin
    def cal_radial_distribution_function(self, rc, nbin=100, max_neigh=None, streaming=None):
        """-> RadialDistributionFunction (``r``, ``g_total``, ``g_partial``).  ``streaming=None`` decides by itself: a cutoff
        of a third of the thinnest periodic direction or more is counted straight from the positions, without a list"""
        cell, frame = self._get_compute_view()
        if streaming is None:
            spans = [t for t, periodic in zip(cell.get_thickness(), cell.boundary) if periodic]
            streaming = rc >= (min(spans) if spans else float("inf")) / 3.0
        if streaming:
            copies = self.box.check_small_box(rc)
            if not policy.is_single(copies):
                frame, cell = tool.replicate(frame, cell, *copies)
            job = RadialDistributionFunction(rc, nbin, cell, type_list=policy.species_of(frame), streaming=True,
                                             x=frame["x"], y=frame["y"], z=frame["z"])
        else:
            self._require_cutoff_list(rc, max_neigh)
            cell, frame = self._get_compute_view()
            job = RadialDistributionFunction(rc, nbin, cell, verlet_list=self.verlet_list, distance_list=self.distance_list,
                                             neighbor_number=self.neighbor_number, type_list=policy.species_of(frame))
        job.compute()
        return job

    @_on_twin
    def cal_warren_cowley_parameter(self, rc, max_neigh=None):
        """-> WarrenCowleyParameter (``WCP`` matrix)"""
        self._require_cutoff_list(rc, max_neigh)
        job = WarrenCowleyParameter(self.verlet_list, self.neighbor_number, self._get_compute_view()[1])
        job.compute()
        return job

    @_on_twin
    def cal_bond_analysis(self, rc, nbin, max_neigh=None):
        """-> BondAnalysis (``bond_length_distribution``, ``bond_angle_distribution``, ``r_length``, ``r_angle``; int64 counts)"""
        if not float(rc) > 0:
            raise ValueError(f"rc must be positive, got {rc}.")
        if int(nbin) < 1:
            raise ValueError(f"nbin must be at least 1, got {nbin}.")
        self._require_cutoff_list(rc, max_neigh)
        cell, frame = self._get_compute_view()
        job = BondAnalysis(frame, cell, rc, nbin, self.verlet_list, self.distance_list, self.neighbor_number)
        job.compute()
        return job

    @_on_twin
    def cal_angular_distribution_function(self, rc_dict, nbin, max_neigh=None):
        """-> AngularDistributionFunction (``bond_angle_distribution`` npattern x nbin, int64, ``r_angle``).  ``rc_dict`` maps
        ``"A-B-C"`` (A the centre) to ``[rij_min, rij_max, rik_min, rik_max]``"""
        assert "element" in self.data.columns, "Data must contain element column."
        rc = adf_reach(rc_dict)
        if rc is None:
            raise ValueError("rc_dict must map 'A-B-C' patterns to [rij_min, rij_max, rik_min, rik_max].")
        if not rc > 0:
            raise ValueError(f"the largest cutoff of rc_dict must be positive, got {rc}.")
        if int(nbin) < 1:
            raise ValueError(f"nbin must be at least 1, got {nbin}.")
        self._require_cutoff_list(rc, max_neigh)
        cell, frame = self._get_compute_view()
        job = AngularDistributionFunction(frame, cell, rc_dict, nbin, self.verlet_list, self.distance_list, self.neighbor_number)
        job.compute()
        return job

    @_on_twin
    def average_by_neighbor(self, average_rc, property_name, include_self=True, output_name=None, max_neigh=None):
        """column ``<property>_ave`` (or ``output_name``): neighbourhood mean of a column within ``average_rc``"""
        self._require_cutoff_list(average_rc, max_neigh)
        averaged = tool.average_by_neighbor(average_rc, self._get_compute_view()[1], property_name, self.verlet_list, self.distance_list,
                                            self.neighbor_number, include_self, output_name)
        name = f"{property_name}_ave" if output_name is None else output_name
        self._store(**{name: averaged[name].to_numpy()})
