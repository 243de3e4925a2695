"""The cell-sorted twin of a ``System`` (mdapy_amd/system.py).

The reference's kernels do not care in which order atoms arrive (a linked list per cell, src/neighbor.cpp:64-100); a GPU's gathers
do: on an id-sorted dump of a diffused system, or a shuffled one, a neighbour's position is an HBM access instead of an L2 hit, and
the fixed-cutoff CNA of 10 M such atoms took 6.7 ms instead of 0.54 (profiles/r05_order_sweep.txt).  A large system that was handed
in in no spatial order therefore gets a TWIN: the same atoms in cell order (csrc/order.hip), with every other column read through
the permutation.  List builds and the analyses that do not depend on atom numbering run on the twin — lists keyed by the original
index, so rows come out in the reference's order and every sum runs over the same numbers in the same order — and what the user
reads is translated back: per-atom columns by one scatter, the rows of a list only if somebody asks for them (devarray.LazyHArray).
MDAPY_SPATIAL_SORT = 0 (never), 1 (always, whatever the order looks like; any size — tests), unset (systems of MDAPY_SORT_MIN_ATOMS
atoms and more whose order statistic says so)."""
import os
import weakref
from collections import namedtuple

import numpy as np

from . import kernels, policy
from .devarray import HArray, LazyHArray, have_gpu
from .frame import Frame, PermutedColumn

SORT_MIN_ATOMS = int(os.environ.get("MDAPY_SORT_MIN_ATOMS", "200000"))
SORT_FAR_FRACTION = 0.25  # of consecutive atoms in bins that do not touch (mdh_order_statistic): a lattice builder's order has < 0.01


def adf_reach(rc_dict):
    """the list cutoff of an angular distribution function: the largest number of all its ranges (system.py:2214), or None"""
    try:
        values = np.asarray(list(rc_dict.values()), dtype=float)
        return float(values.max()) if values.size else None
    except (AttributeError, TypeError, ValueError):
        return None


# The frames of a trajectory share their atom numbering: when a System has just been sorted and the next one brings as many atoms in
# the same box shape, its positions are first read through the LAST permutation — atoms move a fraction of a cell between frames, the
# old cell order is still a spatial order — and the order statistic of the result decides whether that will do (three gathers and a
# sampling pass instead of a sort: the sort is as long as the whole neighbor + CNA step of an ordered frame).  One slot for the whole
# process, held strongly (a weak one would die between the frames of ``for frame: s = System(...)``); the record is replaced whole
# and read as one snapshot, so a reader never pairs one frame's permutation with another's atom count.
Order = namedtuple("Order", "perm n pbc host")  # HArray / ndarray, atoms, boundary flags, whether the permutation is in host memory
_last = None


def forget_order():
    global _last
    _last = None


def _remember_order(perm, n, where):
    global _last
    _last = Order(perm, int(n), tuple(int(v) for v in np.asarray(where[5]).ravel()), isinstance(perm, np.ndarray))


def _sorted_as_last_time(cols, where, n):
    last = _last
    if last is None or last.n != int(n) or os.environ.get("MDAPY_REUSE_ORDER", "1") == "0" \
            or last.pbc != tuple(int(v) for v in np.asarray(where[5]).ravel()):
        return None
    on_dev = any(c._host_arr is None or c._dev is not None for c in cols)
    if on_dev == last.host:
        return None  # (the permutation lives in the other memory space)
    arrs = [c.device_array() if on_dev else c.to_numpy() for c in cols]
    if hasattr(kernels.order, "gather_positions"):
        moved = list(kernels.order.gather_positions(*arrs, last.perm))
    else:
        moved = [kernels.order.permute(a, last.perm) for a in arrs]
    # an absent atom (a coordinate that is NaN; infinite ones with it) is binned by neither the statistic nor a sort: the sort reports
    # fewer atoms than N and the caller makes no twin — so must this path, which never counts (a sum of finite numbers that overflows
    # only sends the frame to the sort)
    if on_dev:
        total = sum(m.dev().sum() for m in moved)
        if not bool(total.isfinite()):
            return None
    elif not np.isfinite(sum(float(np.sum(m)) for m in moved)):
        return None
    if kernels.order.order_statistic(*moved, *where[3:]) > SORT_FAR_FRACTION:
        return None  # another numbering after all: sort
    return moved[0], moved[1], moved[2], last.perm, int(n)


# what of the twin's list the owner shows: the twin's three list objects, their sorted depth, the owner's ``verlet_list`` made from them
Shown = namedtuple("Shown", "rows dist counts depth mirror")


class Twin:
    """all that ties a system (the owner, which keeps it as ``_twin``) to its sorted copy: the decision for one set of position columns
    and one box — held strongly and compared with ``is``, so that "the same object" cannot be a new one at a recycled address — and
    what follows from it.  ``system`` is the sorted ``System`` (of all this it carries a weak reference back, ``_twin_of``), or None: no twin for these"""
    __slots__ = ("made_from", "system", "perm", "order_key", "columns", "shown", "__weakref__")

    def __init__(self, owner):
        cols = tuple(owner._frame[c] for c in ("x", "y", "z"))
        self.made_from = (*cols, owner._cell)
        self.system = self.perm = self.order_key = self.shown = None
        self.columns = {}  # name -> (the owner's column, the same read through the permutation)
        mode = owner._sort_mode
        big = owner.N >= SORT_MIN_ATOMS or (mode == "1" and owner.N >= 2)
        if big and hasattr(kernels, "order") and (have_gpu() or mode == "1") and all(np.dtype(c.dtype) == np.float64 for c in cols) \
                and policy.is_single(owner._safe_repeat()):
            where = (*cols, *policy.box_args(owner.box))
            if mode == "1" or kernels.order.order_statistic(*where) > SORT_FAR_FRACTION:
                xs, ys, zs, perm, n = _sorted_as_last_time(cols, where, owner.N) or kernels.order.spatial_sort(*where)
                if n == owner.N:
                    _remember_order(perm, owner.N, where)
                    self.perm = perm
                    # the in-cell ordering key of the twin's list builds: the ORIGINAL index, so that a row lists its atoms in the
                    # order the reference would (descending index inside a cell, neighbor.cpp:97-98)
                    self.order_key = HArray(perm.dev().long()) if isinstance(perm, HArray) else np.asarray(perm, np.int64)
                    self.system = type(owner)(data=Frame({"x": xs, "y": ys, "z": zs}), box=owner.box)
                    self.system._twin_of = weakref.ref(self)

    def forget_lists(self):
        """the owner's list is gone: the twin's too, and what mirrored it"""
        if self.system is not None:
            self.system._forget_list()
        self.shown = None

    def mirrors(self, owner):
        """whether the list ``owner`` remembers is the twin's list, translated, rows in the twin's order: the mirror itself, its front
        sorted as deep as the twin's (sums, and an ADF whose two ranges differ, depend on the order of a row; see System._sort_front)"""
        shown, mine = self.shown, owner.__dict__.get("verlet_list")
        return shown is not None and mine is shown.mirror and owner._front() == shown.depth

    def listed(self, owner):
        """whether the list ``owner`` remembers is the twin's, translated and in step, and the twin still has it"""
        return self.mirrors(owner) and "verlet_list" in self.system.__dict__

    def may_run(self, owner, name, bound):
        """whether method ``name`` of ``owner`` may run on the twin; ``bound``: the arguments the caller passed, by name"""
        # the list the owner remembers must be the twin's (translated), or neither has one (build_neighbor replaces all of it anyway)
        if owner.__dict__.get("verlet_list") is not None:
            if name != "build_neighbor" and owner._listed_on_twin() is not self.system:
                return False
        elif "verlet_list" in self.system.__dict__:
            self.forget_lists()
        reach = bound.get("rc", bound.get("cutoff", bound.get("average_rc")))
        if name == "cal_angular_distribution_function":
            reach = adf_reach(bound.get("rc_dict"))
        if name in ("cal_bond_analysis", "cal_angular_distribution_function") and isinstance(reach, (int, float, np.integer, np.floating)) \
                and "rc" in owner.__dict__ and owner.rc >= reach and "_list_cutoff" not in owner.__dict__:
            return False  # (a k-nearest list beside a stale rc is reused as it is: its rows are not symmetric, so j > i depends on numbering)
        if isinstance(reach, (int, float, np.integer, np.floating)) and reach > 0 and \
                not policy.is_single(policy.axis_copies(owner.box, 2.0 * float(reach))):
            return False  # the build would search a replica: the ordering key cannot follow
        if name == "cal_steinhardt_bond_orientation" and (bound.get("use_voronoi") or bound.get("identify_liquid")
                                                         or bound.get("weight") is not None):
            return False  # (a caller's weight array lines up with the OWNER's rows, not with the twin's permuted ones)
        return True

    def run(self, owner, name, args, kwargs):
        """method ``name`` on the twin; what it left — columns, list, result — as the owner's"""
        twin, perm = self.system, self.perm
        # every column the twin does not have yet, read through the permutation (nothing moves before a kernel asks)
        cols = {cname: twin._frame[cname] for cname in twin._frame.columns[:3]}
        for cname in owner._frame.columns:
            if cname in ("x", "y", "z"):
                continue
            src = owner._frame[cname]
            hit = self.columns.get(cname)
            if hit is None or hit[0] is not src:
                hit = self.columns[cname] = (src, PermutedColumn(src, perm))
            cols[cname] = hit[1]
        twin._frame = Frame(cols)
        twin._frame.order_key = self.order_key  # (what a k-nearest search on this frame breaks exact ties by: knn.py)
        before = {cname: twin._frame[cname] for cname in twin._frame.columns}
        result = getattr(twin, name)(*args, **kwargs)
        # per-atom results: columns the call added or replaced, back in the owner's order
        restored = {}
        for cname in twin._frame.columns:
            col = twin._frame[cname]
            if before.get(cname) is col:
                continue
            kind = np.dtype(col.dtype)
            if col._host_arr is None and kind.kind in "iuf" and kind.itemsize in (4, 8):
                restored[cname] = kernels.order.permute(col.device_array(), perm, scatter=True)
            else:
                out = np.empty_like(col.to_numpy())
                out[np.asarray(perm)] = col.to_numpy()
                restored[cname] = out
        if restored:
            owner.update_data(owner._frame.with_columns(**restored))
        # the list the twin remembers now, as the owner's: translated when somebody reads it
        self.mirror_lists(owner)
        if "ptm_indices" in twin.__dict__ and name == "cal_polyhedral_template_matching":
            src = twin.ptm_indices
            owner.ptm_indices = LazyHArray(lambda: kernels.order.translate_rows(src, None, None, perm)[0].dev(), src.shape, np.int32) \
                if isinstance(src, HArray) else kernels.order.translate_rows(np.asarray(src), None, None, np.asarray(perm))[0]
        if name == "build_neighbor" and result is not None:  # the labels of build_neighbor(..., _label=True): per atom, the twin's order
            result = kernels.order.permute(result, perm, scatter=True)
        return result

    def mirror_lists(self, owner):
        """what the twin remembers of a list now, as the owner's: nothing, or its mirror — a new one only if the old one is stale"""
        twin = self.system
        if "verlet_list" not in twin.__dict__:
            return owner._forget_list()
        rows, dist, counts, depth = twin.verlet_list, twin.distance_list, twin.neighbor_number, max(twin._front(), 0)
        shown = self.shown
        if shown is None or shown.rows is not rows or shown.dist is not dist or shown.counts is not counts or shown.depth != depth \
                or owner.__dict__.get("verlet_list") is not shown.mirror:
            perm, done = self.perm, {}

            def translated(k):
                if not done:
                    done["v"], done["d"], done["n"] = kernels.order.translate_rows(rows, dist, counts, perm)
                return done[k]

            if isinstance(rows, HArray):
                out = (LazyHArray(lambda: translated("v").dev(), rows.shape, np.int32),
                       LazyHArray(lambda: translated("d").dev(), dist.shape, np.float64),
                       # (the counts alone: `_deep_enough` and the overflow check read them; the N x M rows need not move for that)
                       LazyHArray(lambda: (done["n"] if done else kernels.order.permute(counts, perm, scatter=True)).dev(), counts.shape, np.int32))
            else:
                out = (translated("v"), translated("d"), translated("n"))
            self.shown = Shown(rows, dist, counts, depth, out[0])
            owner.verlet_list, owner.distance_list, owner.neighbor_number = out
        for attr in ("rc", "_list_cutoff"):
            if attr in twin.__dict__:
                setattr(owner, attr, twin.__dict__[attr])
            else:
                owner.__dict__.pop(attr, None)
        owner._sorted_columns = (weakref.ref(owner.verlet_list), depth)
        owner._forget(("_enlarge_box", "_enlarge_data"))  # (the twin never lists a replica)
