"""Host check of what a cell grid build decides before it enqueues anything (mdapy_amd/csrc/grid_plan.hpp plan_grid, through
mdh_debug_grid_plan): the form the atoms are kept in, whether the build keeps its signature's history and samples the order of the
atoms, the planes of a promised cell window and of a centre window, the in-cell sort and the atoms per lane of the binning.
Every rule only picks a path: each line of the tables is a build whose grid holds the same atoms whichever way it goes."""
import ctypes as C

import pytest

from mdapy_amd import _lib

ARRAYS, FOR_ROWS, FOR_ROWS_UNORDERED = 0, 1, 2                       # in: what the atoms are wanted as
F_ARRAYS, F_GATHERED, F_MOVED, F_INDIRECT, F_SLOT = 0, 1, 2, 3, 4    # out: form
S_NONE, S_DENSE, S_CELLS, S_PIECES = 0, 1, 2, 3                      # out: sort

IN_I = ["atoms", "sort_desc", "keyed", "slots_ok", "row_width", "N", "ncell", "nc0", "nc1", "nc2", "mode", "tri", "cells_set", "cells_axis",
        "centre_set", "centre_axis", "order_word", "order_sample", "big", "listed", "record_width", "indirect_on", "slot_on", "slot_force"]
IN_D = ["rc_inv", "h0", "cells_lo", "cells_hi", "centre_lo", "centre_hi"]
OUT = ["form", "keeps_history", "samples_order", "assign4", "p0", "p1", "p2", "p3", "windowed", "win_lo", "win_hi", "cen_lo", "cen_hi", "sort",
       "row_width"]


def plan(values):
    ii = (C.c_int64 * len(IN_I))(*[values[k] for k in IN_I])
    dd = (C.c_double * len(IN_D))(*[values[k] for k in IN_D])
    out = (C.c_int * len(OUT))()
    assert _lib.lib().mdh_debug_grid_plan(ii, dd, out) == 0
    return dict(zip(OUT, out))


def box(edge, planes):
    """An orthogonal periodic box of that edge under rc = 2: `planes` cells per axis."""
    return dict(h0=float(edge), rc_inv=0.5, nc0=planes, nc1=planes, nc2=planes, ncell=planes**3)


def cells(lo, hi, axis=0):
    return dict(cells_set=1, cells_axis=axis, cells_lo=lo, cells_hi=hi)


def centre(lo, hi, axis=0):
    return dict(centre_set=1, centre_axis=axis, centre_lo=lo, centre_hi=hi)


# a build for neighbour rows behind the neighbour pass, no hint pending, nothing known of its signature, every switch as shipped
ROWS = dict(atoms=FOR_ROWS, sort_desc=1, keyed=0, slots_ok=1, row_width=16, N=0, ncell=0, nc0=0, nc1=0, nc2=0, mode=0, tri=0,
            cells_set=0, cells_axis=0, cells_lo=0.0, cells_hi=0.0, centre_set=0, centre_axis=0, centre_lo=0.0, centre_hi=0.0,
            order_word=0, order_sample=0, big=-1, listed=-1, record_width=0, indirect_on=1, slot_on=1, slot_force=0, rc_inv=0.5, h0=0.0)

# ---- planes: edge 128, rc = 2: 64 planes, every fraction dyadic ----
B64 = dict(ROWS, N=1_000_000, **box(128, 64))
ALL64 = dict(windowed=0, p0=0, p1=64, p2=0, p3=0, win_lo=0, win_hi=0)


def one_piece(a, b):
    return dict(windowed=1, p0=a, p1=b, p2=0, p3=0, win_lo=a, win_hi=b, sort=S_PIECES)


def two_pieces(b, c):
    return dict(windowed=1, p0=0, p1=b, p2=c, p3=64, win_lo=0, win_hi=0, sort=S_PIECES)


CELL_WINDOWS = [
    ("a quarter of the box", cells(0.25, 0.5), one_piece(15, 33)),
    ("the margin reaches plane 0", cells(0.015625, 0.71875), one_piece(0, 47)),
    ("just under three quarters", cells(0.125, 0.859375), one_piece(7, 56)),
    ("three quarters wide: not worth it", cells(0.125, 0.875), ALL64),
    ("empty", cells(0.5, 0.5), ALL64),
    ("from the lower face: the margin wraps below", cells(0.0, 0.25), two_pieces(17, 63)),
    ("around the lower face", cells(-0.125, 0.125), two_pieces(9, 55)),
    ("wraps below, wide", cells(0.0, 0.734375), two_pieces(48, 63)),
    ("to the upper face: the margin wraps above", cells(0.75, 1.0), two_pieces(1, 47)),
    ("around the upper face", cells(0.875, 1.125), two_pieces(9, 55)),
    ("15 planes: too few", dict(cells(0.25, 0.5), **box(30, 15)), dict(windowed=0, p0=0, p1=15, p2=0, p3=0, win_lo=0, win_hi=0)),
    ("16 planes: enough", dict(cells(0.25, 0.5), **box(32, 16)), one_piece(3, 9)),
    ("a triclinic box", dict(cells(0.25, 0.5), tri=1), ALL64),
    ("along axis 1", cells(0.25, 0.5, axis=1), ALL64),
    ("equal cells across the box (grid mode 1)", dict(cells(0.25, 0.5), mode=1), ALL64),
    ("a request for sorted arrays", dict(cells(0.25, 0.5), atoms=ARRAYS), ALL64),
    ("no window at all", {}, dict(ALL64, sort=S_CELLS)),
]

CENTRE_WINDOWS = [
    ("a quarter of the box", centre(0.25, 0.5), dict(cen_lo=15, cen_hi=33)),
    ("the whole box", centre(0.0, 1.0), dict(cen_lo=0, cen_hi=64)),
    ("the lowest eighth", centre(0.0, 0.125), dict(cen_lo=0, cen_hi=9)),
    ("the highest eighth", centre(0.875, 1.0), dict(cen_lo=55, cen_hi=64)),
    ("starts below the box: dropped", centre(-0.1, 0.5), dict(cen_lo=0, cen_hi=0)),
    ("ends above the box: dropped", centre(0.5, 1.01), dict(cen_lo=0, cen_hi=0)),
    ("empty: dropped", centre(0.5, 0.5), dict(cen_lo=0, cen_hi=0)),
    ("a triclinic box: dropped", dict(centre(0.25, 0.5), tri=1), dict(cen_lo=0, cen_hi=0)),
    ("along axis 2: dropped", centre(0.25, 0.5, axis=2), dict(cen_lo=0, cen_hi=0)),
    ("a request for sorted arrays: dropped", dict(centre(0.25, 0.5), atoms=ARRAYS), dict(cen_lo=0, cen_hi=0)),
    ("takes no part in the cell window", centre(0.25, 0.5), ALL64),
    ("beside a cell window", dict(centre(0.25, 0.375), **cells(0.125, 0.5)), dict(one_piece(7, 33), cen_lo=15, cen_hi=25)),
]

# ---- form: the headline, 10 061 824 atoms in 159^3 cells ----
HEAD = dict(ROWS, N=10_061_824, **box(318, 159))
SEEN = dict(big=0, listed=0)  # a build of the signature has finished, saw no full cell and listed no tile
DENSE = box(200, 100)         # 10^6 cells: ten atoms a cell at the headline's N

FORMS = [
    ("sorted arrays asked for", dict(SEEN, atoms=ARRAYS), dict(form=F_ARRAYS, keeps_history=0, samples_order=0, assign4=1)),
    ("input known to be unordered", dict(atoms=FOR_ROWS_UNORDERED), dict(form=F_MOVED, keeps_history=0, assign4=0)),
    ("... never indirect or slot, whatever the history", dict(SEEN, atoms=FOR_ROWS_UNORDERED, order_word=0), dict(form=F_MOVED, keeps_history=0)),
    ("the order sample said unordered", dict(SEEN, order_word=1), dict(form=F_MOVED, keeps_history=0, assign4=0)),
    ("the order sample said ordered", dict(order_word=0, slots_ok=0), dict(form=F_INDIRECT, keeps_history=0, assign4=1)),
    ("2^18 atoms: the word is consulted", dict(order_word=1, N=1 << 18), dict(form=F_MOVED)),
    ("below 2^18 atoms it is not", dict(order_word=1, N=(1 << 18) - 1), dict(form=F_INDIRECT, keeps_history=0, assign4=0)),
    ("six atoms a cell", dict(DENSE, N=6_000_000), dict(form=F_INDIRECT)),
    ("more than six atoms a cell", dict(DENSE, N=6_000_001), dict(form=F_GATHERED, keeps_history=0)),
    ("ten atoms a cell", dict(SEEN, **DENSE), dict(form=F_GATHERED, keeps_history=0)),
    ("rows of 17 slots", dict(SEEN, row_width=17), dict(form=F_GATHERED, keeps_history=0, row_width=17)),
    ("row width from the record: 12", dict(row_width=-1, record_width=12), dict(form=F_INDIRECT, row_width=12)),
    ("row width from the record: 24", dict(row_width=-1, record_width=24), dict(form=F_GATHERED, row_width=24)),
    ("row width from a record that is not there", dict(row_width=-1, record_width=24, slots_ok=0), dict(form=F_INDIRECT, row_width=0)),
    ("indirect switched off", dict(SEEN, indirect_on=0), dict(form=F_GATHERED, keeps_history=0)),
    ("cells not sorted", dict(SEEN, sort_desc=0), dict(form=F_GATHERED, keeps_history=0, sort=S_NONE)),
    ("history seen, no full cell, no tile listed", SEEN, dict(form=F_SLOT, keeps_history=1, assign4=1)),
    ("the first build of a signature", dict(big=-1), dict(form=F_INDIRECT, keeps_history=1)),
    ("the last build saw a full cell", dict(big=1, listed=0), dict(form=F_INDIRECT, keeps_history=1)),
    ("the last build listed tiles", dict(big=0, listed=3), dict(form=F_INDIRECT, keeps_history=1)),
    ("listed tiles not known yet", dict(big=0, listed=-1), dict(form=F_INDIRECT, keeps_history=1)),
    ("a build that is not behind the neighbour pass", dict(SEEN, slots_ok=0), dict(form=F_INDIRECT, keeps_history=0)),
    ("a sort key", dict(SEEN, keyed=1), dict(form=F_INDIRECT, keeps_history=0)),
    ("a cell window pending", dict(SEEN, **cells(0.25, 0.5)), dict(form=F_INDIRECT, keeps_history=0, windowed=1)),
    ("a cell window pending that the build drops", dict(SEEN, **cells(0.25, 0.5, axis=1)), dict(form=F_INDIRECT, keeps_history=0, windowed=0)),
    ("a centre window pending", dict(SEEN, **centre(0.25, 0.5)), dict(form=F_INDIRECT, keeps_history=0)),
    ("slot grid switched off", dict(SEEN, slot_on=0), dict(form=F_INDIRECT, keeps_history=1)),
    ("forced: a slot grid on a first build", dict(big=-1, slot_force=1), dict(form=F_SLOT, keeps_history=1)),
    ("forced, but switched off", dict(big=-1, slot_force=1, slot_on=0), dict(form=F_INDIRECT, keeps_history=1)),
    ("forced, but rows of 17 slots", dict(big=-1, slot_force=1, row_width=17), dict(form=F_GATHERED, keeps_history=0)),
]

SORT_AND_LANES = [
    ("cells not sorted", dict(sort_desc=0), dict(sort=S_NONE)),
    ("not sorted, windowed", dict(sort_desc=0, **cells(0.25, 0.5)), dict(sort=S_NONE, windowed=1)),
    ("few atoms a cell", {}, dict(sort=S_CELLS)),
    ("six atoms a cell", dict(DENSE, N=6_000_000), dict(sort=S_CELLS)),
    ("dense cells", dict(DENSE, N=6_000_001), dict(sort=S_DENSE)),
    ("dense cells of a request for sorted arrays", dict(DENSE, atoms=ARRAYS), dict(sort=S_DENSE)),
    ("dense cells with a key", dict(DENSE, keyed=1), dict(sort=S_CELLS)),
    ("dense cells in a window", dict(DENSE, **cells(0.25, 0.5)), dict(sort=S_PIECES, windowed=1)),
    ("a window with a key", dict(keyed=1, **cells(0.25, 0.5)), dict(sort=S_PIECES, windowed=1)),
    ("2^20 atoms: four per lane", dict(N=1 << 20), dict(assign4=1)),
    ("one fewer: one per lane", dict(N=(1 << 20) - 1), dict(assign4=0)),
    ("2^20 atoms known to be unordered", dict(N=1 << 20, atoms=FOR_ROWS_UNORDERED), dict(assign4=0)),
    ("2^20 atoms sampled as unordered", dict(N=1 << 20, order_word=1), dict(assign4=0)),
    ("2^20 atoms for sorted arrays", dict(N=1 << 20, atoms=ARRAYS, order_word=1), dict(assign4=1, form=F_ARRAYS)),
    ("a sample is due", dict(order_sample=1), dict(samples_order=1)),
    ("... also when the last one said unordered", dict(order_sample=1, order_word=1), dict(samples_order=1, form=F_MOVED)),
    ("no sample below 2^18 atoms", dict(order_sample=1, N=(1 << 18) - 1), dict(samples_order=0)),
    ("no sample of input known to be unordered", dict(order_sample=1, atoms=FOR_ROWS_UNORDERED), dict(samples_order=0)),
    ("no sample for sorted arrays", dict(order_sample=1, atoms=ARRAYS), dict(samples_order=0)),
]


def check(base, name, change, want):
    values = dict(base, **change)
    got = plan(values)
    assert {k: got[k] for k in want} == want, (name, values, got)


@pytest.mark.parametrize("name,change,want", CELL_WINDOWS, ids=[t[0] for t in CELL_WINDOWS])
def test_cell_window_planes(name, change, want):
    check(B64, name, change, want)


@pytest.mark.parametrize("name,change,want", CENTRE_WINDOWS, ids=[t[0] for t in CENTRE_WINDOWS])
def test_centre_window_planes(name, change, want):
    check(B64, name, change, want)


@pytest.mark.parametrize("name,change,want", FORMS, ids=[t[0] for t in FORMS])
def test_form(name, change, want):
    check(HEAD, name, change, want)


@pytest.mark.parametrize("name,change,want", SORT_AND_LANES, ids=[t[0] for t in SORT_AND_LANES])
def test_sort_and_lanes(name, change, want):
    check(HEAD, name, change, want)


def test_agrees_with_the_slot_grid_rule():
    """The plan takes the slot grid exactly where mdh_debug_slot_grid_rule says so (tests/test_slot_grid_rule.py has its table)."""
    L = _lib.lib()
    for big, listed in ((-1, -1), (0, 0), (1, 0), (0, 2), (0, -1)):
        for keyed in (0, 1):
            for width in (0, 16, 17):
                got = plan(dict(HEAD, big=big, listed=listed, keyed=keyed, row_width=width))
                rule = L.mdh_debug_slot_grid_rule(int(got["form"] in (F_INDIRECT, F_SLOT)), keyed, 0, width, HEAD["ncell"], HEAD["N"],
                                                  int(big >= 0), int(big > 0), listed)
                assert (got["form"] == F_SLOT) == bool(rule), (big, listed, keyed, width, got)
