"""Host check of the rule by which a neighbour build takes the slot grid (mdapy_amd/csrc/cell_grid.hip slot_grid_rule, through
mdh_debug_slot_grid_rule): spatially ordered input, no sort key, no pending window, rows of at most 16 slots, at most two cells per
atom, slots that 32 bits can index, and a previous build of the signature that has finished, saw no cell of more than eight atoms
and listed no tile.  The rule only picks the faster path: every line of the table is a build whose result is the same either way."""
import pytest

from mdapy_amd import _lib

N = 10_061_824
NCELL = 4_019_679
#        ordered keyed windowed width ncell      N        seen big listed
OK = dict(ordered=1, keyed=0, windowed=0, row_width=16, ncell=NCELL, N=N, seen=1, big=0, listed=0)

TABLE = [
    ("the headline build after its first", {}, 1),
    ("counting pass, width not known", dict(row_width=0), 1),
    ("unordered input (records)", dict(ordered=0), 0),
    ("a sort key (decomposed step)", dict(keyed=1), 0),
    ("a cell or centre window pending", dict(windowed=1), 0),
    ("rows of 17 slots: the wide instance", dict(row_width=17), 0),
    ("two cells per atom", dict(ncell=2 * N), 1),
    ("more than two cells per atom", dict(ncell=2 * N + 1), 0),
    ("a gas: 27 cells, 10 atoms", dict(ncell=27, N=10), 0),
    ("eight slots a cell just within 32 bits", dict(ncell=(1 << 28) - 1, N=1 << 30), 1),
    ("eight slots a cell past 32 bits", dict(ncell=1 << 28, N=1 << 30), 0),
    ("the first build of a signature", dict(seen=0), 0),
    ("the last build saw a cell of nine", dict(big=1), 0),
    ("the last build listed a tile", dict(listed=1), 0),
    ("listed tiles not known yet", dict(listed=-1), 0),
]


@pytest.mark.parametrize("name,change,want", TABLE, ids=[t[0] for t in TABLE])
def test_rule(name, change, want):
    a = dict(OK, **change)
    got = _lib.lib().mdh_debug_slot_grid_rule(a["ordered"], a["keyed"], a["windowed"], a["row_width"], a["ncell"], a["N"], a["seen"], a["big"], a["listed"])
    assert got == want, (name, a)
