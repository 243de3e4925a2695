"""The table of tests/test_neighbor_plan.py and tests/native/neighbor_plan_host.cpp: inputs of the neighbour pass's planners
(mdapy_amd/csrc/neighbor_plan.hpp, through mdh_debug_lane_plan) that take every branch, and the recording of what the planners
answered, tests/golden/neighbor_plan.txt.

The recording was made BEFORE the planners moved into the header — from plan_lane_fresh, the words of mdh_debug_neighbor_plan, the
text of launch_neighbor_lane's geometry and plan_tiled as they stood in neighbor_lane.hip and neighbor_tiled.hip — so the
expectation is not the code under test's.  `python tests/_neighbor_plan_cases.py record` writes the file from the library as built: for a
NEW case only, after reading what it says.

One line per case:  name | 19 integers | 16 doubles | statistics | 46 doubles   (doubles as C99 hex floats; statistics as
index:value pairs, `*` for every index, later pairs over earlier ones)."""
import ctypes as C
import math
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
GOLDEN = os.path.join(HERE, "golden", "neighbor_plan.txt")
NBIN = 99
IN_I = ["nc0", "nc1", "nc2", "ncell", "mode", "pbc0", "pbc1", "pbc2", "tri", "N", "M", "fcna", "count", "win_lo", "win_hi", "cen_lo", "cen_hi",
        "last_listed", "memo"]
OUT = ["txy", "tz", "cap", "tk8", "wgs", "rw", "mid", "T", "full", "occupied", "reason", "lds_bytes", "pop", "over96", "runs",
       "hook0", "hook1", "hook2", "hook3", "hook4", "hook5", "hook6", "hook7",
       "nt0", "nt1", "nt2", "ntiles", "tiles", "tile_base", "nt0_run", "per", "grid", "standby", "slice_pass", "nsub", "nt2b", "list_cap",
       "mop_tile_z", "mop_nt2", "t_tile", "t_tile_z", "t_cellshift", "t_full", "t_occupied", "cen_lo", "cen_hi"]
ALL, WINDOW, LIST = 0, 1, 2  # out: tiles


def case(nc, N, M, rc=3.0, pbc=(1, 1, 1), stats=None, h=None, thick=None, origin=(0.0, 0.0, 0.0), tri=0, mode=0, fcna=0, count=0,
         win=(0, 0), cen=(0, 0), last_listed=-1, ncell=None):
    """An orthogonal box of nc cells of width 3 (a hair more) per axis unless h / thick are given; stats: [(index, value), ...]
    ('*': every index), default: every cell occupied, every run of round(3 N / ncell) atoms."""
    nc = tuple(nc)
    ncell = nc[0] * nc[1] * nc[2] if ncell is None else ncell
    edge = [n * 3.0 * 1.0000001 for n in nc]  # (the cells are counted in nc; the box only bounds the coordinates)
    h = [edge[0], 0.0, 0.0, 0.0, edge[1], 0.0, 0.0, 0.0, edge[2]] if h is None else list(h)
    thick = edge if thick is None else list(thick)
    if stats is None:
        stats = [(0, ncell), (1 + min(97, max(0, round(3 * N / max(1, ncell)))), ncell)]
    ii = [nc[0], nc[1], nc[2], ncell, mode, pbc[0], pbc[1], pbc[2], tri, N, M, fcna, count, win[0], win[1], cen[0], cen[1], last_listed, 0]
    dd = h + list(origin) + thick + [rc]
    return {"i": ii, "d": [float(v) for v in dd], "stats": list(stats)}


def delta(occupied, length, runs):
    return [(0, occupied), (1 + length, runs)]


def tri_box():
    h = np.array([[120.0, 0.0, 0.0], [30.0, 120.0, 0.0], [20.0, 10.0, 120.0]])
    vol = abs(np.linalg.det(h))
    thick = [vol / np.linalg.norm(np.cross(h[(d + 1) % 3], h[(d + 2) % 3])) for d in range(3)]
    return h.ravel().tolist(), [float(t) for t in thick]


def table():
    t = {}
    G20, G40 = (20, 20, 20), (40, 40, 40)
    # ---- refusals ----
    t["refuse_no_atoms"] = case(G20, 0, 16)
    t["refuse_mode"] = case(G20, 20000, 16, mode=1)
    t["refuse_M0"] = case(G20, 20000, 0)
    t["refuse_M129"] = case(G20, 20000, 129)
    t["M128"] = case(G20, 20000, 128)
    t["refuse_periodic_6_cells"] = case((7, 6, 7), 800, 16)
    t["periodic_7_cells"] = case((7, 7, 7), 800, 16)
    t["refuse_open_3_cells"] = case((4, 4, 3), 150, 16, pbc=(0, 0, 0))
    t["open_4_cells"] = case((4, 4, 4), 150, 16, pbc=(0, 0, 0))
    t["mixed_open_4_periodic_7"] = case((4, 7, 7), 500, 16, pbc=(0, 1, 1))
    t["refuse_rc_tiny"] = case(G20, 20000, 16, rc=1e-13)
    t["refuse_rc_huge"] = case(G20, 20000, 16, rc=1e12)
    t["refuse_rc_nan"] = case(G20, 20000, 16, rc=float("nan"))
    t["refuse_long_runs"] = case(G20, 80000, 50, stats=[(0, 8000), (1 + 30, 949), (1 + 90, 51)])      # 5.1 % of the runs at 89 or above
    t["long_runs_at_the_limit"] = case(G20, 80000, 50, stats=[(0, 8000), (1 + 30, 950), (1 + 90, 50)])  # 5 %: not more
    t["refuse_M65_pop_above"] = case((10, 10, 10), 19501, 65, stats=delta(1000, 58, 1000))
    t["M65_pop_below"] = case((10, 10, 10), 19499, 65, stats=delta(1000, 58, 1000))
    t["M64_pop_above"] = case((10, 10, 10), 19501, 64, stats=delta(1000, 58, 1000))
    t["refuse_no_shape"] = case((10, 10, 10), 70000, 64, stats=delta(1000, 60, 1000))
    # ---- instance ----
    t["M16_short_runs"] = case(G20, 20000, 16, stats=[(0, 8000), (1 + 8, 7000), (1 + 28, 1000)])
    t["M16_runs_of_29_0.3pc"] = case(G20, 20000, 16, stats=[(0, 8000), (1 + 8, 7976), (1 + 29, 24)])
    t["M16_runs_of_29_0.1pc"] = case(G20, 20000, 16, stats=[(0, 8000), (1 + 8, 7992), (1 + 29, 8)])
    t["M17"] = case(G20, 20000, 17)
    t["count_M50"] = case(G20, 20000, 50, count=1)
    t["count_M1"] = case(G20, 20000, 1, count=1)
    t["M16_fcna"] = case(G20, 20000, 16, fcna=1)
    # ---- shape search ----
    t["headline"] = case((159, 159, 159), 10061824, 16)
    t["headline_fcna"] = case((159, 159, 159), 10061824, 16, fcna=1)
    t["pop1_M50"] = case(G40, 64000, 50)
    t["pop6_M50"] = case(G40, 6 * 64000, 50)
    t["pop11_M50"] = case(G40, 11 * 64000, 50)
    t["pop19_M128"] = case(G40, 19 * 64000, 128)
    t["mostly_empty"] = case(G40, 16000, 16, stats=delta(6400, 8, 6400))
    h, thick = tri_box()
    t["triclinic"] = case(tuple(int(th // 3.0) for th in thick), 400000, 16, h=h, thick=thick, tri=1, origin=(-5.0, 2.0, 40.0))
    t["triclinic_M50"] = case(tuple(int(th // 3.0) for th in thick), 400000, 50, h=h, thick=thick, tri=1, origin=(-5.0, 2.0, 40.0))
    t["orthogonal_far_origin"] = case(G40, 160000, 16, origin=(1e9, -1e9, 0.0))
    t["full_at_98pc"] = case(G40, 160000, 16, stats=delta(62720, 8, 64000))
    t["not_full_below_98pc"] = case(G40, 160000, 16, stats=delta(62719, 8, 64000))
    # ---- launch geometry (one shape: 40^3 cells, 2.5 atoms per cell, rows of 16) ----
    part = delta(30000, 8, 64000)
    for tag, ll in (("none_listed", 0), ("some_listed", 5), ("unknown_listed", -1)):
        t["launch_all_" + tag] = case(G40, 160000, 16, last_listed=ll)
        t["launch_list_standby_" + tag] = case(G40, 8000, 16, stats=delta(3200, 8, 3200), last_listed=ll)
        t["launch_list_whole_" + tag] = case(G40, 150000, 16, stats=delta(60000, 8, 64000), last_listed=ll)
        t["launch_window_" + tag] = case(G40, 75000, 16, stats=part, win=(8, 20), last_listed=ll)
    t["launch_window_centre_inside"] = case(G40, 75000, 16, stats=part, win=(8, 20), cen=(10, 14))
    t["launch_window_centre_one_plane"] = case(G40, 75000, 16, stats=part, win=(8, 20), cen=(12, 13))
    t["launch_window_centre_wider"] = case(G40, 75000, 16, stats=part, win=(8, 20), cen=(2, 30))
    t["launch_window_one_plane"] = case(G40, 75000, 16, stats=part, win=(8, 9))
    t["launch_window_last_plane"] = case(G40, 75000, 16, stats=part, win=(39, 40))
    t["launch_centre_without_window"] = case(G40, 75000, 16, stats=part, cen=(10, 14))
    t["launch_window_on_a_full_grid"] = case(G40, 160000, 16, win=(8, 20))
    # ---- the round-1 tiled plan ----
    for M in (32, 33, 47, 48):  # (a power of two and one above; the last row width whose tickets fit LDS and the first that does not)
        t[f"tiled_M{M}"] = case(G20, 12 * 8000, M)
    t["tiled_6_periodic_cells"] = case((6, 8, 8), 12 * 384, 16)
    t["tiled_7_periodic_cells"] = case((7, 8, 8), 12 * 448, 16)
    t["tiled_6_open_cells"] = case((6, 8, 8), 12 * 384, 16, pbc=(0, 1, 1))
    t["tiled_full"] = case(G20, 12 * 8000, 16)
    t["tiled_one_cell_empty"] = case(G20, 12 * 8000, 16, stats=delta(7999, 36, 8000))
    t["tiled_occupancy_unknown"] = case(G20, 12 * 8000, 16, stats=[(1 + 36, 8000)])
    t["tiled_pop_too_high"] = case(G20, 200 * 8000, 16, stats=delta(8000, 30, 8000))
    # ---- degenerate statistics ----
    t["stats_all_zero"] = case(G20, 20000, 16, stats=[])
    t["stats_all_huge"] = case(G20, 20000, 16, stats=[("*", (2**31 - 1) // 128)])
    t["stats_huge_but_long_runs"] = case(G20, 20000, 16, stats=[("*", (2**31 - 1) // 128)] + [(1 + k, 0) for k in range(29, 98)])
    t["stats_negative_occupancy"] = case(G20, 20000, 16, stats=[(0, -5), (1 + 8, 8000)])
    return t


def stats_array(pairs):
    v = [0] * NBIN
    for k, val in pairs:
        for q in (range(NBIN) if k == "*" else [k]):
            v[q] = val
    return v


def run(c, memo=0, lib=None):
    """The planners' 46 answers for a case, through the library."""
    if lib is None:
        from mdapy_amd import _lib
        lib = _lib.lib()
    ii = list(c["i"]); ii[18] = memo
    a = (C.c_int64 * 19)(*ii)
    d = (C.c_double * 16)(*c["d"])
    s = (C.c_int * NBIN)(*stats_array(c["stats"]))
    out = (C.c_double * 46)()
    f = lib.mdh_debug_lane_plan
    f.argtypes = [C.c_void_p] * 4
    assert f(a, d, s, out) == 0
    return list(out)


def line_of(name, c, out):
    hx = lambda v: "nan" if v != v else float(v).hex()
    return " | ".join([name, " ".join(str(v) for v in c["i"]), " ".join(hx(v) for v in c["d"]),
                       " ".join(f"{k}:{v}" for k, v in c["stats"]) or "-", " ".join(hx(v) for v in out)])


def read_golden(path=GOLDEN):
    """{name: (the line's inputs as line_of writes them, the 46 recorded answers)}"""
    got = {}
    for ln in open(path):
        if not ln.strip() or ln.startswith("#"):
            continue
        name, ii, dd, ss, oo = [f.strip() for f in ln.split("|")]
        got[name] = (" | ".join([ii, dd, ss]), [float.fromhex(v) if v != "nan" else math.nan for v in oo.split()])
    return got


if __name__ == "__main__":
    if sys.argv[1:2] != ["record"]:
        raise SystemExit(__doc__)
    lib = C.CDLL(sys.argv[2]) if len(sys.argv) > 2 else None
    with open(GOLDEN, "w") as f:
        f.write("# name | in_i | in_d | stats | out  (tests/_neighbor_plan_cases.py)\n")
        for name, c in table().items():
            f.write(line_of(name, c, run(c, lib=lib)) + "\n")
