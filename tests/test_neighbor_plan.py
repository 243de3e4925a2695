"""Host check of what a pass over a built cell grid decides before it enqueues anything (mdapy_amd/csrc/neighbor_plan.hpp, through
mdh_debug_lane_plan): whether the LDS-tile kernel takes the call and why not, its tile, LDS budget, instance and decision band,
the words mdh_debug_neighbor_plan reports, the launch geometry, and the round-1 tiled kernel's plan.

The expectation is tests/golden/neighbor_plan.txt: what the planners answered for the table of tests/_neighbor_plan_cases.py while
they still stood in neighbor_lane.hip and neighbor_tiled.hip — recorded before they moved into the header, so not the answers of the
code under test.  Every rule only picks a path or a tile: the rows are the same whichever way a pass goes (the GPU tests)."""
import os
import struct
import subprocess

import numpy as np
import pytest

from _neighbor_plan_cases import ALL, GOLDEN, LIST, OUT, WINDOW, case, line_of, read_golden, run, table
from mdapy_amd import _lib

HERE = os.path.dirname(os.path.abspath(__file__))
TABLE = table()
RECORDED = read_golden()
BITS = ("mid", "T")  # single-precision numbers, compared by bit pattern


def f32_bits(v):
    return struct.unpack("<I", struct.pack("<f", v))[0]


def same(got, want):
    """field for field; the first difference, or None"""
    for k, name in enumerate(OUT):
        a, b = got[k], want[k]
        if name in BITS:
            assert float(np.float32(a)) == a and float(np.float32(b)) == b, (name, a, b)  # a double carries a float exactly
            a, b = f32_bits(a), f32_bits(b)
        if a != b:
            return name, a, b
    return None


def named(out):
    return dict(zip(OUT, out))


def test_table_and_recording_agree():
    """The recording holds exactly the table's cases with the table's inputs."""
    assert sorted(RECORDED) == sorted(TABLE)
    for name, c in TABLE.items():
        ins = line_of(name, c, []).split(" | ", 1)[1].rsplit(" | ", 1)[0]
        assert RECORDED[name][0] == ins, name


@pytest.mark.parametrize("name", sorted(TABLE))
def test_planner_reproduces_the_recording(name):
    assert same(run(TABLE[name]), RECORDED[name][1]) is None, name


def test_recording_takes_every_branch():
    """What the recorded table covers, read off the recording itself (a case that drifted to another branch would go unnoticed
    otherwise)."""
    r = {name: named(out) for name, (_, out) in RECORDED.items()}
    hook = lambda d: [int(d[f"hook{k}"]) for k in range(8)]
    # refusals: the reason, and the eight words
    for name, why in (("refuse_no_atoms", -1), ("refuse_mode", -1), ("refuse_M0", -1), ("refuse_M129", -1), ("refuse_periodic_6_cells", -3),
                      ("refuse_open_3_cells", -3), ("refuse_rc_tiny", -4), ("refuse_rc_huge", -4), ("refuse_rc_nan", -4), ("refuse_no_shape", -6)):
        assert r[name]["txy"] == 0 and r[name]["reason"] == why and hook(r[name]) == [0, 0, 0, 0, 0, 0, why, 0], name
    assert r["refuse_long_runs"]["reason"] == -5 and hook(r["refuse_long_runs"]) == [0, 0, 0, 0, 1000, 51, -5, 0]
    assert r["refuse_M65_pop_above"]["reason"] == -7 and hook(r["refuse_M65_pop_above"]) == [0, 0, 0, 0, 0, 19501, -7, 0]
    for name in ("M128", "periodic_7_cells", "open_4_cells", "mixed_open_4_periodic_7", "long_runs_at_the_limit", "M65_pop_below", "M64_pop_above"):
        d = r[name]
        assert d["txy"] > 0 and d["reason"] == 0, name
        assert hook(d) == [d["txy"], d["tz"], d["cap"], d["lds_bytes"], int(d["full"]) | int(d["tk8"]) << 1 | int(d["wgs"]) << 2, d["pop"],
                           d["occupied"], 1], name
    # instance
    assert r["M16_short_runs"]["tk8"] == 1 and r["M16_short_runs"]["wgs"] == 4
    assert r["M16_runs_of_29_0.3pc"]["tk8"] == 0 and r["M16_runs_of_29_0.1pc"]["tk8"] == 1
    assert r["M17"]["tk8"] == 0 and r["count_M50"]["tk8"] == 1
    # shapes: the headline's tile, and several others
    assert (r["headline"]["txy"], r["headline"]["tz"], r["headline"]["cap"], r["headline"]["lds_bytes"]) == (4, 5, 795, 39792)
    assert len({(r[n]["txy"], r[n]["tz"], r[n]["wgs"], r[n]["rw"]) for n in ("headline", "pop1_M50", "pop6_M50", "pop11_M50", "pop19_M128", "triclinic")}) == 6
    assert r["mostly_empty"]["full"] == 0 and r["mostly_empty"]["occupied"] == 6400
    assert r["full_at_98pc"]["full"] == 1 and r["not_full_below_98pc"]["full"] == 0
    assert r["headline"]["mid"] > r["orthogonal_far_origin"]["mid"] and r["headline"]["mid"] > r["triclinic"]["mid"]  # (wider bands: each branch of the bound)
    # launch geometry
    for tag, sl in (("none_listed", 0), ("some_listed", 1), ("unknown_listed", 1)):
        assert r["launch_all_" + tag]["tiles"] == ALL and r["launch_all_" + tag]["slice_pass"] == sl
        a, b, w = r["launch_list_standby_" + tag], r["launch_list_whole_" + tag], r["launch_window_" + tag]
        assert a["tiles"] == LIST and a["standby"] == 1 and a["grid"] == 8 * a["per"] < a["ntiles"] and a["slice_pass"] == sl
        assert b["tiles"] == LIST and b["standby"] == 0 and b["grid"] >= b["ntiles"] and b["slice_pass"] == sl
        assert w["tiles"] == WINDOW and w["standby"] == 0 and w["slice_pass"] == sl
        for d in (a, b, w):
            assert (d["list_cap"], d["mop_tile_z"], d["mop_nt2"]) == ((d["ntiles"] * d["tz"], 1, d["nt2"] * d["tz"]) if sl else (d["ntiles"], d["tz"], d["nt2"]))
    w = r["launch_window_some_listed"]  # planes [8, 20) in tiles of 4: tile planes 2, 3, 4
    assert (w["tile_base"], w["nt0_run"], w["grid"]) == (2 * w["nt1"] * w["nt2"], 3, 8 * w["per"]) and w["per"] * 8 >= 3 * w["nt1"] * w["nt2"]
    assert (r["launch_window_centre_inside"]["nt0_run"], r["launch_window_centre_inside"]["cen_lo"], r["launch_window_centre_inside"]["cen_hi"]) == (2, 10, 14)
    assert r["launch_window_centre_one_plane"]["nt0_run"] == 1 and r["launch_window_one_plane"]["nt0_run"] == 1
    assert (r["launch_window_some_listed"]["cen_lo"], r["launch_window_some_listed"]["cen_hi"]) == (0, 0x7FFFFFFF)
    assert r["launch_window_on_a_full_grid"]["tiles"] == ALL and r["launch_centre_without_window"]["tiles"] == LIST
    # the round-1 tiled plan
    assert r["triclinic"]["t_tile"] == 0
    assert r["tiled_M32"]["t_tile"] > 0 and r["tiled_M33"]["t_tile"] > 0 and r["tiled_M47"]["t_tile"] > 0 and r["tiled_M48"]["t_tile"] == 0
    assert r["tiled_6_periodic_cells"]["t_tile"] > 0 and r["tiled_6_periodic_cells"]["t_cellshift"] == 0
    assert r["tiled_7_periodic_cells"]["t_cellshift"] == 1 and r["tiled_6_open_cells"]["t_cellshift"] == 1
    assert r["tiled_full"]["t_full"] == 1 and r["tiled_one_cell_empty"]["t_full"] == 0 and r["tiled_one_cell_empty"]["t_occupied"] == 7999
    assert r["tiled_occupancy_unknown"]["t_full"] == 0 and r["tiled_occupancy_unknown"]["t_occupied"] == 8000
    assert r["tiled_pop_too_high"]["t_tile"] == 0


def test_memo_hands_out_the_right_plan():
    """Through the thread's memo, as a build goes: twice the same inputs, then inputs that differ in ONE statistic (enough for another
    instance), then the first again; and a refusal between two plans.  mdh_debug_neighbor_plan reports each."""
    a, b, refused = TABLE["M16_runs_of_29_0.1pc"], TABLE["M16_runs_of_29_0.3pc"], TABLE["refuse_long_runs"]
    one = dict(a, stats=[(k, v + (16 if k == 1 + 29 else 0)) for k, v in a["stats"]])  # 8 -> 24 runs of 29: the wide instance
    ra, rb = RECORDED["M16_runs_of_29_0.1pc"][1], RECORDED["M16_runs_of_29_0.3pc"][1]
    plan8 = np.zeros(8, np.int32)
    for c, want in ((a, ra), (a, ra), (one, None), (a, ra), (b, rb), (refused, RECORDED["refuse_long_runs"][1]), (b, rb), (a, ra)):
        got = run(c, memo=1)
        if want is None:  # (one statistic off the recorded case: the same tile as b's, the wide instance)
            assert same(got, run(one)) is None and named(got)["tk8"] == 0 and named(got)["lds_bytes"] == named(rb)["lds_bytes"]
            want = got
        assert same(got, want) is None
        assert _lib.lib().mdh_debug_neighbor_plan(plan8.ctypes.data) == 0
        assert plan8.tolist()[:4] == [int(want[15 + k]) for k in range(4)] and plan8[5] == want[20] and plan8[6] == want[21] and plan8[7] == want[22]
        assert (plan8[4] & ~256 if plan8[0] > 0 else plan8[4]) == want[19]  # (bit 8: the last cell grid's form, not the plan's)
        _lib.lib().mdh_debug_neighbor_plan(plan8.ctypes.data)
        assert plan8[7] == 0  # read once


def budget(wgs):
    return 160 * 1024 // wgs - 1088 - (64 if wgs == 4 else 1600)


def check_properties(tag, c, out):
    """What the kernel's comments promise of any plan."""
    d = named(out)
    if d["txy"] == 0:
        assert d["reason"] in (-1, -3, -4, -5, -6, -7), tag
        return None
    txy, tz, rc = int(d["txy"]), int(d["tz"]), c["d"][15]
    assert d["reason"] == 0 and 1 <= txy <= 8 and 1 <= tz <= 24, tag
    assert (txy + 2) ** 2 * (tz + 2) <= 256, tag               # one halo cell per thread
    assert 64 <= d["cap"] <= 2040, tag                         # a centre's LDS index takes 11 bits
    assert 1 <= d["wgs"] <= (4 if d["tk8"] else 3) and d["lds_bytes"] <= budget(int(d["wgs"])), tag
    assert d["rw"] % 4 == 0 and 8 <= d["rw"] <= 64 and (d["rw"] == 64 or not d["tk8"]), tag
    assert d["mid"] < rc * rc and d["T"] > 0 and d["T"] > rc * rc - d["mid"], tag  # mid <= rc^2 - tol, T >= (rc^2 - mid) + tol, tol > 0
    assert _lib.lib().mdh_debug_run_offset_table(txy, tz, np.zeros(3, np.uint32).ctypes.data) == 0, tag  # a shape the run table is proved for
    return txy, tz


def test_properties_of_every_plan():
    """... over the table, and over a sweep of populations and row widths that reaches many of the shapes
    test_run_offset_table_reproduces_run_cell (test_gpu_tile_front.py) enumerates."""
    for name, c in TABLE.items():
        check_properties(name, c, run(c))
    shapes = set()
    for M, count in ((1, 1), (8, 0), (16, 0), (24, 0), (50, 0), (64, 0), (65, 0), (128, 0)):
        for tri in (0, 1):
            for occupied in (64000, 6400):
                for k in range(60):
                    pop = 0.05 * 1.13**k  # 0.05 ... 68 atoms per cell
                    N = max(1, int(pop * occupied))
                    length = min(97, round(3 * pop))
                    c = case((40, 40, 40), N, M, count=count, tri=tri, stats=[(0, occupied), (1 + length, 64000)])
                    shapes.add(check_properties((M, tri, occupied, pop), c, run(c)))
    shapes.discard(None)
    assert len(shapes) >= 12, sorted(shapes)


def test_header_builds_with_a_plain_host_compiler_and_its_program_passes():
    """neighbor_plan.hpp has no HIP in it: tests/native/neighbor_plan_host.cpp — its own main, the header, this table — compiles with
    the host compiler alone and reproduces the recording.  (The same program is what one builds with -fsanitize=address,undefined.)"""
    src = os.path.join(HERE, "native", "neighbor_plan_host.cpp")
    exe = os.path.join(HERE, "native", "_build", "neighbor_plan_host")
    os.makedirs(os.path.dirname(exe), exist_ok=True)
    subprocess.check_call(["g++", "-O1", "-std=c++17", "-Wall", "-ffp-contract=off", "-o", exe, src])
    done = subprocess.run([exe, GOLDEN], capture_output=True, text=True)
    assert done.returncode == 0, done.stdout + done.stderr
    assert f"{len(TABLE)} cases" in done.stdout, done.stdout
