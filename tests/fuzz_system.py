#!/usr/bin/env python
"""Randomised System-level parity sweep on the GPU box: the same random call sequence on a random system, once
through the HIP library and once with the host classes routed to the CPU oracle (tests/_oracle_backend.py), then
every per-atom column and every returned curve compared.

    python tests/fuzz_system.py [seconds] [first_seed]

FUZZ_TWIN=1: the HIP side is analysed on System's cell-sorted twin (forced, whatever the size and order of the system).

The tool runs the ``extended`` plan — the entries ``bond``, ``adf``, ``chill``, ``strain`` and ``ws`` of ``consumer_calls`` beside the
old ones, the oracle side with the numpy restatements of tests/_bond_ref.py, _chill_ref.py, _strain_ref.py and _ws_ref.py — and
draws every third system from ``fuzz_parity.draw_water``.  ``plan(s)`` without ``extended`` is what tests/test_gpu_fuzz.py pins.

This exercises the policy layer above the C ABI as well (small-box replication, list reuse, triclinic alignment of
the Voronoi calls, column naming).  Integer columns must be equal, floating ones agree to 1e-6; the two strain columns are equal
bit for bit, and the CHILL+ labels follow the rule of tests/_chill_ref.py on the HIP system's own list.  Test infrastructure.
"""
import os
import sys
import time
import traceback

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np
from _pytest.monkeypatch import MonkeyPatch

import _oracle_backend as ob
import mdapy_amd as mp
from mdapy_amd import devarray
import fuzz_parity as FP
from fuzz_parity import draw, draw_water
from oracle import oracle as O

ELEMENTS = ["Al", "Cu", "Fe", "Ni"]  # (make_system hands out Al and Cu; an ADF call of more than 32 patterns relabels with all four)


def make_system(s):
    rng = np.random.default_rng(s["seed"] + 3)
    box = mp.Box(s["box"], origin=s["origin"], boundary=s["bnd"])
    sysm = mp.System(pos=s["pos"], box=box)
    n = sysm.N
    cols = dict(type=rng.integers(1, 3, n).astype(np.int32), vx=rng.normal(0, 3, n), vy=rng.normal(0, 3, n), vz=rng.normal(0, 3, n),
                element=rng.choice(["Cu", "Al"], n))
    sysm.update_data(sysm.data.with_columns(**cols))
    return sysm


class Result(dict):
    """what one of the calls below leaves for the comparison: named arrays (``curves`` reads them) and notes in ``info``"""

    def __init__(self, info=None, **arrays):
        super().__init__(arrays)
        self.info = info or {}


def _box_of(y, cell=None):
    return mp.Box(np.asarray(y.box.box, float)[:3] if cell is None else cell, boundary=y.box.boundary, origin=y.box.origin)


def _positions(y):
    return np.column_stack([y.data[c].to_numpy() for c in "xyz"])


def consumer_calls(s, rc):
    """the entries of the extended plan: bond / angular distribution, CHILL+, atomic strain, Wigner-Seitz.  Every random choice
    comes from a generator seeded by the system's seed — those made at call time (from the positions the system has THEN, so that
    a frame made after ``replicate`` has its N) from a fresh one inside the call — so the HIP and the oracle side get the same
    arguments.  None of the five is left out for a kind of box or boundary: the reference's pbc() of a position difference, its
    cutoff list and its nearest-site wrap are defined for sheared, rotated, open and unwrapped systems alike."""
    seed = s["seed"]
    rng = np.random.default_rng(seed + 11)
    water = bool(s.get("water"))
    Q = dict(bond_nbin=FP.draw_nbin(rng), adf_nbin=FP.draw_nbin(rng), adf_many=rng.random() < 0.25, adf_wide=rng.random() < 0.3,
             adf_absent=rng.random() < 0.1, chill_rc=float(rng.uniform(3.2, 3.8)) if water else rc,
             affine=bool(rng.integers(0, 2)), ws_affine=bool(rng.integers(0, 2)))

    def bond(y):
        job = y.cal_bond_analysis(rc, Q["bond_nbin"])
        return Result(bond_length_distribution=job.bond_length_distribution, bond_angle_distribution=job.bond_angle_distribution,
                      r_length=job.r_length, r_angle=job.r_angle)

    def adf(y):
        r = np.random.default_rng(seed + 13)
        names, nbin = ELEMENTS[:2], Q["adf_nbin"]
        # The numpy yardstick walks every pair of slots once per pattern: no long pattern table on an inherited list of rows wider
        # than 48 columns (so more than BA_PAT patterns are swept on narrow rows only; wide rows get the short tables).  Decided
        # once, by the first of the two systems that comes here, and kept for the other: both get the same arguments.
        if "long" not in Q:
            Q["long"] = Q["adf_many"] and not ("verlet_list" in y.__dict__ and y.verlet_list.shape[1] > 48)
        if Q["long"]:  # more patterns than two elements can name: relabel (both sides alike; later calls inherit the column)
            names = ELEMENTS
            y.update_data(y.data.with_columns(element=r.choice(names, y.N)))
            if Q["adf_wide"]:
                nbin = 263  # the first launch of 32 patterns has 32 x 263 bins: beyond the 8192 of BA_HIST_LDS (257 is the first)
        elif Q["adf_wide"]:
            nbin = 2050  # five or six patterns of them
        triples, ranges, kinds = FP.draw_patterns(r, list(range(len(names))), rc, len(names) > 2, 5 if Q["adf_wide"] else 1)
        rc_dict = {"-".join(names[c] for c in t): list(map(float, b)) for t, b in zip(triples, ranges)}
        if Q["adf_absent"]:  # an element the system lacks: refused by both sides (which ends the sequence)
            rc_dict["Al-Zr-Al"] = [0.0, rc, 0.0, rc]
        job = y.cal_angular_distribution_function(rc_dict, nbin)
        return Result(dict(kinds=kinds, nbin=nbin), bond_angle_distribution=job.bond_angle_distribution, r_angle=job.r_angle)

    def chill(y):
        y.cal_chill_plus(Q["chill_rc"])
        return Result(dict(cutoff=Q["chill_rc"]))

    def strain(y):
        r = np.random.default_rng(seed + 17)
        grad = FP.deformation(r)
        cell = np.asarray(y.box.box, float)[:3]
        cur = mp.System(pos=_positions(y) @ grad + r.normal(0, 0.03, (y.N, 3)),
                        box=mp.Box(cell @ grad, boundary=y.box.boundary, origin=np.asarray(y.box.origin, float) @ grad))
        job = mp.AtomicStrain(rc, y, Q["affine"], max_neigh=None)
        job.compute(cur)
        info = dict(affine=Q["affine"], replica="_enlarge_data" in y.__dict__, twin=job._reference()[4] is not None)
        return Result(info, shear_strain=cur.data["shear_strain"].to_numpy(), volumetric_strain=cur.data["volumetric_strain"].to_numpy())

    def ws(y):
        r = np.random.default_rng(seed + 19)
        pos, cell = _positions(y), np.asarray(y.box.box, float)[:3]
        keep = r.random(y.N) < 0.97
        keep[int(r.integers(0, y.N))] = True
        added = r.random((int(r.integers(1, 6)), 3)) @ cell + np.asarray(y.box.origin, float)
        pos = np.vstack([pos[keep] + r.normal(0, 0.15, (int(keep.sum()), 3)), added])
        if not s["tri"]:  # the plain kinds: a scaled box as well
            scale = np.diag(r.uniform(0.97, 1.03, 3))
            pos, cell = pos @ scale, cell @ scale
        cur = mp.System(pos=pos, box=mp.Box(cell, boundary=y.box.boundary, origin=y.box.origin))
        return Result(**mp.WignerSeitzAnalysis(y, Q["ws_affine"]).compute(cur))

    # (CHILL+ not on unrattled metal crystals, where the reference's c is rounding noise: fuzz_parity.chill_defined)
    return [("bond", bond), ("adf", adf)] + ([("chill", chill)] if FP.chill_defined(s) else []) + [("strain", strain), ("ws", ws)]


def plan(s, extended=False):
    """the call sequence of one seed: (label, callable(system) -> object with curves or None).  ``extended``: the entries of
    ``consumer_calls`` join the table before the permutation (the default gives the sequences it always gave)"""
    rng = np.random.default_rng(s["seed"] + 5)
    rc = float(rng.uniform(2.8, 4.8))
    ortho = not np.any(s["box"] - np.diag(np.diag(s["box"])))
    P = dict(csp_n=int(rng.choice([8, 12])), ent_local=bool(rng.integers(0, 2)), ent_avg=float(rng.choice([0.0, rc * 0.8])),
             cl_rc=float(rng.uniform(1.5, 3.2)), st_avg=bool(rng.integers(0, 2)), nbin=int(rng.integers(20, 120)),
             rdf_long=float(rng.uniform(5.0, 9.0)), sf_kmax=float(rng.uniform(3.0, 6.0)), sf_partial=bool(rng.integers(0, 2)),
             sf_rc=float(rng.uniform(6.0, 9.0)), vw=bool(rng.integers(0, 2)),
             rep=[int(v) for v in rng.permutation([2, 1, 1])])
    calls = [
        ("neighbor", lambda y: y.build_neighbor(rc)),
        ("cna_rc", lambda y: y.cal_common_neighbor_analysis(rc=min(rc, 3.6))),
        ("cna_adaptive", lambda y: y.cal_common_neighbor_analysis()),
        ("csp", lambda y: y.cal_centro_symmetry_parameter(P["csp_n"])),
        ("ids", lambda y: y.cal_identify_diamond_structure()),
        ("aja", lambda y: y.cal_ackland_jones_analysis()),
        ("cnp", lambda y: y.cal_common_neighbor_parameter(min(rc, 3.5))),
        ("entropy", lambda y: y.cal_structure_entropy(rc, 0.2, P["ent_local"], P["ent_avg"])),
        ("temperature", lambda y: y.cal_atomic_temperature(rc)),
        ("cluster", lambda y: y.cal_cluster_analysis(P["cl_rc"])),
        ("cluster_by_type", lambda y: y.cal_cluster_analysis({"1-1": 2.9, "1-2": 2.4, "2-2": 2.0})),
        ("steinhardt_nnn", lambda y: y.cal_steinhardt_bond_orientation([4, 6], nnn=12, average=P["st_avg"], wl=True, wlhat=True)),
        ("steinhardt_rc", lambda y: y.cal_steinhardt_bond_orientation([6, 8], rc=rc, identify_liquid=True)),
        ("rdf", lambda y: y.cal_radial_distribution_function(rc, P["nbin"])),
        ("rdf_long", lambda y: y.cal_radial_distribution_function(P["rdf_long"], 60)),
        ("wcp", lambda y: y.cal_warren_cowley_parameter(rc)),
        ("sfc_direct", lambda y: y.cal_structure_factor(0.5, P["sf_kmax"], 40, cal_partial=P["sf_partial"], mode="direct")),
        ("wrap", lambda y: y.wrap_pos()),
        ("replicate", lambda y: y.replicate(*P["rep"])),
        ("average", lambda y: y.average_by_neighbor(rc * 0.8, "vx", include_self=P["st_avg"])),
        ("sfc_debye", lambda y: y.cal_structure_factor(0.5, 8.0, 50, mode="debye", rc=P["sf_rc"])),
    ]
    if extended:
        calls += consumer_calls(s, rc)
    if not s["unwrapped"] and not s.get("water"):  # (the water draws are for the list consumers: PTM and Voronoi keep to draw's kinds)
        if s["sigma"] != 0.0:
            calls.append(("ptm", lambda y: y.cal_polyhedral_template_matching("default", return_rmsd=True, return_ordering=True, return_atomic_distance=True)))
            calls.append(("ptm_faults", lambda y: y.cal_polyhedral_template_matching("fcc-hcp-bcc", identify_fcc_planar_faults=True)))
        if O.have_voro_ref() and s["kind"] not in ("blob", "tiny") and (ortho or all(s["bnd"])):
            calls.append(("voronoi_volume", lambda y: y.cal_voronoi_volume()))
            if all(s["bnd"]):
                calls.append(("steinhardt_voronoi", lambda y: y.cal_steinhardt_bond_orientation([6], use_voronoi=True, use_weight=P["vw"])))
    order = rng.permutation(len(calls))[: int(rng.integers(4, 9))]
    return [calls[i] for i in order]


EXACT = ("shear_strain", "volumetric_strain")  # bitwise, NaN for NaN, as tests/test_gpu_strain.py has it
WS_KEYS = ("site_occupancy", "atom_site_index", "atom_site_type", "atom_occupancy", "vacancy_count", "interstitial_count")


def curves(obj):
    out = {}
    if obj is None:
        return out
    for name in ("g_total", "g", "r", "Npair", "WCP", "k", "Sk", "Sk_partial", "coordination", "bond_length_distribution",
                 "bond_angle_distribution", "r_length", "r_angle") + EXACT + WS_KEYS:
        v = obj.get(name) if isinstance(obj, dict) else getattr(obj, name, None)
        if v is None:
            continue
        if isinstance(v, dict):
            for kk, vv in v.items():
                out[f"{name}[{kk}]"] = np.asarray(vv)
        else:
            try:
                out[name] = np.asarray(v)
            except Exception:
                pass
    return out


def same(a, b, exact=False):
    a, b = np.asarray(a), np.asarray(b)
    if a.shape != b.shape:
        return False
    if exact:
        return bool(a.dtype == b.dtype and np.array_equal(a, b, equal_nan=True))
    if a.dtype.kind in "iub" or a.dtype.kind in "USO":
        return bool(np.array_equal(a, b))
    fin = np.isfinite(a)
    return bool(np.array_equal(fin, np.isfinite(b)) and np.allclose(a[fin], b[fin], rtol=1e-6, atol=1e-8))


def _watch_twin(system, seen):
    """note which System methods of ``system`` ran on its cell-sorted twin"""
    inner = system._run_on_twin

    def run(twin, name, args, kwargs):
        seen.add(name)
        return inner(twin, name, args, kwargs)

    system._run_on_twin = run


def _note_yardstick(label, result, system):
    """what the oracle side's results say about the sweep itself (tests/test_gpu_fuzz_consumers.py asserts it was not vacuous)"""
    FP._note("ran " + label)
    if label == "adf":
        FP.note_adf(result["bond_angle_distribution"], result.info["kinds"], result.info["nbin"])
    elif label == "bond":
        FP._note("bond lengths", int(result["bond_length_distribution"].sum()))
    elif label == "strain":
        FP._note("strain affine" if result.info["affine"] else "strain plain")
        FP._note("strain replica", int(result.info["replica"]))
    elif label == "ws":
        FP._note("ws vacancies", result["vacancy_count"])
        FP._note("ws interstitials", result["interstitial_count"])


def run_seed(seed, fails, extended=False, water=False, host_only=False):
    """``host_only``: the first system goes through the oracle and the restatements too (tests/test_fuzz_plans.py: the plans and the
    policy layer, the twin's included, on a machine without a GPU)"""
    s = draw_water(seed) if water else draw(seed)
    ran = 0
    try:
        calls = plan(s, extended)
    except Exception as e:
        fails.append((seed, "plan", repr(e)[:160]))
        return 0
    a, b = make_system(s), make_system(s)
    if os.environ.get("FUZZ_TWIN") == "1":  # the HIP side analysed on its cell-sorted twin whatever its size and order, the oracle side as it is
        a._sort_mode, b._sort_mode = "1", "0"
        on_twin = set()
        _watch_twin(a, on_twin)
    for label, fn in calls:
        if os.environ.get("FUZZ_TRACE"):
            print("  call", label, flush=True)
        res = []
        for which, sysm in (("hip", a), ("oracle", b)):
            patch = MonkeyPatch()
            try:
                if which == "oracle" or host_only:  # host classes -> oracle, output buffers -> numpy
                    ob.install(patch)
                    ob.install_consumers(patch)
                    patch.setattr(devarray, "_gpu", False)
                res.append(("ok", fn(sysm)))
            except Exception as e:
                res.append(("err", f"{type(e).__name__}: {str(e)[:140]}"))
            finally:
                patch.undo()
        if res[0][0] != res[1][0]:
            fails.append((seed, label, f"hip={res[0]} oracle={res[1]}"[:300]))
            break
        if res[0][0] == "err":
            if res[0][1].split(":")[0] != res[1][1].split(":")[0]:
                fails.append((seed, label, f"different errors: hip={res[0][1]} oracle={res[1][1]}"[:300]))
            break  # the same refusal on both sides ends the sequence
        # (the labels of CHILL+ live under the rule of tests/_chill_ref.py, below, not under equality)
        bad = [c for c in a.data.columns if c != "chill_plus" and (c not in b.data.columns or not same(a.data[c].to_numpy(), b.data[c].to_numpy()))]
        ca, cb = curves(res[0][1]), curves(res[1][1])
        bad += [f"curve {k}" for k in ca if k not in cb or not same(ca[k], cb[k], exact=k in EXACT)]
        bad += [f"curve {k} missing" for k in cb if k not in ca]
        if label == "chill":  # the yardstick on the HIP system's own list
            import _chill_ref

            want, _, ambiguous = _chill_ref.on_system_list(a, res[0][1].info["cutoff"])
            try:
                FP.chill_rule(a.data["chill_plus"].to_numpy(), want, ambiguous)
            except AssertionError as e:
                bad.append(f"chill_plus: {e}")
            if b.data["chill_plus"].to_numpy().shape != want.shape:
                bad.append("chill_plus: the oracle side has another number of atoms")
        if bad:
            fails.append((seed, label, "differs: " + ", ".join(bad)))
            if os.environ.get("FUZZ_DEBUG") and hasattr(a, "verlet_list") and hasattr(b, "verlet_list"):
                va, vb = np.asarray(a.verlet_list), np.asarray(b.verlet_list)
                print("   debug", seed, label, "lists", va.shape, vb.shape, "equal", va.shape == vb.shape and np.array_equal(va, vb),
                      "dist equal", np.array_equal(np.asarray(a.distance_list), np.asarray(b.distance_list)),
                      "nn equal", np.array_equal(np.asarray(a.neighbor_number), np.asarray(b.neighbor_number)),
                      "rc", getattr(a, "rc", None), getattr(b, "rc", None), "ncl", getattr(a, "cluster_number", None), getattr(b, "cluster_number", None), flush=True)
                if "cluster_id" in a.data.columns:
                    ca, cb = a.data["cluster_id"].to_numpy(), b.data["cluster_id"].to_numpy()
                    w = np.flatnonzero(ca != cb)
                    print("   debug ids: N", len(ca), "differ at", len(w), w[:8], "hip", ca[w[:8]], "oracle", cb[w[:8]], "hip min/max", ca.min(), ca.max(), "oracle min/max", cb.min(), cb.max(),
                          "nn of those", np.asarray(a.neighbor_number)[w[:8]], flush=True)
            break
        ran += 1
        if isinstance(res[1][1], Result):
            _note_yardstick(label, res[1][1], b)
            if os.environ.get("FUZZ_TWIN") == "1":
                used = {"bond": "cal_bond_analysis" in on_twin, "chill": "cal_chill_plus" in on_twin, "adf": "cal_angular_distribution_function" in on_twin,
                        "strain": res[0][1].info.get("twin", False)}.get(label, False)
                FP._note("twin " + label, int(bool(used)))
                on_twin.clear()
    return ran


def main():
    budget = float(sys.argv[1]) if len(sys.argv) > 1 else 120.0
    seed = int(sys.argv[2]) if len(sys.argv) > 2 else 1000
    t0 = time.time()
    fails, ran = [], 0
    while time.time() - t0 < budget:
        if os.environ.get("FUZZ_TRACE"):
            print("seed", seed, flush=True)
        try:
            ran += run_seed(seed, fails, extended=True, water=seed % 3 == 2)
        except Exception:
            fails.append((seed, "driver", traceback.format_exc()[-300:]))
        seed += 1
    print(f"fuzz_system: {ran} calls agreed over seeds up to {seed - 1}; {len(fails)} failures", flush=True)
    for f in fails[:60]:
        s = draw_water(f[0]) if f[0] % 3 == 2 else draw(f[0])
        print("  FAIL seed=%d call=%s %s  [kind=%s tri=%s unwrapped=%s bnd=%s N=%d]" % (f + (s["kind"], s["tri"], s["unwrapped"], s["bnd"].tolist(), len(s["pos"]))))
    return len(fails)


if __name__ == "__main__":
    sys.exit(min(main(), 100))
