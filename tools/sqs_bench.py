"""Times the SQS search (mdapy_amd/_sqs.py, csrc/sqs.hip) and writes profiles/sqs.md.

Cells: the 256-atom three-element fcc cell at cutoffs {2: 4.0, 3: 3.0} and the 108-atom five-element fcc cell at
{2: 4.0, 3: 3.0, 4: 3.0}.  Per n_replicas in 1, 64, 256, 1024, 4096: wall time of one ``run_mc`` of --steps steps (tables up,
every launch, results down; the call synchronises), swap attempts per second per chain and in total, and the best objective
reached.  Once per kernel, from ``hipcc -Rpass-analysis=kernel-resource-usage``: registers, spills, occupancy; per cell the LDS a
replica takes and how many replicas a CU holds.  Also the library's launch bound and the time of one launch of that many steps.

Usage: python tools/sqs_bench.py [--steps 100000] [--replicas 1 64 256 1024 4096] [--out profiles/sqs.md] [--isa-only]"""
import argparse
import json
import os
import re
import subprocess
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
LAUNCH_STEPS = 4096  # SQS_LAUNCH_STEPS of csrc/sqs.hip
CU_LDS, CU_WAVES = 160 * 1024, 32  # per CU: LDS bytes, wave slots (8 on each of 4 SIMDs)
CELLS = (
    ("fcc 4x4x4, 3 elements", "fcc", 3.6, 4, ("A", "B", "C"), {2: 4.0, 3: 3.0}),
    ("fcc 3x3x3, 5 elements", "fcc", 3.55, 3, ("Fe", "Ni", "Co", "Mn", "Cr"), {2: 4.0, 3: 3.0, 4: 3.0}),
)


def resource_usage():
    """{kernel: {VGPRs, SGPRs, VGPR spill, SGPR spill, scratch, occupancy}} from the compiler's remarks; needs no device"""
    src = os.path.join(ROOT, "mdapy_amd", "csrc", "sqs.hip")
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    with tempfile.TemporaryDirectory() as tmp:
        done = subprocess.run([hipcc, "-O3", "-std=c++17", "--offload-arch=gfx950", "-ffp-contract=off", "--cuda-device-only", "-c",
                               "-Rpass-analysis=kernel-resource-usage", src, "-o", os.path.join(tmp, "sqs.o")], stderr=subprocess.PIPE, text=True, check=True)
    found, name = {}, None
    fields = {"VGPRs": "vgprs", "TotalSGPRs": "sgprs", "VGPRs Spill": "vgpr_spill", "SGPRs Spill": "sgpr_spill",
              "ScratchSize [bytes/lane]": "scratch", "Occupancy [waves/SIMD]": "occupancy"}
    for line in done.stderr.splitlines():
        if "Function Name:" in line:
            m = re.search(r"Function Name: _ZN3mdh\d+(k_sqs_\w+?)E", line)
            name = m.group(1) if m else None
            if name:
                found[name] = {}
        m = re.search(r"remark:\s+([A-Za-z \[\]/]+): (\d+)", line)
        if m and name in found and m.group(1).strip() in fields:
            found[name][fields[m.group(1).strip()]] = int(m.group(2))
    return found


def lds_per_replica(N, G, C, H):
    return 16 * C + 4 * H + 4 * ((G + 31) // 32) + 2 * ((N + 7) & ~7)


def build(structure, a, n, elements, cutoffs):
    """(engine, types) of a cell — the engine filled as SQS.compute fills it"""
    import mdapy_amd as mp
    from mdapy_amd.build_lattice import lattice_positions

    pos, box = lattice_positions(structure, a, n, n, n)
    alloy = mp.build_hea_fromsystem(mp.System(pos=pos, box=box), elements, (1.0 / len(elements),) * len(elements), 1)
    sqs = mp.SQS(alloy, cutoffs=cutoffs, max_steps=0).compute()
    return sqs._engine, sqs._best_types.tolist()


def main():
    p = argparse.ArgumentParser()
    p.add_argument("--steps", type=int, default=100000)
    p.add_argument("--replicas", type=int, nargs="+", default=[1, 64, 256, 1024, 4096])
    p.add_argument("--out", default=os.path.join(ROOT, "profiles", "sqs.md"))
    p.add_argument("--isa-only", action="store_true")
    args = p.parse_args()
    usage = resource_usage()
    print(json.dumps({"isa": usage}), flush=True)
    if args.isa_only:
        return
    from mdapy_amd import _lib

    if _lib.device_count() < 1:
        raise RuntimeError("sqs_bench needs a HIP device")
    T, seed = 0.02, 1
    out = ["# SQS search on one MI355X (`sqs.hip`, `tools/sqs_bench.py`)", "",
           f"`python tools/sqs_bench.py --steps {args.steps}`: one `run_mc` per row (tables up, the shuffle, every launch of "
           f"{LAUNCH_STEPS} steps, the winner, results down; the call ends in a device synchronise), T = {T}, seed {seed}, after a "
           "warm-up call of one launch.  A swap attempt is one step of one chain, the skipped ones (i = j or equal species) included.  "
           "There is no threshold; these are the first numbers, and no CPU figure stands beside them: the reference's engine was not run.", ""]
    for title, structure, a, n, elements, cutoffs in CELLS:
        engine, types = build(structure, a, n, elements, cutoffs)
        N, m, I, G, C, H = (int(v) for v in engine._model["dims"][:6])
        lds = lds_per_replica(N, G, C, H)
        taken = lds
        resident = min(CU_WAVES * usage.get("k_sqs_steps", {}).get("occupancy", 8) // 8, CU_LDS // taken)
        touched = float(np.diff(engine._model["a2i_off"]).mean())
        head = {"cell": title, "N": N, "species": m, "cutoffs": {str(k): v for k, v in cutoffs.items()}, "instances": I, "groups": G, "channels": C,
                "histogram_bins": H, "instances_per_atom": touched, "lds_per_replica": lds, "replicas_per_cu": resident}
        print(json.dumps(head), flush=True)
        out += [f"## {title}, cutoffs {cutoffs}", "",
                f"{N} atoms, {I} instances in {G} groups ({touched:.0f} per atom: a swap touches up to twice that), {C} channels, {H} histogram "
                f"bins.  One replica takes {lds} bytes of LDS: {resident} replicas resident per CU "
                f"(the smaller of {CU_LDS // taken} by LDS and {CU_WAVES * usage.get('k_sqs_steps', {}).get('occupancy', 8) // 8} by wave slots), "
                f"{256 * resident} on 256 CUs.", ""]
        engine.run_mc(types, LAUNCH_STEPS, T, 64, seed)  # warm-up
        laps = []
        for R in (1, 256, 4096):
            t0 = time.perf_counter()
            engine.run_mc(types, LAUNCH_STEPS, T, R, seed)
            laps.append((R, time.perf_counter() - t0))
            print(json.dumps({"cell": title, "one_launch_steps": LAUNCH_STEPS, "n_replicas": R, "ms": 1e3 * laps[-1][1]}), flush=True)
        out += [f"One call of a single launch of {LAUNCH_STEPS} steps (the library's bound), everything around it included: "
                + ", ".join(f"{1e3 * s:.1f} ms with {R} replicas" for R, s in laps) + ".", "",
                "| n_replicas | wall s | attempts / s per chain | attempts / s in total | best objective |", "|---|---|---|---|---|"]
        for R in args.replicas:
            t0 = time.perf_counter()
            _, best, _ = engine.run_mc(types, args.steps, T, R, seed)
            s = time.perf_counter() - t0
            row = {"cell": title, "n_replicas": R, "steps": args.steps, "wall_s": s, "attempts_per_s_chain": args.steps / s,
                   "attempts_per_s_total": args.steps * R / s, "best_objective": best}
            print(json.dumps(row), flush=True)
            out.append(f"| {R} | {s:.3f} | {args.steps / s:.3e} | {args.steps * R / s:.3e} | {best:.5f} |")
        out.append("")
    out += ["## Resource usage (`hipcc -Rpass-analysis=kernel-resource-usage`, gfx950)", "",
            "| kernel | VGPRs | SGPRs | VGPR spills | SGPR spills | scratch B/lane | occupancy waves/SIMD |", "|---|---|---|---|---|---|---|"]
    for name, u in usage.items():
        out.append(f"| `{name}` | {u.get('vgprs')} | {u.get('sgprs')} | {u.get('vgpr_spill')} | {u.get('sgpr_spill')} | {u.get('scratch')} | {u.get('occupancy')} |")
    out += ["", "LDS is dynamic (the compiler reports 0): the bytes per replica are given with each cell above.  A workgroup is one wavefront."]
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write("\n".join(out) + "\n")
    print(json.dumps({"written": args.out}), flush=True)


if __name__ == "__main__":
    main()
