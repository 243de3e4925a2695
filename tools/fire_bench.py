"""Times the FIRE minimizer on the EAM bench's frame (tools/eam_bench.py, case "three"): fcc, 100^3 cells (4 000 000 atoms), N(0, 0.05 A)
rattle, Ni / Co / Cr at random, under tests/golden/eam/NiCoCr.lammps.eam.gz (rc 5.88 A).  One JSON line per figure:

  resources  VGPRs / SGPRs / LDS / scratch of the kernels of csrc/fire.hip (hipcc -Rpass-analysis=kernel-resource-usage); --isa-only stops here
  hbm        ``FIRE(system).run(--steps, fmax=0, show_process=False)`` on the HBM path, with and without ``optimize_cell``: the time per
             step (a run of its own after a warm-up run of two steps, ending in a device synchronise), and from a second run under the
             library's event pairs (mdh_prof_*) the step's kernels in three groups — the list build, the EAM passes, FIRE's own
             (``k_fire_*``) — with the bytes FIRE's kernels move per step and their bytes per second beside the copy ceiling
  host       the host path (``device=False``) of the same class on the same frame, --host-steps steps

Usage: python tools/fire_bench.py [--cells 100] [--steps 10] [--host-steps 3] [--isa-only] [--no-host]"""
import argparse
import ctypes
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
A = 3.615
HBM_COPY = 6.29e12  # bytes per second: what a float4 copy reaches on an MI355X (profiles/eam.md)
# bytes per row (24 an (n, 3) pass, 8 a column) FIRE's kernels move in a downhill step: dots reads v, f; kick reads v, f, writes v; mix
# the same; move reads v, writes dr, reads and writes the positions (columns, or the unstrained rows)
ROW_BYTES = {"k_fire_dots": 48, "k_fire_kick": 72, "k_fire_mix": 72, "k_fire_move": 96, "k_fire_rowmat": 48}


def resources():
    src = os.path.join(ROOT, "mdapy_amd", "csrc", "fire.hip")
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    with tempfile.TemporaryDirectory() as tmp:
        done = subprocess.run([hipcc, "-O3", "-std=c++17", "--offload-arch=gfx950", "-ffp-contract=off", "--cuda-device-only", "-c",
                               "-Rpass-analysis=kernel-resource-usage", src, "-o", os.path.join(tmp, "fire.o")],
                              stderr=subprocess.PIPE, text=True, check=True)
    table, name = {}, None
    keys = {"TotalSGPRs": "sgprs", "VGPRs": "vgprs", "ScratchSize [bytes/lane]": "scratch_bytes_per_lane",
            "Occupancy [waves/SIMD]": "waves_per_simd", "LDS Size [bytes/block]": "lds_bytes"}
    for line in done.stderr.splitlines():
        m = re.search(r"remark:\s+(.*?):\s+(\S+) \[-Rpass", line)
        if not m:
            continue
        if m.group(1) == "Function Name":
            name = re.sub(r"^_ZN3mdh\d+(k_\w+?)E.*$", r"\1", m.group(2))
            table[name] = {}
        elif name and m.group(1) in keys:
            table[name][keys[m.group(1)]] = int(m.group(2))
    return table


def main():
    p = argparse.ArgumentParser()
    p.add_argument("--cells", type=int, default=100)
    p.add_argument("--steps", type=int, default=10)
    p.add_argument("--host-steps", type=int, default=3)
    p.add_argument("--isa-only", action="store_true")
    p.add_argument("--no-host", action="store_true")
    args = p.parse_args()
    print(json.dumps({"resources": resources()}), flush=True)
    if args.isa_only:
        return
    import torch

    import mdapy_amd as mp
    from mdapy_amd import _lib
    from mdapy_amd.build_lattice import lattice_positions
    from mdapy_amd.devarray import HArray
    from mdapy_amd.frame import Frame

    if not torch.cuda.is_available():
        raise RuntimeError("fire_bench needs a HIP device")
    L = _lib.lib()
    eam = mp.EAM(os.path.join(ROOT, "tests", "golden", "eam", "NiCoCr.lammps.eam.gz"))
    pos, box = lattice_positions("fcc", A, args.cells, args.cells, args.cells)
    cell = np.array(box, float)[:3]
    rng = np.random.default_rng(0)
    pos = pos + rng.normal(0, 0.05, pos.shape)
    n = len(pos)
    names = np.array(["Ni", "Co", "Cr"], dtype=object)[rng.integers(0, 3, n)]
    element = Frame({"element": names})["element"]  # (one column object for every System: the calculator codes it once)

    def system():
        cols = {c: HArray(torch.from_numpy(np.ascontiguousarray(pos[:, k])).cuda()) for k, c in enumerate("xyz")}
        s = mp.System(data=Frame({**cols, "element": element}), box=cell)
        s.calc = eam
        return s

    def timed(fn):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        return 1e3 * (time.perf_counter() - t0)

    def kernel_times(fn):
        torch.cuda.synchronize()
        L.mdh_prof_reset()
        L.mdh_prof_enable(1)
        fn()
        torch.cuda.synchronize()
        L.mdh_prof_enable(0)
        buf = ctypes.create_string_buffer(1 << 16)
        L.mdh_prof_report(buf, len(buf))
        out = {}
        for line in buf.value.decode().strip().splitlines():
            name, count, total = line.split()
            out[name] = (int(count), float(total))
        return out

    for kwargs in (dict(), dict(optimize_cell=True)):
        mp.FIRE(system(), **kwargs).run(2, fmax=0, show_process=False)  # warm-up: code objects, the allocator's blocks
        s = system()
        fire = mp.FIRE(s, **kwargs)
        ms = timed(lambda: fire.run(args.steps, fmax=0, show_process=False))
        out = {"case": "hbm", "atoms": n, "optimize_cell": bool(kwargs), "steps": args.steps, "on_hbm_path": bool(fire._hbm),
               "ms_per_step": ms / args.steps}
        s = system()
        fire = mp.FIRE(s, **kwargs)
        ranges = kernel_times(lambda: fire.run(args.steps, fmax=0, show_process=False))
        groups = {"fire": 0.0, "eam": 0.0, "list_build": 0.0}
        for name, (count, total) in ranges.items():
            groups["fire" if name.startswith("k_fire") else "eam" if name.startswith(("k_eam", "k_column_sums9")) else "list_build"] += total
        out["kernel_ms_per_step"] = {k: v / args.steps for k, v in groups.items()}
        out["fire_kernels_ms_per_call"] = {k: t / c for k, (c, t) in ranges.items() if k.startswith("k_fire")}
        out["fire_kernel_calls"] = {k: c for k, (c, t) in ranges.items() if k.startswith("k_fire")}
        rows = n + (3 if kwargs else 0)
        moved = sum(ROW_BYTES.get(k, 0) * rows * c for k, (c, t) in ranges.items() if k.startswith("k_fire"))
        out["fire_bytes_per_step"] = moved / args.steps
        out["fire_bytes_per_second"] = moved / (groups["fire"] * 1e-3) if groups["fire"] else None
        out["share_of_copy_ceiling"] = out["fire_bytes_per_second"] / HBM_COPY if groups["fire"] else None
        out["added_to_list_build_plus_eam"] = groups["fire"] / (groups["eam"] + groups["list_build"])
        print(json.dumps(out), flush=True)

    if not args.no_host:
        s = system()
        fire = mp.FIRE(s, device=False)
        fire.run(1, fmax=0, show_process=False)
        ms = timed(lambda: fire.run(args.host_steps, fmax=0, show_process=False))
        print(json.dumps({"case": "host", "atoms": n, "steps": args.host_steps, "on_hbm_path": bool(fire._hbm),
                          "ms_per_step": ms / args.host_steps}), flush=True)


if __name__ == "__main__":
    main()
