"""Times the NEP calculator on the EAM bench's frame (tools/eam_bench.py): fcc, 100^3 cells (4 000 000 atoms), N(0, 0.05 A) rattle,
under tests/golden/nep/UNEP-v1.txt.gz (cutoffs 6 and 5 A), for a single-element assignment (every atom Ni) and a 3-element one
(random Al / Cr / Ni).  One JSON line per figure:

  resources  VGPRs / LDS / scratch of the kernels of csrc/nep.hip (hipcc -Rpass-analysis=kernel-resource-usage); --isa-only stops here
  first      System.get_energies() on a new System: the list build, the model's upload, the first launches, the results' download
  build      System.build_neighbor(rc) alone, median of --calls
  kernels    the raw shim on the list in HBM, results left in HBM — the whole call (median, best, worst of --calls after a warm-up
             call, each ending in a device synchronise) and its kernels' own times from the library's event pairs (mdh_prof_*: a
             run of its own): pass A is k_nep_descriptor, pass B is k_nep_pair (the table's writer) and k_nep_gather (its reader)
  pairs      list entries inside the radial and the angular cutoff, the (N, M, 3) table's size and the rate at which the gather
             reads it (two entries per pair: its own and the one on the way back)
  eam        EAM (tests/golden/eam/NiCoCr.lammps.eam.gz, rc 5.88 A; Al stands in as Co) on the same positions, the same way

Usage: python tools/nep_bench.py [--cells 100] [--calls 5] [--isa-only]"""
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


def resources():
    src = os.path.join(ROOT, "mdapy_amd", "csrc", "nep.hip")
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    with tempfile.TemporaryDirectory() as tmp:
        done = subprocess.run([hipcc, "-O3", "-std=c++17", "--offload-arch=gfx950", "-ffp-contract=off", "--cuda-device-only", "-c",
                               "-Rpass-analysis=kernel-resource-usage", src, "-o", os.path.join(tmp, "nep.o")],
                              stderr=subprocess.PIPE, text=True, check=True)
    table, name = {}, None
    keys = {"TotalSGPRs": "sgprs", "VGPRs": "vgprs", "AGPRs": "agprs", "ScratchSize [bytes/lane]": "scratch_bytes_per_lane",
            "Occupancy [waves/SIMD]": "waves_per_simd", "LDS Size [bytes/block]": "lds_bytes"}
    for line in done.stderr.splitlines():
        m = re.search(r"remark:\s+(.*?):\s+(\S+) \[-Rpass", line)
        if not m:
            continue
        if m.group(1) == "Function Name":
            width, flags = re.search(r"ILi(\d+)E", m.group(2)), re.findall(r"Lb([01])E", m.group(2))
            marks = ([width.group(1)] if width else []) + (["tri" if flags[0] == "1" else "ortho"] if flags else [])
            marks += ["charge"] if len(flags) > 1 and flags[1] == "1" else []  # (the instantiations csrc/nep_charge.hip launches)
            name = re.sub(r"^_ZN3mdh\d+(k_\w+?)(I|E).*$", r"\1", m.group(2)) + (f"<{', '.join(marks)}>" if marks else "")
            table[name] = {}
        elif name and m.group(1) in keys:
            table[name][keys[m.group(1)]] = int(m.group(2))
    return table


def main():
    p = argparse.ArgumentParser()
    p.add_argument("--cells", type=int, default=100)
    p.add_argument("--calls", type=int, default=5)
    p.add_argument("--isa-only", action="store_true")
    args = p.parse_args()
    print(json.dumps({"resources": resources()}), flush=True)
    if args.isa_only:
        return
    import torch

    import mdapy_amd as mp
    from mdapy_amd import _lib, kernels
    from mdapy_amd.build_lattice import lattice_positions
    from mdapy_amd.devarray import HArray
    from mdapy_amd.frame import Frame

    if not torch.cuda.is_available():
        raise RuntimeError("nep_bench needs a HIP device")
    L = _lib.lib()
    nep = mp.NEP(os.path.join(ROOT, "tests", "golden", "nep", "UNEP-v1.txt.gz"))
    eam = mp.EAM(os.path.join(ROOT, "tests", "golden", "eam", "NiCoCr.lammps.eam.gz"))

    def sync():
        torch.cuda.synchronize()

    def timed(fn):
        sync()
        t0 = time.perf_counter()
        fn()
        sync()
        return 1e3 * (time.perf_counter() - t0)

    def laps(fn):
        fn()  # warm-up
        ms = [timed(fn) for _ in range(max(args.calls, 1))]
        return {"ms": float(np.median(ms)), "ms_best": float(np.min(ms)), "ms_worst": float(np.max(ms)), "calls": len(ms)}

    def kernel_times(fn):
        sync()
        L.mdh_prof_reset()
        L.mdh_prof_enable(1)
        for _ in range(3):
            fn()
        sync()
        L.mdh_prof_enable(0)
        buf = ctypes.create_string_buffer(1 << 16)
        L.mdh_prof_report(buf, len(buf))
        out = {}
        for line in buf.value.decode().strip().splitlines():
            name, count, total = line.split()
            out[name] = float(total) / int(count)
        return out

    pos, box = lattice_positions("fcc", A, args.cells, args.cells, args.cells)
    cell = np.array(box, float)[:3]
    rng = np.random.default_rng(0)
    pos = pos + rng.normal(0, 0.05, pos.shape)
    n = len(pos)
    up = lambda a: HArray(torch.from_numpy(np.ascontiguousarray(a)).cuda())
    species = np.array(["Ni", "Al", "Cr"], dtype=object)
    stand_in = {"Ni": "Ni", "Al": "Co", "Cr": "Cr"}

    cols = {c: up(pos[:, k]) for k, c in enumerate("xyz")}

    def system(names, calc):
        frame = Frame(dict(cols)).with_columns(element=names)
        s = mp.System(data=frame, box=cell)
        s.calc = calc
        return s

    def case(tag, codes):
        names = species[codes]
        s = system(names, nep)
        out = {"case": tag, "atoms": n, "rc": nep.rc, "first_ms": timed(s.get_energies)}
        M = int(s.verlet_list.shape[1])
        counts = s.neighbor_number.numpy()
        dist = s.distance_list.dev()
        listed = torch.arange(M, device=dist.device)[None, :] < s.neighbor_number.dev()[:, None]
        inside_r = int(((dist < 6.0) & listed).sum().item())
        inside_a = int(((dist < 5.0) & listed).sum().item())
        del listed
        out["row_width"], out["mean_neighbours"] = M, float(counts.mean())
        out["build"] = laps(lambda: s.build_neighbor(nep.rc))
        present = tuple(sorted({nep.element_list.index(e) for e in set(names.tolist())}))
        type_map = np.full(len(nep.element_list), -1, np.int32)
        type_map[list(present)] = np.arange(len(present))
        types = up(np.array([nep.element_list.index(e) for e in species], np.int32)[codes])
        model = nep._model(present)
        energy, force, virial, total = (HArray.empty(shape, np.float64) for shape in ((n,), (n, 3), (n, 9), (9,)))
        raw = lambda: kernels.nep.calculate(cols["x"], cols["y"], cols["z"], types, type_map, cell, np.zeros(3), np.ones(3, np.int32), s.verlet_list, s.distance_list,
                                            s.neighbor_number, model, energy=energy, force=force, virial=virial, virial_sum=total, n_real=n)
        out["kernels"] = laps(raw)
        out["kernel_ms"] = kernel_times(raw)
        out["pairs"] = {"radial": inside_r, "angular": inside_a, "table_bytes": n * M * 24, "model_block_bytes": int(model.block.nbytes)}
        if "k_nep_gather" in out["kernel_ms"]:
            out["pairs"]["table_read_bytes_per_s"] = 2 * 24 * float(counts.sum()) / (out["kernel_ms"]["k_nep_gather"] * 1e-3)

        def through_system():
            nep.results = {}
            s.get_energies()
            s.get_force()

        out["system"] = laps(through_system)
        print(json.dumps(out), flush=True)
        del s, energy, force, virial
        e = system(np.array([stand_in[x] for x in names], dtype=object), eam)
        again = {"case": tag + "_eam", "atoms": n, "rc": eam.rc, "first_ms": timed(e.get_energies)}
        again["build"] = laps(lambda: e.build_neighbor(eam.rc))

        def eam_through_system():
            eam.results = {}
            e.get_energies()
            e.get_force()

        again["kernel_ms"] = kernel_times(eam_through_system)
        again["system"] = laps(eam_through_system)
        print(json.dumps(again), flush=True)

    case("single", np.zeros(n, np.int64))
    case("three", rng.integers(0, 3, n))


if __name__ == "__main__":
    main()
