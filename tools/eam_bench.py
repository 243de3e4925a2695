"""Times the EAM calculator on frames like tools/consumer_times.py's: fcc, 100^3 cells (4 000 000 atoms), N(0, 0.05 A) rattle, under
tests/golden/eam/NiCoCr.lammps.eam.gz (rc 5.88 A).  One JSON line per figure:

  resources  VGPRs / LDS / scratch of the kernels of csrc/eam.hip (hipcc -Rpass-analysis=kernel-resource-usage); --isa-only stops here
  first      System.get_energies() on a new System: the list build, the tables' upload, the first launches, the results' download
  build      System.build_neighbor(rc) alone, median of --calls: the share of a calculation that is the list
  kernels    the raw shim on the list in HBM, results left in HBM, accumulate off — the whole call (median, best, worst of --calls
             after a warm-up call, each ending in a device synchronise) and its kernels' own times from the library's event pairs
             (mdh_prof_*: a run of its own, the events add a few microseconds per launch), with the bytes every pass must move
             (rows once per pass, per-atom inputs and outputs once) against the copy ceiling
  system     System.get_energies() + get_force() on a System that remembers its list (calc.results cleared in between): the kernels
             plus 104 bytes per atom of results to the host
  temp       System.cal_atomic_temperature(rc) on the same list, in the same process: the closest existing kernel
  host       the numpy restatement (tests/_eam_ref.py) at --host-cells^3 cells, once

for a single-element assignment (every atom Ni: one table of the three is read) and a 3-element one (random Ni / Co / Cr).

Usage: python tools/eam_bench.py [--cells 100] [--calls 10] [--host-cells 8] [--isa-only] [--no-host]"""
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
HBM_COPY = 6.29e12  # bytes per second: what a float4 copy reaches on an MI355X


def resources():
    src = os.path.join(ROOT, "mdapy_amd", "csrc", "eam.hip")
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    with tempfile.TemporaryDirectory() as tmp:
        done = subprocess.run([hipcc, "-O3", "-std=c++17", "--offload-arch=gfx950", "-ffp-contract=off", "--cuda-device-only", "-c",
                               "-Rpass-analysis=kernel-resource-usage", src, "-o", os.path.join(tmp, "eam.o")],
                              stderr=subprocess.PIPE, text=True, check=True)
    table, name = {}, None
    keys = {"TotalSGPRs": "sgprs", "VGPRs": "vgprs", "AGPRs": "agprs", "ScratchSize [bytes/lane]": "scratch_bytes_per_lane",
            "Occupancy [waves/SIMD]": "waves_per_simd", "LDS Size [bytes/block]": "lds_bytes"}
    for line in done.stderr.splitlines():
        m = re.search(r"remark:\s+(.*?):\s+(\S+) \[-Rpass", line)
        if not m:
            continue
        if m.group(1) == "Function Name":
            name = re.sub(r"^_ZN3mdh\d+(k_\w+?)(I|E).*$", r"\1", m.group(2)) + ("<tri>" if "ILb1E" in m.group(2) else "")
            table[name] = {}
        elif name and m.group(1) in keys:
            table[name][keys[m.group(1)]] = int(m.group(2))
    return table


def main():
    p = argparse.ArgumentParser()
    p.add_argument("--cells", type=int, default=100)
    p.add_argument("--calls", type=int, default=10)
    p.add_argument("--host-cells", type=int, default=8)
    p.add_argument("--isa-only", action="store_true")
    p.add_argument("--no-host", action="store_true")
    args = p.parse_args()
    print(json.dumps({"resources": resources()}), flush=True)
    if args.isa_only:
        return
    import torch

    import mdapy_amd as mp
    from mdapy_amd import _eam, _lib
    from mdapy_amd.build_lattice import lattice_positions
    from mdapy_amd.devarray import HArray
    from mdapy_amd.frame import Frame

    if not torch.cuda.is_available():
        raise RuntimeError("eam_bench needs a HIP device")
    L = _lib.lib()
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
    vel = rng.normal(0, 1.0, pos.shape)
    n = len(pos)
    up = lambda a: HArray(torch.from_numpy(np.ascontiguousarray(a)).cuda())

    species = np.array(["Ni", "Co", "Cr"], dtype=object)
    file_index = np.array([eam.elements_list.index(e) for e in species], np.int32)

    def case(tag, codes):
        names = species[codes]
        cols = {c: up(pos[:, k]) for k, c in enumerate("xyz")}
        cols.update(vx=up(vel[:, 0]), vy=up(vel[:, 1]), vz=up(vel[:, 2]), amass=up(np.full(n, 58.6934)))
        frame = Frame(cols).with_columns(element=names)
        s = mp.System(data=frame, box=cell)
        s.calc = eam
        out = {"case": tag, "atoms": n, "rc": eam.rc, "first_ms": timed(s.get_energies)}
        M = int(s.verlet_list.shape[1])
        out["row_width"], out["mean_neighbours"] = M, float(s.neighbor_number.numpy().mean())
        out["build"] = laps(lambda: s.build_neighbor(eam.rc))
        types = up(file_index[codes])
        shim = _eam.EAM(eam.rc, eam.dr, eam.drho, eam.F_rho, eam.rho_r, eam._rphi_r)
        energy, force, virial, total = (HArray.empty(shape, np.float64) for shape in ((n,), (n, 3), (n, 9), (9,)))
        raw = lambda: shim.calculate(cols["x"], cols["y"], cols["z"], types, cell, np.zeros(3), np.ones(3, np.int32), s.verlet_list,
                                     s.distance_list, s.neighbor_number, force, virial, energy, accumulate=False, n_real=n, virial_sum=total)
        out["kernels"] = laps(raw)
        out["kernel_ms"] = kernel_times(raw)
        rows = n * M * 12  # ids and distances, once per pass
        moved = {"k_eam_density": rows + n * (4 + 4 + 16), "k_eam_pair": rows + n * (4 + 32 + 16 + 104), "k_column_sums9": n * 72}
        out["bytes"] = moved
        out["share_of_copy_ceiling"] = {k: moved[k] / HBM_COPY / (out["kernel_ms"][k] * 1e-3) for k in moved if k in out["kernel_ms"]}

        def through_system():
            eam.results = {}
            s.get_energies()
            s.get_force()

        out["system"] = laps(through_system)
        out["temp"] = laps(lambda: s.cal_atomic_temperature(eam.rc))
        out["build_share_of_a_first_calculation"] = out["build"]["ms"] / (out["build"]["ms"] + out["system"]["ms"])
        print(json.dumps(out), flush=True)

    case("single", np.zeros(n, np.int64))
    case("three", rng.integers(0, 3, n))

    if not args.no_host:
        sys.path.insert(0, os.path.join(ROOT, "tests"))
        import _eam_ref

        c = args.host_cells
        hpos, hbox = lattice_positions("fcc", A, c, c, c)
        hpos = hpos + rng.normal(0, 0.05, hpos.shape)
        hnames = np.array(["Ni", "Co", "Cr"], dtype=object)[rng.integers(0, 3, len(hpos))]
        hs = mp.System(pos=hpos, box=hbox)
        hs.set_element(hnames)
        hs.calc = eam
        gpu_ms = timed(hs.get_energies)
        t0 = time.perf_counter()
        want = _eam_ref.on_system_list(hs, eam)
        host_ms = 1e3 * (time.perf_counter() - t0)
        print(json.dumps({"case": "host", "atoms": len(hpos), "numpy_restatement_ms": host_ms, "system_first_call_ms": gpu_ms,
                          "bitwise_equal": bool(np.array_equal(want[0], hs.get_energies()) and np.array_equal(want[1], hs.get_force()))}),
              flush=True)


if __name__ == "__main__":
    main()
