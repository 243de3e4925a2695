"""Times ``System.create_bonds`` and ``System.cal_chemical_species`` (csrc/bonds.hip, mdapy_amd/_build_bond.py) on the water frame
of tests/golden/bond replicated --copies times (4 x 6 x 7: 4 128 768 atoms), list already built.  One JSON line per figure:

  resources  registers, scratch, LDS and occupancy of every kernel of csrc/bonds.hip as hipcc reports them
             (-Rpass-analysis=kernel-resource-usage); needs no device
  case       atoms, the list's reach and width, bonds, clusters
  ranges     the library's own HIP-event ranges, ms per call: k_bond_count, bond_scan, k_bond_write — for one cutoff and for
             the per-pair matrix — and the bytes per second of the two bond passes (12 B per slot of the (N, M) rows, nn and
             the row's type per atom; the write pass also 4 B of offset per row and 8 B per bond) beside the 4.93 TB/s a copy
             reaches; the gathered types of the neighbours are not counted
  calls      host clock around whole calls, each ending in a device synchronise: create_bonds with one cutoff and with the
             matrix, cal_chemical_species with a search list (and mol_id) and without, cal_cluster_analysis with the same
             per-pair cutoffs (the share of cal_chemical_species that is the existing clustering) and with one cutoff
  host       numpy's run of tests/_bond_pairs_ref.py's bond rule on the first list (the copy to the host not counted), and
             whether it gives the same pairs

The same for a second, wider list (--wide-rc 4.0: what a system that was analysed before remembers).  Medians of --calls calls
after a warm-up call, best and worst beside them.

Usage: python tools/bond_pairs_bench.py [--copies 4 6 7] [--scale 0.6] [--wide-rc 4.0] [--calls 5] [--isa-only] [--no-host]"""
import argparse
import ctypes
import gzip
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
HBM_COPY = 4.93e12  # bytes per second a copy (read + write) reaches on this device (tools/ceilings.py)


def resources():
    src = os.path.join(ROOT, "mdapy_amd", "csrc", "bonds.hip")
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    with tempfile.TemporaryDirectory() as tmp:
        done = subprocess.run([hipcc, "-O3", "-std=c++17", "--offload-arch=gfx950", "-ffp-contract=off", "--cuda-device-only", "-c",
                               "-Rpass-analysis=kernel-resource-usage", src, "-o", os.path.join(tmp, "bonds.o")],
                              stderr=subprocess.PIPE, text=True, check=True)
    table, name = {}, None
    keys = {"TotalSGPRs": "sgprs", "VGPRs": "vgprs", "AGPRs": "agprs", "ScratchSize [bytes/lane]": "scratch_bytes_per_lane",
            "Occupancy [waves/SIMD]": "waves_per_simd", "LDS Size [bytes/block]": "lds_bytes"}
    for line in done.stderr.splitlines():
        m = re.search(r"remark:\s+(.*?):\s+(\S+) \[-Rpass", line)
        if not m:
            continue
        if m.group(1) == "Function Name":
            mangled = m.group(2)
            name = re.sub(r"^_ZN3mdh\d+(k_\w+?)(I|E).*$", r"\1", mangled)
            t = re.search(r"ILi(\d+)ELi(\d+)ELb([01])E", mangled) or re.search(r"()()ILb([01])E", mangled)
            if t:  # k_bond_rows<lanes per row, rows per group, pass>, k_bond_rows_wide<pass>
                name += "<" + ", ".join(filter(None, [t.group(1), t.group(2), "write" if t.group(3) == "1" else "count"])) + ">"
            table[name] = {}
        elif name and m.group(1) in keys:
            table[name][keys[m.group(1)]] = int(m.group(2))
    return table


def main():
    p = argparse.ArgumentParser()
    p.add_argument("--copies", type=int, nargs=3, default=[4, 6, 7])
    p.add_argument("--scale", type=float, default=0.6)
    p.add_argument("--wide-rc", type=float, default=4.0)
    p.add_argument("--calls", type=int, default=5)
    p.add_argument("--isa-only", action="store_true")
    p.add_argument("--no-host", action="store_true")
    args = p.parse_args()
    print(json.dumps({"resources": resources()}), flush=True)
    if args.isa_only:
        return
    import torch

    import mdapy_amd as mp
    from mdapy_amd import _lib
    from mdapy_amd.devarray import as_numpy
    from mdapy_amd.system import _normalize_bond_cutoff

    if not torch.cuda.is_available():
        raise RuntimeError("bond_pairs_bench needs a HIP device")
    L = _lib.lib()

    def timed(fn):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        out = fn()
        torch.cuda.synchronize()
        return time.perf_counter() - t0, out

    def laps(fn):
        fn()  # warm-up
        s = [timed(fn)[0] for _ in range(max(args.calls, 1))]
        return {"ms": 1e3 * float(np.median(s)), "ms_best": 1e3 * float(np.min(s)), "ms_worst": 1e3 * float(np.max(s))}

    def ranges(fn):
        buf = ctypes.create_string_buffer(1 << 16)
        fn()
        torch.cuda.synchronize()
        L.mdh_prof_reset()
        L.mdh_prof_enable(1)
        for _ in range(max(args.calls, 1)):
            fn()
        torch.cuda.synchronize()
        L.mdh_prof_enable(0)
        L.mdh_prof_report(buf, len(buf))
        out = {}
        for line in buf.value.decode().strip().splitlines():
            name, count, ms = line.split()
            out[name] = float(ms) / int(count)
        return out

    with tempfile.TemporaryDirectory() as tmp:
        path = os.path.join(tmp, "water.xyz")
        with gzip.open(os.path.join(ROOT, "tests", "golden", "bond", "water.xyz.gz"), "rb") as src, open(path, "wb") as dst:
            dst.write(src.read())
        system = mp.System(path)
    system.replicate(*args.copies)
    n = system.N
    present = sorted(set(np.unique(system.data["element"].to_numpy()).tolist()))
    radii = [mp.vdw_radii.vdw_radius(e) for e in present]
    matrix = np.array([[(a + b) * args.scale for b in radii] for a in radii])
    by_name = {(present[a], present[b]): matrix[a, b] for a in range(len(present)) for b in range(a, len(present))}
    by_type = {f"{a + 1}-{b + 1}": matrix[a, b] for a in range(len(present)) for b in range(a, len(present))}
    reach = float(matrix.max())
    for label, rc in (("own_list", reach), ("wide_list", args.wide_rc)):
        system.build_neighbor(rc)
        m = int(system.verlet_list.shape[1])
        found = system.cal_chemical_species(scale=args.scale, check_most=4)  # (also sets the type column the matrix goes by)
        nbond = int(system.create_bonds(matrix).shape[0])
        print(json.dumps({"case": label, "atoms": n, "list_rc": rc, "list_width": m, "bonds_matrix": nbond,
                          "bonds_one_cutoff": int(system.create_bonds(reach).shape[0]), "clusters": int(system.cluster_number),
                          "most_frequent": found}), flush=True)
        for what, cut in (("one_cutoff", reach), ("matrix", matrix)):
            k = ranges(lambda: system.create_bonds(cut))
            k = {name: k[name] for name in ("k_bond_count", "bond_scan", "k_bond_write") if name in k}
            pairs = int(system.bond.shape[0])
            count_bytes = n * m * 12 + n * 8
            write_bytes = count_bytes + n * 4 + pairs * 8
            rate = {"count": count_bytes / (k["k_bond_count"] * 1e-3), "write": write_bytes / (k["k_bond_write"] * 1e-3)}
            print(json.dumps({"case": label, "cutoff": what, "ranges_ms": k, "count_pass_bytes": count_bytes, "write_pass_bytes": write_bytes,
                              "bytes_per_s": rate, "of_copy_ceiling": {name: r / HBM_COPY for name, r in rate.items()}}), flush=True)
        calls = {"create_bonds_one_cutoff": laps(lambda: system.create_bonds(reach)),
                 "create_bonds_matrix": laps(lambda: system.create_bonds(matrix)),
                 "create_bonds_element_dict": laps(lambda: system.create_bonds(by_name)),
                 "species_search_mol_id": laps(lambda: system.cal_chemical_species(["H2O", "H4O2"], scale=args.scale, add_mol_id=True)),
                 "species_most_frequent": laps(lambda: system.cal_chemical_species(scale=args.scale)),
                 "cluster_per_pair": laps(lambda: system.cal_cluster_analysis(by_type)),
                 "cluster_one_cutoff": laps(lambda: system.cal_cluster_analysis(reach))}
        share = {name: calls["cluster_per_pair"]["ms"] / calls[name]["ms"] for name in ("species_search_mol_id", "species_most_frequent")}
        print(json.dumps({"case": label, "calls": calls, "clustering_share_of_species": share}), flush=True)
        if not args.no_host and label == "own_list":  # (the wide list: a dozen (N, M) int64 temporaries on the host)
            sys.path.insert(0, os.path.join(ROOT, "tests"))
            import _bond_pairs_ref

            lists = [np.asarray(as_numpy(a)) for a in (system.verlet_list, system.distance_list, system.neighbor_number)]
            _, compact, _ = _normalize_bond_cutoff(matrix, system.data)
            t0 = time.perf_counter()
            want = _bond_pairs_ref.build_bond(*lists, compact, matrix)
            t1 = time.perf_counter()
            print(json.dumps({"case": label, "host_numpy_ms": {"bond_rule_matrix": 1e3 * (t1 - t0)},
                              "same_bonds": bool(np.array_equal(want, as_numpy(system.create_bonds(matrix))))}), flush=True)
            del lists, want
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
