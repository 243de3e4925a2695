"""Times the void analysis (mdapy_amd/void_analysis.py, csrc/voids.hip) on the headline box — fcc Cu, 136^3 cells of a = 3.615,
10 061 824 sites, positions resident in HBM — with three spherical voids (radii 40, 60 and 80), and on the same box with ONE
spherical void of half the box's volume: every point of that void adds to one word of the cluster sizes.  One JSON line per
figure:

  resources  registers, scratch, LDS and occupancy of every kernel of csrc/voids.hip as hipcc reports them
             (-Rpass-analysis=kernel-resource-usage); needs no device
  case       atoms, grid, empty cells, points kept, voids
  ranges     the library's own HIP-event ranges, ms per call: k_void_fill (the occupancy kernel alone: 24 B read per atom; its
             bytes per second beside the 8.0 TB/s of the HBM's specification and the 6.29 TB/s a float4 copy reaches),
             void_rank (flags + prefix sum), k_void_points (the first ordered compaction), void_prune (sizes, two prefix sums,
             the second ordered compaction)
  calls      host clock around whole shim calls, each ending in a device synchronise: fill, points (both of its library
             calls), cluster (System of the void points + cal_cluster_analysis(1.1 rc): the existing neighbour build and
             clustering), prune, and compute() as a whole with the share of it that `cluster` is
  host       numpy's run of tests/_void_ref.py's grid, points and pruning on the host (the clustering left out: its brute
             force is for test sizes), for orientation only

Medians of --calls calls after a warm-up call, best and worst beside them.

Usage: python tools/void_bench.py [--cells 136] [--rc 4.0] [--calls 5] [--isa-only] [--no-host]"""
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
HBM_SPEC, HBM_COPY = 8.0e12, 6.29e12  # bytes per second: the specification, and what a float4 copy reaches


def resources():
    src = os.path.join(ROOT, "mdapy_amd", "csrc", "voids.hip")
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    with tempfile.TemporaryDirectory() as tmp:
        done = subprocess.run([hipcc, "-O3", "-std=c++17", "--offload-arch=gfx950", "-ffp-contract=off", "--cuda-device-only", "-c",
                               "-Rpass-analysis=kernel-resource-usage", src, "-o", os.path.join(tmp, "voids.o")],
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
    p.add_argument("--cells", type=int, default=136)
    p.add_argument("--rc", type=float, default=4.0)
    p.add_argument("--calls", type=int, default=5)
    p.add_argument("--isa-only", action="store_true")
    p.add_argument("--no-host", action="store_true")
    args = p.parse_args()
    print(json.dumps({"resources": resources()}), flush=True)
    if args.isa_only:
        return
    import torch

    import mdapy_amd as mp
    from mdapy_amd import _lib, kernels
    from mdapy_amd.devarray import HArray

    if not torch.cuda.is_available():
        raise RuntimeError("void_bench needs a HIP device")
    L = _lib.lib()
    edge, rc = A * args.cells, args.rc
    cell = mp.Box(np.eye(3) * edge, [1, 1, 1])

    def lattice():
        """the fcc sites as three columns in HBM, in the lattice builder's order (cell by cell, four sites each)"""
        k = torch.arange(args.cells, device="cuda", dtype=torch.float64) * A
        basis = torch.tensor([[0, 0, 0], [0.5, 0.5, 0], [0.5, 0, 0.5], [0, 0.5, 0.5]], device="cuda", dtype=torch.float64) * A
        gx, gy, gz = torch.meshgrid(k, k, k, indexing="ij")
        corner = torch.stack([gx, gy, gz], dim=-1).reshape(-1, 1, 3)
        return (corner + basis[None]).reshape(-1, 3)

    def without(pos, spheres):
        keep = torch.ones(len(pos), dtype=torch.bool, device="cuda")
        for centre, radius in spheres:
            keep &= torch.linalg.norm(pos - torch.tensor(centre, device="cuda", dtype=torch.float64), dim=1) > radius
        return tuple(HArray(pos[keep][:, k].contiguous()) for k in range(3))

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

    pos = lattice()
    half = edge * (3.0 / (8.0 * np.pi)) ** (1.0 / 3.0)  # the sphere of half the box's volume: 0.4924 edge, it just fits
    jobs = {"three_voids": [((0.25 * edge,) * 3, 40.0), ((0.7 * edge, 0.3 * edge, 0.6 * edge), 60.0), ((0.4 * edge, 0.75 * edge, 0.3 * edge), 80.0)],
            "one_void_of_half_the_box": [((0.5 * edge,) * 3, half)]}
    for name, spheres in jobs.items():
        x, y, z = without(pos, spheres)
        n = len(x)
        system = mp.System(data={"x": x, "y": y, "z": z}, box=cell)
        where = (x, y, z, cell.box, cell.origin, cell.boundary, rc)
        grid = kernels.neighbor._fill_cell_for_void(*where)
        px, py, pz = kernels.void.void_points(grid, cell.box, cell.origin)

        def clustered():
            points = mp.System(data={"x": px, "y": py, "z": pz}, box=cell)
            points.cal_cluster_analysis(rc=rc * 1.1)
            return points

        points = clustered()
        ids, number = points.data["cluster_id"].device_array(), points.cluster_number
        job = mp.VoidAnalysis(system, rc)
        job.compute()
        print(json.dumps({"case": name, "atoms": n, "grid": list(grid.shape), "cells": int(grid.size), "empty_cells": len(px),
                          "clusters": int(number), "points_kept": 0 if job.void_system is None else job.void_system.N,
                          "voids": job.void_number, "void_volume": job.void_volume}), flush=True)
        k = ranges(lambda: (kernels.neighbor._fill_cell_for_void(*where), kernels.void.void_points(grid, cell.box, cell.origin),
                            kernels.void.prune(px, py, pz, ids, number)))
        fill_s = k.get("k_void_fill", float("nan")) * 1e-3
        print(json.dumps({"case": name, "ranges_ms": k, "k_void_fill_bytes": 24 * n, "k_void_fill_bytes_per_s": 24 * n / fill_s,
                          "of_hbm_spec": 24 * n / fill_s / HBM_SPEC, "of_float4_copy": 24 * n / fill_s / HBM_COPY}), flush=True)
        calls = {"fill": laps(lambda: kernels.neighbor._fill_cell_for_void(*where)),
                 "points": laps(lambda: kernels.void.void_points(grid, cell.box, cell.origin)),
                 "cluster": laps(clustered),
                 "prune": laps(lambda: kernels.void.prune(px, py, pz, ids, number)),
                 "compute": laps(lambda: mp.VoidAnalysis(system, rc).compute())}
        print(json.dumps({"case": name, "calls": calls, "cluster_share_of_compute": calls["cluster"]["ms"] / calls["compute"]["ms"]}), flush=True)
        if not args.no_host:
            sys.path.insert(0, os.path.join(ROOT, "tests"))
            import _void_ref

            hx, hy, hz = (a.numpy() for a in (x, y, z))
            host_ids = np.asarray(ids.numpy())
            t0 = time.perf_counter()
            g = _void_ref._fill_cell_for_void(hx, hy, hz, cell.box, cell.origin, cell.boundary, rc)
            t1 = time.perf_counter()
            c = _void_ref.void_points(g, cell.box, cell.origin)
            t2 = time.perf_counter()
            kept = _void_ref.prune(*c, host_ids, number)
            t3 = time.perf_counter()
            print(json.dumps({"case": name, "host_numpy_ms": {"fill": 1e3 * (t1 - t0), "points": 1e3 * (t2 - t1), "prune": 1e3 * (t3 - t2),
                                                              "all_but_the_clustering": 1e3 * (t3 - t0)},
                              "same_grid": bool(np.array_equal(g, grid.numpy())), "same_points": bool(np.array_equal(c[0], px.numpy())),
                              "same_kept": bool(np.array_equal(kept[3], job.void_system.data["cluster_id"].to_numpy()))}), flush=True)
        del x, y, z, system, grid, px, py, pz, points, ids, job
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
