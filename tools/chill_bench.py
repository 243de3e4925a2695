"""Times System.cal_chill_plus on cubic ice: diamond O sites, 80^3 cells (4 096 000 atoms), a = 6.37, N(0, 0.15 A) noise, rc 3.5,
columns resident in HBM, the list built once before timing.  One JSON line per case:

  chill    cal_chill_plus(rc) on the remembered list: median, best and worst of --calls calls after a warm-up call, each ending
           in a device synchronise (the position pack, both passes and the store of the column are timed)
  temp     cal_atomic_temperature(rc) of the same System on the same list: the closest existing kernel (two sweeps of one
           32-byte gather per neighbour against one sweep of 32-byte and one of 64-byte gathers)
  kernels  per-pass times from the library's own event pairs (mdh_prof_enable), median over the same number of calls in a loop
           of its own (an event pair costs stream time: the call times above are taken with it off)
  bytes    what each pass asks the memory system for — rows at 12 B per slot (id + distance) in both passes, one 32-byte position
           per bond and one for the atom in pass 1, one 64-byte record per bond and one for the atom in pass 2, 64 B written per
           atom by pass 1 and 4 B by pass 2 — and what it cannot avoid (every row, position and record once); over the kernel
           time, as a fraction of the 6.3 TB/s an MI355X reaches on streaming reads

  shuffled the same atoms handed in in one random order (the call runs on the cell-sorted twin and scatters the column back)

--list-rc R builds the remembered list at a larger cutoff R (a list borrowed from another analysis: wide rows, most entries no bonds).

Usage: python tools/chill_bench.py [--cells 80] [--calls 10] [--rc 3.5] [--list-rc R] [--no-shuffled]"""
import argparse
import ctypes
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

HBM_ACHIEVABLE = 6.3e12  # B/s


def main():
    p = argparse.ArgumentParser()
    p.add_argument("--cells", type=int, default=80)
    p.add_argument("--calls", type=int, default=10)
    p.add_argument("--rc", type=float, default=3.5)
    p.add_argument("--sigma", type=float, default=0.15)
    p.add_argument("--list-rc", type=float, default=None)
    p.add_argument("--no-shuffled", action="store_true")
    args = p.parse_args()
    import torch

    import mdapy_amd as mp
    from mdapy_amd import _lib
    from mdapy_amd.build_lattice import lattice_positions
    from mdapy_amd.devarray import HArray
    from mdapy_amd.frame import Frame

    if not torch.cuda.is_available():
        raise RuntimeError("chill_bench needs a HIP device")
    L = _lib.lib()

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

    def kernel_ms(fn, names):
        """median per-call time of each named range over --calls calls"""
        seen = {name: [] for name in names}
        buf = ctypes.create_string_buffer(1 << 16)
        for _ in range(max(args.calls, 1)):
            sync()
            L.mdh_prof_reset()
            L.mdh_prof_enable(1)
            fn()
            sync()
            L.mdh_prof_enable(0)
            L.mdh_prof_report(buf, len(buf))
            for line in buf.value.decode().splitlines():
                name, count, ms = line.split()
                if name in seen:
                    seen[name].append(float(ms))
        L.mdh_prof_reset()
        return {name: float(np.median(v)) for name, v in seen.items() if v}

    def in_hbm(xyz, **more):
        cols = {c: HArray(torch.from_numpy(np.ascontiguousarray(xyz[:, k])).cuda()) for k, c in enumerate("xyz")}
        cols.update({k: HArray(torch.from_numpy(np.ascontiguousarray(v)).cuda()) for k, v in more.items()})
        return Frame(cols)

    pos, box = lattice_positions("diamond", 6.37, args.cells, args.cells, args.cells)
    cell = np.array(box, float)[:3]
    rng = np.random.default_rng(0)
    pos = pos + rng.normal(0, args.sigma, pos.shape)
    vel = rng.normal(0, 1.0, pos.shape)
    n = len(pos)

    def case(tag, order):
        s = mp.System(data=in_hbm(pos[order], vx=vel[order, 0], vy=vel[order, 1], vz=vel[order, 2], amass=np.full(n, 15.999)), box=cell)
        list_rc = args.list_rc or args.rc
        out = {"case": tag, "atoms": n, "rc": args.rc, "list_rc": list_rc, "sigma": args.sigma, "build_ms": timed(lambda: s.build_neighbor(list_rc))}
        out["row_width"] = width = int(s.verlet_list.shape[1])
        out["on_twin"] = s._listed_on_twin() is not None
        out["chill"] = laps(lambda: s.cal_chill_plus(args.rc))
        out["temp"] = laps(lambda: s.cal_atomic_temperature(args.rc))
        out["kernels_ms"] = kernel_ms(lambda: s.cal_chill_plus(args.rc), ("k_chill_q", "k_chill_classify"))
        out["kernels_ms"].update(kernel_ms(lambda: s.cal_atomic_temperature(args.rc), ("k_atomic_temp",)))
        labels = s.data["chill_plus"].to_numpy()
        out["classes"] = np.bincount(labels, minlength=6).tolist()
        bonds = float((s.distance_list.dev() <= args.rc).sum().item()) / n  # (pads carry a distance beyond the list's cutoff)
        out["bonds_per_atom"] = bonds
        asked = {"k_chill_q": n * (12 * width + 32 * (1 + bonds) + 64), "k_chill_classify": n * (12 * width + 64 * (1 + bonds) + 4)}
        least = {"k_chill_q": n * (12 * width + 32 + 64), "k_chill_classify": n * (12 * width + 64 + 4)}
        # (the yardstick's range holds its pack kernel, 32 B read and 32 B written per atom, and two sweeps over the rows)
        asked["k_atomic_temp"] = n * (64 + 2 * (12 * width + 32 * (1 + bonds)) + 8)
        least["k_atomic_temp"] = n * (64 + 2 * 12 * width + 32 + 8)
        out["bytes"] = {}
        for name in asked:
            ms = out["kernels_ms"].get(name)
            out["bytes"][name] = {"asked": asked[name], "least": least[name]}
            if ms:
                out["bytes"][name].update(asked_TBps=asked[name] / ms / 1e9, least_TBps=least[name] / ms / 1e9,
                                          least_over_hbm=least[name] / (ms * 1e-3) / HBM_ACHIEVABLE)
        print(json.dumps(out), flush=True)

    case("ordered", np.arange(n))
    if not args.no_shuffled:
        case("shuffled", np.random.default_rng(1).permutation(n))


if __name__ == "__main__":
    main()
