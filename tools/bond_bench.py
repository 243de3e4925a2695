"""Times System.cal_bond_analysis / cal_angular_distribution_function on the bench's own frames (bench.slab_positions),
device-resident, with the neighbour list built beforehand and not timed, one warm-up call each:

  (a) cal_bond_analysis(3.087, 180) on config 2: the 136^3-cell FCC Cu lattice rattled by N(0, 0.05 A), 10.06 M atoms;
  (b) config 4, the 9.84 M-atom Cu64Zr36 glass-like frame (elements from `type`): cal_angular_distribution_function with the six
      Cu/Zr centre patterns at [0, 3.6, 0, 3.6], then cal_bond_analysis(3.6, 180).

Prints one JSON line per case: ms, triplets per second (triplets the kernel looked at: sum over rows of nn (nn - 1) / 2) and the
bytes per atom the kernel reads at least once (its row of ids and distances, its count and position, and one type for the ADF).
Usage: python tools/bond_bench.py [--cells 136] [--repeat 5]"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    p = argparse.ArgumentParser()
    p.add_argument("--cells", type=int, default=136)
    p.add_argument("--repeat", type=int, default=5)
    args = p.parse_args()
    import torch

    import bench
    import mdapy_amd as mp
    from mdapy_amd.devarray import HArray
    from mdapy_amd.frame import Frame

    dev = torch.device("cuda")

    def lap(fn):
        fn()  # warm-up
        torch.cuda.synchronize()
        best = []
        for _ in range(args.repeat):
            t0 = time.perf_counter()
            fn()
            torch.cuda.synchronize()
            best.append(time.perf_counter() - t0)
        return 1e3 * float(np.median(best)), 1e3 * float(np.min(best))

    def stats(s):
        nn = s.neighbor_number.dev().to(torch.int64)
        width = int(s.verlet_list.shape[1])
        return int((nn * (nn - 1) // 2).sum()), float(nn.float().mean()), width

    cells = args.cells
    x, y, z, _ = bench.slab_positions(torch, dev, cells, 0, 0.05)
    n = int(x.shape[0])
    s = mp.System(data=Frame({"x": HArray(x), "y": HArray(y), "z": HArray(z)}), box=mp.Box(np.diag([bench.A_CU * cells] * 3)))
    s.build_neighbor(3.087)
    trip, mean_nn, width = stats(s)
    med, best = lap(lambda: s.cal_bond_analysis(3.087, 180))
    print(json.dumps({"case": "a: cal_bond_analysis(3.087, 180), config 2", "atoms": n, "row_width": width, "mean_nn": mean_nn,
                      "triplets": trip, "ms": med, "ms_best": best, "triplets_per_s": trip / (med * 1e-3),
                      "bytes_per_atom": round(4 + 24 + 12 * mean_nn, 1)}), flush=True)
    del s, x, y, z

    gc = cells - 1 if cells > 8 else cells
    x, y, z, _ = bench.slab_positions(torch, dev, gc, 0, 0.35, a=4.0)
    n = int(x.shape[0])
    gen = torch.Generator(device=dev)
    gen.manual_seed(42)
    ty = (torch.rand(n, device=dev, generator=gen) < 0.36).to(torch.int32) + 1
    element = np.where(ty.cpu().numpy() == 1, "Cu", "Zr")
    s = mp.System(data=Frame({"x": HArray(x), "y": HArray(y), "z": HArray(z), "type": HArray(ty), "element": element}),
                  box=mp.Box(np.diag([4.0 * gc] * 3)))
    s.build_neighbor(3.6)
    trip, mean_nn, width = stats(s)
    pats = {f"{a}-{b}-{c}": [0, 3.6, 0, 3.6] for a in ("Cu", "Zr") for b, c in (("Cu", "Cu"), ("Cu", "Zr"), ("Zr", "Zr"))}
    med_adf, best_adf = lap(lambda: s.cal_angular_distribution_function(pats, 180))
    med_ba, best_ba = lap(lambda: s.cal_bond_analysis(3.6, 180))
    print(json.dumps({"case": "b: ADF six Cu/Zr centre patterns [0, 3.6, 0, 3.6] + cal_bond_analysis(3.6, 180), config 4",
                      "atoms": n, "row_width": width, "mean_nn": mean_nn, "triplets": trip, "ms_adf": med_adf, "ms_bond": med_ba,
                      "ms": med_adf + med_ba, "ms_best": best_adf + best_ba, "triplets_per_s": 2 * trip / ((med_adf + med_ba) * 1e-3),
                      "bytes_per_atom": round(2 * (4 + 24 + 12 * mean_nn) + 4, 1)}), flush=True)


if __name__ == "__main__":
    main()
