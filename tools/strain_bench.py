"""Times AtomicStrain.compute on frames like tools/consumer_times.py's: fcc Cu, 100^3 cells (4 000 000 atoms), N(0, 0.05 A) rattle,
rc 5.0, with a sheared, stretched and rattled copy as the current frame.  One JSON line per figure:

  first    AtomicStrain(rc, ref) + the first compute: the list build, the reference pack, the first launch of every kernel
  steady   one compute on a new current System, median and best of --calls calls after a warm-up call, each ending in a
           device synchronise (the current columns are in HBM already; the frame's pack, the gather and the store are timed)
  temp     System.cal_atomic_temperature(rc) of the reference System, in the same process and on the same list: the closest
           existing kernel (two sweeps of 32-byte gathers against strain's one sweep of two)
  shuffled the same atoms handed in in one random order for both frames (the reference runs on its cell-sorted twin)

Usage: python tools/strain_bench.py [--cells 100] [--calls 10] [--rc 5.0] [--no-shuffled]"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

GRAD = np.array([[1.03, 0.0, 0.0], [0.04, 0.98, 0.0], [-0.02, 0.03, 1.01]])


def main():
    p = argparse.ArgumentParser()
    p.add_argument("--cells", type=int, default=100)
    p.add_argument("--calls", type=int, default=10)
    p.add_argument("--rc", type=float, default=5.0)
    p.add_argument("--no-shuffled", action="store_true")
    args = p.parse_args()
    import torch

    import mdapy_amd as mp
    from mdapy_amd.build_lattice import lattice_positions
    from mdapy_amd.devarray import HArray
    from mdapy_amd.frame import Frame

    if not torch.cuda.is_available():
        raise RuntimeError("strain_bench needs a HIP device")

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

    def in_hbm(xyz, **more):
        cols = {c: HArray(torch.from_numpy(np.ascontiguousarray(xyz[:, k])).cuda()) for k, c in enumerate("xyz")}
        cols.update({k: HArray(torch.from_numpy(np.ascontiguousarray(v)).cuda()) for k, v in more.items()})
        return Frame(cols)

    pos, box = lattice_positions("fcc", 3.615, args.cells, args.cells, args.cells)
    cell = np.array(box, float)[:3]
    rng = np.random.default_rng(0)
    pos = pos + rng.normal(0, 0.05, pos.shape)
    vel = rng.normal(0, 1.0, pos.shape)
    moved, moved_cell = pos @ GRAD + rng.normal(0, 0.03, pos.shape), cell @ GRAD
    n = len(pos)

    def case(tag, order):
        ref = mp.System(data=in_hbm(pos[order], vx=vel[order, 0], vy=vel[order, 1], vz=vel[order, 2], amass=np.full(n, 63.546)), box=cell)
        cur_frame = in_hbm(moved[order])
        state = {}

        def first():
            state["strain"] = mp.AtomicStrain(args.rc, ref)
            state["strain"].compute(mp.System(data=cur_frame, box=mp.Box(moved_cell)))

        out = {"case": tag, "atoms": n, "rc": args.rc, "first_ms": timed(first)}
        strain = state["strain"]
        out["row_width"] = int(ref.verlet_list.shape[1])
        out["on_twin"] = ref._listed_on_twin() is not None
        out["steady"] = laps(lambda: strain.compute(mp.System(data=cur_frame, box=mp.Box(moved_cell))))
        mapped = mp.AtomicStrain(args.rc, ref, affine=True)  # (builds the list again: not timed)
        out["steady_affine"] = laps(lambda: mapped.compute(mp.System(data=cur_frame, box=mp.Box(moved_cell))))
        out["temp"] = laps(lambda: ref.cal_atomic_temperature(args.rc))
        print(json.dumps(out), flush=True)

    case("ordered", np.arange(n))
    if not args.no_shuffled:
        case("shuffled", np.random.default_rng(1).permutation(n))


if __name__ == "__main__":
    main()
