"""Times the Wigner-Seitz analysis on frames like tools/strain_bench.py's: fcc Cu, 100^3 cells (4 000 000 sites), the sites
rattled by N(0, 0.05 A); the current frame is the lattice rattled by about 0.1 A with 0.1 % of its atoms removed and as many
inserted at random positions.  One JSON line per case ("ordered": both frames in lattice order; "shuffled": each in a random
order of its own), every figure on its own:

  build      Tree.build_with_coords: wrap, bin, pack the site records (what WignerSeitzAnalysis(ref) costs)
  query      Tree.query_nearest_batch over the current frame, plain and through an affine map
  occupancy  cal_site_occupancy: histogram, gather, the two counts read back
  compute    WignerSeitzAnalysis.compute as a user calls it (query + occupancy + the result arrays copied to the host)
  strain     AtomicStrain(rc).compute on the same frame (needs as many atoms as sites: run on the frame before removal / insertion)
  knn1       _fast_knn.knn(k = 1) over the current frame's own atoms
  bytes      bytes per atom each pass must move, from the shapes (not measured)

Medians of --calls calls after a warm-up call, best and worst beside them; every timed call ends in a device synchronise.

Usage: python tools/ws_bench.py [--cells 100] [--calls 10] [--rc 5.0] [--no-shuffled] [--no-yardsticks]"""
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
    p.add_argument("--cells", type=int, default=100)
    p.add_argument("--calls", type=int, default=10)
    p.add_argument("--rc", type=float, default=5.0)
    p.add_argument("--no-shuffled", action="store_true")
    p.add_argument("--no-yardsticks", action="store_true")
    args = p.parse_args()
    import torch

    import mdapy_amd as mp
    from mdapy_amd import _fast_knn
    from mdapy_amd.build_lattice import lattice_positions
    from mdapy_amd.devarray import HArray
    from mdapy_amd.frame import Frame

    if not torch.cuda.is_available():
        raise RuntimeError("ws_bench needs a HIP device")

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

    def up(a):
        return HArray(torch.from_numpy(np.ascontiguousarray(a)).cuda())

    def in_hbm(xyz):
        return Frame({c: up(xyz[:, k]) for k, c in enumerate("xyz")})

    pos, box = lattice_positions("fcc", 3.615, args.cells, args.cells, args.cells)
    cell = np.array(box, float)[:3]
    rng = np.random.default_rng(0)
    sites = pos + rng.normal(0, 0.05, pos.shape)
    n = len(pos)
    rattled = pos + rng.normal(0, 0.1 / np.sqrt(3.0), pos.shape)
    gone = max(n // 1000, 1)
    keep = np.sort(rng.permutation(n)[gone:])
    atoms = np.vstack([rattled[keep], rng.random((gone, 3)) @ cell])
    stretch = np.diag([1.01, 0.99, 1.02])  # the current box of the affine query

    def case(tag, site_order, atom_order):
        s, a = sites[site_order], atoms[atom_order]
        site_cols, atom_cols = [up(s[:, k]) for k in range(3)], [up(a[:, k]) for k in range(3)]
        bx = mp.Box(cell)
        out = {"case": tag, "sites": n, "atoms": len(a)}
        tree = _fast_knn.Tree()
        out["build"] = laps(lambda: tree.build_with_coords(*site_cols, bx.box, bx.origin, bx.boundary, 1))
        out["cells"] = int(tree.cell_start.shape[0]) - 1
        index = HArray.empty((len(a),), np.int32)
        out["query"] = laps(lambda: tree.query_nearest_batch(*atom_cols, index, 1))
        m = np.linalg.solve(cell @ stretch, cell)
        mapped = [up((a @ stretch)[:, k]) for k in range(3)]
        out["query_affine"] = laps(lambda: tree.query_nearest_batch(*mapped, index, 1, affine_map=m))
        tree.query_nearest_batch(*atom_cols, index, 1)
        kinds = up(np.ones(n, np.int32))
        occ, aocc, atype = HArray.empty((n,), np.int32), HArray.empty((len(a),), np.int32), HArray.empty((len(a),), np.int32)
        counts = {}
        out["occupancy"] = laps(lambda: counts.update(c=_fast_knn.cal_site_occupancy(index, kinds, occ, aocc, atype)))
        out["vacancies"], out["interstitials"] = counts["c"]
        ref = mp.System(data=Frame(dict(zip("xyz", site_cols))), box=bx)
        ws = mp.WignerSeitzAnalysis(ref)
        cur_frame = Frame(dict(zip("xyz", atom_cols)))
        out["compute"] = laps(lambda: ws.compute(mp.System(data=cur_frame, box=bx)))
        # bytes per atom from the shapes: build reads 24 and writes 24 (wrap), bins (24 read, 8 + 4 written, 28 gathered and written)
        # and packs (28 read, 32 written); a query reads 24 and writes 4 and gathers ~27 cells x 1.5 sites x 32 bytes, mostly from
        # cache; occupancy reads 4, adds 4, reads 4 + 4 + 4 and writes 8 per atom and reads 4 per site
        out["bytes_per_atom"] = {"build": 24 + 24 + 24 + 12 + 2 * 28 + 28 + 32, "query_stream": 28, "query_gather": int(27 * 1.5 * 32), "occupancy": 4 + 4 + 12 + 8 + 4}
        if not args.no_yardsticks:
            full = rattled[site_order]  # as many atoms as sites, in the sites' order
            strain = mp.AtomicStrain(args.rc, ref)
            full_frame = in_hbm(full)
            out["strain"] = laps(lambda: strain.compute(mp.System(data=full_frame, box=bx)))
            ki, kd = HArray.empty((len(a), 1), np.int32), HArray.empty((len(a), 1), np.float64)
            out["knn1"] = laps(lambda: _fast_knn.knn(*atom_cols, bx.box, bx.origin, bx.boundary, 1, ki, kd, 1))
        print(json.dumps(out), flush=True)

    case("ordered", np.arange(n), np.arange(len(atoms)))
    if not args.no_shuffled:
        case("shuffled", np.random.default_rng(1).permutation(n), np.random.default_rng(2).permutation(len(atoms)))


if __name__ == "__main__":
    main()
