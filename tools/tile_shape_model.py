"""Cost model of the tile kernel's VALU work over tile shapes, on the real per-cell populations of the headline lattice (CPU only).

    python tools/tile_shape_model.py [--cells 136] [--slab 8]

A tile's four waves each pay the front phases once (F wave-instructions: halo table, staging, run table) and the tile's centres
are worked off in chunks of 64 lanes (C wave-instructions per chunk: scan, tickets, label, write-out):

    cost per atom = sum over tiles (4 F + ceil(centres / 64) C) / atoms

F = 450 and C = 3120 reproduce the measured 3 294 VALU instructions per wave at the 3.646 chunks per tile of the 4x4x5 shape
(profiles/r07_fused_ledger.md).  Shapes: every (tx, ty, tz) whose halo (tx + 2)(ty + 2)(tz + 2) has at most 256 cells (a halo
cell per thread).  --slab W: the same for the 1-of-W slab of the box along x, with the global tile grid and with the grid's
origin moved to the slab's first plane."""
import argparse
import itertools

import numpy as np

A_CU = 3.615
RC = 0.854 * A_CU
F, C = 450.0, 3120.0


def populations(cells, x0=0, x1=None):
    """atoms per grid cell of the fcc lattice of cells^3 unit cells (lattice cells x0 .. x1 along x), binned as k_assign bins them"""
    x1 = cells if x1 is None else x1
    nc = max(int(np.floor(A_CU * cells / RC)), 3)
    basis = np.array([[0.0, 0.0, 0.0], [0.5, 0.5, 0.0], [0.0, 0.5, 0.5], [0.5, 0.0, 0.5]]) * A_CU
    pop = np.zeros((nc, nc, nc), np.int32)
    iy = np.arange(cells) * A_CU
    ix = np.arange(x0, x1) * A_CU
    for bx, by, bz in basis:
        c = [np.clip(np.floor((v + o) * (1.0 / RC)), 0, nc - 1).astype(np.int64) for v, o in ((ix, bx), (iy, by), (iy, bz))]
        np.add.at(pop, (c[0][:, None, None], c[1][None, :, None], c[2][None, None, :]), 1)
    return pop


def cost(pop, shape, origin=0):
    """wave-instructions per atom; origin: first plane of the tile grid along x"""
    p = pop[origin:] if origin else pop
    pads = [(-p.shape[d]) % shape[d] for d in range(3)]
    p = np.pad(p, [(0, pads[0]), (0, pads[1]), (0, pads[2])])
    t = p.reshape(p.shape[0] // shape[0], shape[0], p.shape[1] // shape[1], shape[1], p.shape[2] // shape[2], shape[2]).sum(axis=(1, 3, 5))
    live = t[t > 0]
    chunks = np.ceil(live / 64.0)
    return float((4 * F * len(live) + C * chunks.sum()) / pop.sum()), float(chunks.mean()), float(live.mean() / (64.0 * chunks.mean()))


def table(pop, origin=0, top=8):
    rows = []
    for s in itertools.product(range(1, 9), repeat=3):
        if (s[0] + 2) * (s[1] + 2) * (s[2] + 2) <= 256:
            rows.append((cost(pop, s, origin), s))
    rows.sort()
    return rows[:top], dict((s, c) for c, s in rows)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--cells", type=int, default=136)
    ap.add_argument("--slab", type=int, default=8)
    a = ap.parse_args()
    pop = populations(a.cells)
    best, every = table(pop)
    print(f"{a.cells}^3 lattice cells, {int(pop.sum())} atoms, {pop.shape[0]}^3 grid cells")
    print(f"  4x4x5 (the kernel's): {every[(4, 4, 5)][0]:.1f} wave-instructions per atom, {every[(4, 4, 5)][1]:.3f} chunks per tile, lane fill {every[(4, 4, 5)][2]:.3f}")
    for (c, ch, fill), s in best:
        print(f"  {s[0]}x{s[1]}x{s[2]}: {c:.1f}  ({ch:.3f} chunks per tile, lane fill {fill:.3f})")
    if a.slab > 1 and a.cells % a.slab == 0:
        cx = a.cells // a.slab
        slab = populations(a.cells, cx, 2 * cx)  # the second slab of the box: its first plane is no multiple of the tile edge
        first = int(np.nonzero(slab.sum(axis=(1, 2)))[0][0])
        print(f"1-of-{a.slab} slab ({int(slab.sum())} atoms, planes from {first}):")
        print(f"  4x4x5, global grid: {cost(slab, (4, 4, 5))[0]:.1f}; origin at the slab's first plane: {cost(slab, (4, 4, 5), first)[0]:.1f}")
        best_s, _ = table(slab, first, top=4)
        for (c, ch, fill), s in best_s:
            print(f"  {s[0]}x{s[1]}x{s[2]} from the slab's first plane: {c:.1f}")


if __name__ == "__main__":
    main()
