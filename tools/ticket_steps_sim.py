#!/usr/bin/env python
"""Ticket steps of the tile kernel under a fixed step count per run (profiles/tile_front.md, item 5).  The ticket stage of
neighbor_lane.hip runs three unconditional steps for each of a centre's nine runs and a ballot loop for runs in which some lane of
the wave has more hits: a wave executes max(3, most hits of any lane) steps per run.  With f(r) unconditional steps it would execute
max(f(r), most hits).  This counts both on the CPU (numpy + scipy), in the kernel's own centre order — tiles of 4 x 4 x 5 cells, the
centres of a tile by halo cell (z fastest), chunks of 64 — for the headline lattice, the lattice rattled by 0.05 and 0.20 A and a
polycrystal made the way bench.py's is (Voronoi grains with random rotations in the same box, atoms closer than 2.0 A to an atom of
another grain removed), each in a box of 28 unit cells (87 808 lattice sites; the statistics are per chunk, not per box).  The
polycrystal here has 8 grains in a (101 A)^3 box; bench.py's has one grain per 2.3e6 A^3, grains about ten times larger in volume, so
this one has roughly twice the grain-boundary fraction per atom and overstates what the boundaries add.

    python tools/ticket_steps_sim.py"""
import numpy as np
from scipy.spatial import cKDTree
from scipy.spatial.transform import Rotation

A, NCELL = 3.615, 28
RC = 0.854 * A
L = A * NCELL
TXY, TZ = 4, 5


def lattice(sigma, seed=0):
    i = np.stack(np.meshgrid(*[np.arange(NCELL)] * 3, indexing="ij"), -1).reshape(-1, 1, 3)
    basis = np.array([[0, 0, 0], [.5, .5, 0], [.5, 0, .5], [0, .5, .5]])
    pos = ((i + basis[None]) * A).reshape(-1, 3)
    if sigma:
        pos = pos + np.random.default_rng(seed).normal(0, sigma, pos.shape)
    return pos % L


def polycrystal(grains=8, seed=2024):
    rng = np.random.default_rng(seed)
    seeds = rng.random((grains, 3)) * L
    tree = cKDTree(seeds, boxsize=L)
    i = np.stack(np.meshgrid(*[np.arange(-NCELL, NCELL)] * 3, indexing="ij"), -1).reshape(-1, 1, 3)
    basis = np.array([[0, 0, 0], [.5, .5, 0], [.5, 0, .5], [0, .5, .5]])
    cube = ((i + basis[None]) * A).reshape(-1, 3)
    parts, owner = [], []
    for g in range(grains):
        p = Rotation.from_euler("xyz", rng.uniform(-180, 180, 3), degrees=True).apply(cube) + seeds[g]
        p = p[(np.abs(p - seeds[g]) < L / 2).all(1)] % L
        p = p[tree.query(p)[1] == g]
        parts.append(p); owner.append(np.full(len(p), g))
    pos, owner = np.concatenate(parts), np.concatenate(owner)
    keep = np.ones(len(pos), bool)
    for a, b in cKDTree(pos, boxsize=L).query_pairs(2.0):
        if owner[a] != owner[b] and keep[a] and keep[b]:
            keep[max(a, b)] = False
    return pos[keep]


def count(name, pos):
    nc = int(np.floor(L / RC))
    cell = np.minimum((pos / (L / nc) * (L / nc / RC)).astype(int), nc - 1)  # rc-wide cells, the last takes the rest (neighbor.cpp:29-62)
    pairs = cKDTree(pos, boxsize=L).query_pairs(RC, output_type="ndarray")
    pairs = np.concatenate([pairs, pairs[:, ::-1]])
    d = cell[pairs[:, 1]] - cell[pairs[:, 0]]
    d = (d + nc // 2) % nc - nc // 2
    ok = (np.abs(d) <= 1).all(1)  # (a pair two cells apart in the wide last cell of an axis: not in this count)
    run = (d[:, 0] + 1) * 3 + (d[:, 1] + 1)
    hits = np.zeros((len(pos), 9), int)
    np.add.at(hits, (pairs[ok, 0], run[ok]), 1)
    # the kernel's centre order: tile, then halo cell (x, y, z with z fastest), then the atoms of the cell
    tile = (cell[:, 0] // TXY, cell[:, 1] // TXY, cell[:, 2] // TZ)
    order = np.lexsort((-np.arange(len(pos)), cell[:, 2], cell[:, 1], cell[:, 0], tile[2], tile[1], tile[0]))
    tid = (tile[0] * 1000 + tile[1]) * 1000 + tile[2]
    today = fixed = loop_today = loop_fixed = chunks = 0
    worst = np.zeros(9, int)
    mean = np.zeros(9)
    f = np.array([1, 3, 1, 3, 3, 3, 1, 3, 1])  # one step for the corner columns (da, db) = (+-1, +-1), three elsewhere
    tids = tid[order]
    cuts = np.flatnonzero(np.diff(tids)) + 1
    for s, e in zip(np.r_[0, cuts], np.r_[cuts, len(order)]):
        for c0 in range(s, e, 64):
            mx = hits[order[c0:min(c0 + 64, e)]].max(0)
            today += np.maximum(3, mx).sum(); fixed += np.maximum(f, mx).sum()
            loop_today += np.maximum(0, mx - 3).sum(); loop_fixed += np.maximum(0, mx - f).sum()
            worst = np.maximum(worst, mx); mean += mx; chunks += 1
    print(f"{name:12s} atoms {len(pos):7d} chunks {chunks:5d}  steps per chunk: today {today / chunks:6.2f}  fixed {fixed / chunks:6.2f}"
          f"  of them in the ballot loop: today {loop_today / chunks:5.2f}  fixed {loop_fixed / chunks:5.2f}")
    print(f"{'':12s} most hits of a lane, per run: mean over chunks {np.round(mean / chunks, 2).tolist()}  largest {worst.tolist()}")


if __name__ == "__main__":
    count("lattice", lattice(0.0))
    count("sigma 0.05", lattice(0.05))
    count("sigma 0.20", lattice(0.20))
    count("polycrystal", polycrystal())
