"""TEST INFRASTRUCTURE: the inputs the void-analysis tests share, and — computed once per process — what tests/_void_ref.py makes
of them.  ``FIXED`` maps a name to (atoms, voids, cells kept): counts that were checked on the CPU with an independent numpy /
scipy restatement."""
import functools

import numpy as np

import _void_ref
import mdapy_amd as mp
from mdapy_amd.build_lattice import lattice_positions

A, RC = 4.05, 4.1


@functools.lru_cache(maxsize=None)
def _fcc(cells):
    pos, box = lattice_positions("fcc", A, cells, cells, cells)
    return np.ascontiguousarray(pos, np.float64), np.array(box, np.float64)[:3]


def _without_spheres(pos, edge, spheres, minimum_image=False):
    keep = np.ones(len(pos), bool)
    for centre, radius in spheres:
        d = pos - np.asarray(centre, np.float64)
        if minimum_image:
            d -= edge * np.round(d / edge)
        keep &= np.linalg.norm(d, axis=1) > radius
    return pos[keep]


def _without_cells(pos, cell, rc, cells):
    idx = _void_ref.cell_indices(cell, rc, pos[:, 0], pos[:, 1], pos[:, 2])
    gone = np.zeros(len(pos), bool)
    for c in cells:
        gone |= np.all(idx == np.asarray(c), axis=1)
    return pos[~gone]


SINGLE_CELLS = ((1, 1, 1), (4, 4, 4), (7, 2, 9), (7, 3, 9), (9, 9, 2), (9, 9, 3), (9, 8, 3))

# name -> (atoms, void_number, points kept)
FIXED = {
    "full": (6912, 0, 0),
    "three_spheres": (6613, 3, 44),
    "corner_periodic": (6357, 1, 38),
    "corner_open": (6357, 8, 38),
    "corner_small_open": (None, 4, 13),
    "single_cells": (None, 2, 5),
    "reference_scaled": (54584, 3, 115),
}


@functools.lru_cache(maxsize=None)
def fixed(name):
    """(positions (N, 3), Box, rc) of a fixed case"""
    cells = 24 if name == "reference_scaled" else 12
    pos, box = _fcc(cells)
    edge = A * cells
    boundary = [0, 0, 0] if name.endswith("_open") else [1, 1, 1]
    cell = mp.Box(box, boundary)
    if name == "three_spheres":
        pos = _without_spheres(pos, edge, [((12, 12, 12), 6), ((30, 30, 30), 6), ((34, 12, 12), 9)])
    elif name in ("corner_periodic", "corner_open"):
        pos = _without_spheres(pos, edge, [((0, 0, 0), 13)], minimum_image=True)
    elif name == "corner_small_open":
        pos = _without_spheres(pos, edge, [((0, 0, 0), 11)], minimum_image=True)
    elif name == "single_cells":
        pos = _without_cells(pos, cell, RC, SINGLE_CELLS)
    elif name == "reference_scaled":
        pos = _without_spheres(pos, edge, [((25, 25, 25), 8), ((50, 50, 50), 8), ((72, 72, 72), 12)])
    else:
        assert name == "full"
    pos = np.ascontiguousarray(pos)
    pos.setflags(write=False)
    return pos, cell, RC


@functools.lru_cache(maxsize=None)
def restated(name):
    pos, cell, rc = fixed(name)
    return _void_ref.analyse(pos, cell, rc)
