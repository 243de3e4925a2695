"""-m gpu: the state a slot-grid build carries from call to call (cell_grid.hip): the history per (N, grid) that picks the grid
form, the two counter arrays that alternate from one slot build to the next — the in-cell sort of a build clears the array the
next one counts into — and what a failed call leaves behind.  Every result (rows, distances, counts, labels; bitwise) equals
that of a FRESH process's compact build of the same input (MDH_SLOT_GRID=0: one child process makes all of them, once)."""
import ctypes
import os
import subprocess
import sys

import numpy as np
import pytest

from mdapy_amd import _lib, _neighbor
from mdapy_amd.build_lattice import lattice_positions

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
PBC = np.array([1, 1, 1], np.int32)
ORG0 = np.zeros(3)
A_CU = 3.615
RC = 0.854 * A_CU
M = 16


def _inputs():
    """name -> (positions, box): rattled fcc Cu, every system with an N of its own; 6, 7 and 12 lattice cells leave no grid cell
    much wider than the others, so no cell holds more than eight atoms"""
    out = {}
    for name, dims, seed in (("a", (12, 12, 6), 31), ("b", (12, 6, 6), 32), ("c", (12, 12, 7), 33), ("d", (12, 12, 12), 34), ("e", (6, 6, 6), 35)):
        pos, box = lattice_positions("fcc", A_CU, *dims)
        pos = pos + np.random.default_rng(seed).normal(0.0, 0.05, pos.shape)
        out[name] = (np.ascontiguousarray(pos), np.asarray(box, float))
    # "a" a step later: the same system, other positions
    out["a2"] = (np.ascontiguousarray(out["a"][0] + np.random.default_rng(36).normal(0.0, 0.02, out["a"][0].shape)), out["a"][1])
    return out


def _build(pos, box):
    x, y, z = (np.ascontiguousarray(pos[:, k]) for k in range(3))
    n = len(x)
    v = np.empty((n, M), np.int32); d = np.empty((n, M)); c = np.zeros(n, np.int32); p = np.zeros(n, np.int32)
    _neighbor.build_neighbor_fcna(x, y, z, box, ORG0, PBC, RC, v, d, c, p, 1, fill_pads=True)
    plan = np.zeros(8, np.int32)
    _lib.lib().mdh_debug_neighbor_plan(plan.ctypes.data)
    assert plan[0] > 0, plan.tolist()
    return (v, d, c, p), bool(plan[4] & 256)


def _write_reference(path):
    """(the child process) every input through one compact build"""
    assert os.environ.get("MDH_SLOT_GRID") == "0"
    arrays = {}
    for name, (pos, box) in _inputs().items():
        out, slot = _build(pos, box)
        assert not slot
        for key, a in zip("vdcp", out):
            arrays[name + "_" + key] = a
    np.savez(path, **arrays)


@pytest.fixture(scope="module")
def reference(tmp_path_factory):
    path = str(tmp_path_factory.mktemp("slot_grid") / "reference.npz")
    code = "import sys; sys.path[:0] = [%r, %r]; import test_gpu_slot_grid_sequences as t; t._write_reference(%r)" % (ROOT, HERE, path)
    run = subprocess.run([sys.executable, "-c", code], cwd=ROOT, env=dict(os.environ, MDH_SLOT_GRID="0"), capture_output=True, text=True, timeout=600)
    assert run.returncode == 0, (run.stdout + run.stderr)[-2000:]
    with np.load(path) as z:
        return {k: z[k] for k in z.files}


@pytest.fixture(autouse=True)
def fresh_history():
    """every signature's history forgotten: a test's first build of a system is a compact one whatever ran before"""
    _lib.lib().mdh_debug_set_slot_grid(2)
    yield
    _lib.lib().mdh_debug_set_slot_grid(1)


def _run(reference, inputs, sequence):
    """sequence: (input name, expected form) per call"""
    for k, (name, want) in enumerate(sequence):
        out, slot = _build(*inputs[name])
        assert slot == want, (k, name, "slot grid" if slot else "compact")
        for key, a in zip("vdcp", out):
            assert np.array_equal(a, reference[name + "_" + key]), (k, name, key)


def test_slot_slot_compact_of_another_n_slot_slot(reference):
    """the first build of "b" in the middle is a compact one (its own scan, its own counters); the slot builds around it find the
    counter array their predecessor's sort cleared"""
    _run(reference, _inputs(), [("a", False), ("a", True), ("a2", True), ("b", False), ("a", True), ("a2", True), ("b", True)])


def test_slot_build_after_a_failed_call(reference):
    """a call that fails between its grid build and its rows — the exact-width driver whose row allocator refuses — and the slot
    builds behind it"""
    inputs = _inputs()
    _run(reference, inputs, [("c", False), ("c", True)])
    pos, box = inputs["c"]
    x, y, z = (np.ascontiguousarray(pos[:, k]) for k in range(3))
    nn = np.zeros(len(x), np.int32)
    width = ctypes.c_int64(0)
    refuse = _lib.ALLOC_ROWS(lambda user, n, m, pv, pd: 1)
    keep, (pb, po, pp) = _lib.host_box(box, ORG0, PBC)
    rc_ = _lib.lib().mdh_build_neighbor_exact_fcna(x.ctypes.data, y.ctypes.data, z.ctypes.data, len(x), pb, po, pp, float(RC), nn.ctypes.data,
                                                   ctypes.addressof(width), refuse, None, None, None, 0, None)
    assert rc_ != 0
    _run(reference, inputs, [("c", True), ("c", True)])


def test_two_systems_interleaved(reference):
    """two Systems of different N, call about: each keeps its own history, and they hand the counter arrays to each other"""
    _run(reference, _inputs(), [("d", False), ("e", False), ("d", True), ("e", True), ("d", True), ("e", True)])
