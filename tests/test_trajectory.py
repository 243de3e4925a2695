"""The trajectory helper (tests/_trajectory.py) itself, on the CPU: it needs neither torch nor a device, and its `gap` step does
what tests/test_gpu_sequences.py relies on — the slabs keep their atoms while their ghost layers empty."""
import subprocess
import sys
import os

import numpy as np
import pytest

import _trajectory as T

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_helper_imports_without_torch_or_the_package():
    code = ("import sys; sys.path.insert(0, 'tests'); import _trajectory as T; f = T.start('bcc', (4, 4, 4), 1); "
            "assert f.n == 128 and 'torch' not in sys.modules and 'mdapy_amd' not in sys.modules and 'oracle' not in sys.modules")
    run = subprocess.run([sys.executable, "-c", code], cwd=ROOT, capture_output=True, text=True)
    assert run.returncode == 0, run.stderr[-1500:]


@pytest.mark.parametrize("world", [2, 4])
def test_gap_keeps_slab_ownership_and_empties_the_ghost_layers(world):
    import mdapy_amd as mp
    from mdapy_amd.distributed import partition_atoms

    frame, rc = T.decomposed_frame()
    faces = [r / world for r in range(world)]
    gapped = T.gap(frame, 0, faces, rc)
    box = mp.Box(frame.box)
    before, after = partition_atoms(frame.pos, box, world, axis=0), partition_atoms(gapped.pos, box, world, axis=0)
    assert all(np.array_equal(b, a) for b, a in zip(before, after)) and sum(len(b) for b in before) == frame.n

    def near_a_face(f):
        x = f.frac(0)
        x = x - np.floor(x)
        d = np.abs(x[:, None] - np.asarray(faces + [1.0])[None, :]).min(axis=1) * frame.box[0, 0]
        return d < rc

    moved = (gapped.pos != frame.pos).any(axis=1)
    assert near_a_face(frame).sum() > 500 * world and np.array_equal(moved, near_a_face(frame)) and not near_a_face(gapped).any()
    assert np.array_equal(gapped.pos[:, 1:], frame.pos[:, 1:])  # (along the slab axis only)


@pytest.mark.parametrize("box", ["orthogonal", "sheared", "open"])
@pytest.mark.parametrize("kind", ["fcc", "bcc", "gas"])
def test_steps_do_what_they_say(kind, box):
    f = T.start(kind, (6, 5, 4), seed=3)
    f = {"orthogonal": lambda q: q, "sheared": T.sheared, "open": lambda q: T.open_along(q, 2)}[box](f)
    rng = np.random.default_rng(4)
    n = f.n
    assert n == (2 if kind == "bcc" else 4) * 120
    d = T.drift(f, rng)
    assert d.n == n and 0 < np.abs(d.pos - f.pos).max() < 0.5
    j = T.jump(f, rng)
    hops = (j.pos - f.pos) @ np.linalg.inv(f.box)
    assert np.allclose(hops, np.rint(hops), atol=1e-9) and 0 < (np.abs(hops) > 0.5).any(axis=1).sum() < 0.1 * n
    assert not (np.abs(hops[:, f.boundary == 0]) > 0.5).any()
    r = T.renumber(f, rng)
    assert not np.array_equal(r.pos, f.pos) and np.array_equal(np.sort(r.pos[:, 0]), np.sort(f.pos[:, 0]))
    assert T.resize(f, rng).n == int(0.9 * n)
    s = T.reshape(f, rng)
    assert s.n == n and not np.array_equal(s.box, f.box) and np.array_equal(s.boundary, f.boundary) and np.allclose(s.frac(), f.frac(), atol=1e-9)
    p = T.repbc(f, rng, (1, 0, 1))
    assert np.array_equal(p.pos, f.pos) and not np.array_equal(p.boundary, f.boundary)
    h = T.nan_atom(f, rng)
    assert np.isnan(h.pos[:, 0]).sum() == 1 and np.isnan(h.pos).sum() == 1 and (~T.finite(h)).sum() == 1
    seq = T.sequence(f, ["drift", "renumber", "nan_atom"], seed=9)
    again = T.sequence(f, ["drift", "renumber", "nan_atom"], seed=9)
    assert len(seq) == 4 and all(np.array_equal(a.pos, b.pos, equal_nan=True) for a, b in zip(seq, again))


def test_expected_answers_leave_a_nan_atom_out():
    f = T.start("fcc", (6, 6, 6), seed=8)
    rc = 0.854 * 3.615
    whole = T.expected_cutoff(f, rc)
    h = T.nan_atom(f, np.random.default_rng(2))
    gone = int(np.nonzero(~T.finite(h))[0][0])
    e = T.expected_cutoff(h, rc)
    assert e["counts"][gone] == 0 and e["cna"][gone] == 0 and (e["rows"][gone] == -1).all() and not (e["rows"] == gone).any()
    far = ~(whole["rows"] == gone).any(axis=1)
    far[gone] = False
    M = e["rows"].shape[1]
    assert np.array_equal(e["rows"][far], whole["rows"][far][:, :M]) and np.array_equal(e["dist"][far], whole["dist"][far][:, :M])
    k = T.expected_knn(h, 12, csp=12)
    assert not (k["rows"][k["finite"]] == gone).any() and np.isnan(k["csp"][gone]) and np.isfinite(k["csp"][k["finite"]]).all()
