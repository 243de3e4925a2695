"""Atomic strain on the CPU: the host layer — ``AtomicStrain``, its small-box and shuffled-frame paths, where the columns land —
with the neighbour build routed to the oracle (fixture ``oracle_backend``) and ``kernels.strain`` replaced by the numpy
restatement of tests/_strain_ref.py; and the restatement itself against the reference's OVITO-derived fixture and against the
closed form of a homogeneous deformation."""
import os

import numpy as np
import pytest

import _strain_ref
import mdapy_amd as mp
from mdapy_amd import policy
from mdapy_amd import tool_function as tool
from mdapy_amd.build_lattice import lattice_positions
from mdapy_amd.devarray import as_numpy

HERE = os.path.dirname(os.path.abspath(__file__))
GOLDEN = os.path.join(HERE, "golden", "strain")
A = 3.615


@pytest.fixture
def restated(oracle_backend, monkeypatch):
    import mdapy_amd.kernels as K

    monkeypatch.setattr(K, "strain", _strain_ref)
    return _strain_ref


def _columns(s):
    return s.data["shear_strain"].to_numpy(), s.data["volumetric_strain"].to_numpy()


def _deformed(pos, box, seed, noise=0.03):
    """a shear-plus-stretch of box and atoms, and a rattle on top"""
    cell = np.array(box, float)[:3]
    grad = np.array([[1.03, 0.0, 0.0], [0.04, 0.98, 0.0], [-0.02, 0.03, 1.01]])
    moved = pos @ grad + np.random.default_rng(seed).normal(0, noise, pos.shape)
    return moved, cell @ grad, grad


_direct = _strain_ref.on_system_list


@pytest.mark.parametrize("affine", [False, True])
def test_reference_fixture(restated, affine):
    want = np.load(os.path.join(GOLDEN, "atomic_strain.npz"))
    ref = mp.System(os.path.join(GOLDEN, "strain.0.xyz"))
    cur = mp.System(os.path.join(GOLDEN, "strain.1.xyz"))
    mp.AtomicStrain(float(want["cutoff"]), ref, max_neigh=30, affine=affine).compute(cur)
    shear, vol = _columns(cur)
    tag = "_affine" if affine else ""
    d_shear = float(np.abs(shear - want["shear_strain" + tag]).max())
    d_vol = float(np.abs(vol - want["volumetric_strain" + tag]).max())
    print(f"fixture affine={affine}: max |d shear| = {d_shear:.3e}, max |d volumetric| = {d_vol:.3e}")
    assert shear.shape == (256,) and d_shear < 1e-12
    assert d_vol < 1e-12


def test_homogeneous_deformation_has_the_closed_form(restated):
    """an unrattled affine deformation G: every atom's F is G, so s = (G^T G - I) / 2 — an answer the restatement did
    not produce itself; with affine=True the strain vanishes"""
    pos, box = lattice_positions("fcc", A, 5, 5, 5)
    pos = pos + np.random.default_rng(0).normal(0, 0.05, pos.shape)
    moved, cell, grad = _deformed(pos, box, 0, noise=0.0)
    s = (grad.T @ grad - np.eye(3)) / 2.0
    shear0 = np.sqrt(s[0, 1] ** 2 + s[0, 2] ** 2 + s[1, 2] ** 2
                     + ((s[0, 0] - s[1, 1]) ** 2 + (s[0, 0] - s[2, 2]) ** 2 + (s[1, 1] - s[2, 2]) ** 2) / 6.0)
    cur = mp.System(pos=moved, box=mp.Box(cell))
    mp.AtomicStrain(3.1, mp.System(pos=pos, box=box)).compute(cur)
    shear, vol = _columns(cur)
    assert np.abs(shear - shear0).max() < 1e-12 and np.abs(vol - np.trace(s) / 3.0).max() < 1e-12
    cur = mp.System(pos=moved, box=mp.Box(cell))
    mp.AtomicStrain(3.1, mp.System(pos=pos, box=box), affine=True).compute(cur)
    shear, vol = _columns(cur)
    assert np.abs(shear).max() < 1e-12 and np.abs(vol).max() < 1e-12


def test_unequal_atom_numbers_are_refused(restated):
    pos, box = lattice_positions("fcc", A, 4, 4, 4)
    strain = mp.AtomicStrain(3.1, mp.System(pos=pos, box=box))
    with pytest.raises(AssertionError):
        strain.compute(mp.System(pos=pos[:-1], box=box))


def test_columns_land_on_current_only_and_ref_keeps_its_list(restated):
    pos, box = lattice_positions("fcc", A, 4, 4, 4)
    moved, cell, _ = _deformed(pos, box, 1)
    ref = mp.System(pos=pos, box=box)
    strain = mp.AtomicStrain(3.1, ref, max_neigh=20)
    assert ref.rc == 3.1 and ref.verlet_list.shape == (len(pos), 20)
    assert strain.rc == 3.1 and strain.max_neigh == 20 and strain.affine is False and policy.is_single(strain.repeat)
    rows, columns = ref.verlet_list, list(ref.data.columns)
    cur = mp.System(pos=moved, box=mp.Box(cell))
    assert strain.compute(cur) is None
    assert ref.verlet_list is rows and list(ref.data.columns) == columns
    assert "verlet_list" not in cur.__dict__
    assert list(cur.data.columns) == ["x", "y", "z", "shear_strain", "volumetric_strain"]
    shear, vol = _columns(cur)
    assert shear.dtype == np.float64 and shear.shape == (len(pos),) and vol.shape == (len(pos),)
    want = _direct(strain, cur)
    assert np.array_equal(shear, want[0]) and np.array_equal(vol, want[1])
    assert (shear > 0).all()


def test_small_box_equals_the_explicitly_replicated_pair(restated):
    pos, box = lattice_positions("fcc", A, 2, 2, 2)  # 7.23 A: a 3.7 A list is built on a replica
    pos = pos + np.random.default_rng(5).normal(0, 0.05, pos.shape)
    moved, cell, _ = _deformed(pos, box, 6)
    for affine in (False, True):
        ref = mp.System(pos=pos, box=box)
        strain = mp.AtomicStrain(3.7, ref, affine=affine)
        assert "_enlarge_data" in ref.__dict__ and tuple(int(c) for c in strain.repeat) == (2, 2, 2)
        cur = mp.System(pos=moved, box=mp.Box(cell))
        strain.compute(cur)
        big_ref = mp.System(pos=ref._enlarge_data.select("x", "y", "z").to_numpy(), box=ref._enlarge_box)
        big_data, big_box = tool._replicate_pos(cur.data, cur.box, 2, 2, 2)
        big_cur = mp.System(pos=big_data.to_numpy(), box=big_box)
        big = mp.AtomicStrain(3.7, big_ref, affine=affine)
        assert "_enlarge_data" not in big_ref.__dict__
        big.compute(big_cur)
        n = len(pos)
        for got, want in zip(_columns(cur), _columns(big_cur)):
            assert got.shape == (n,) and np.array_equal(got, want[:n])
        assert _columns(cur)[0].max() > 1e-3


def test_an_atom_without_neighbours(restated):
    rng = np.random.default_rng(2)
    pos = np.vstack([rng.random((40, 3)) * 6.0, [[50.0, 50.0, 50.0]]])
    box = mp.Box(np.diag([60.0] * 3), [0, 0, 0])
    ref = mp.System(pos=pos, box=box)
    cur = mp.System(pos=pos * 1.01 + rng.normal(0, 0.02, pos.shape), box=box)
    mp.AtomicStrain(2.5, ref).compute(cur)
    assert int(as_numpy(ref.neighbor_number)[-1]) == 0
    shear, vol = _columns(cur)
    assert shear[-1] == 0.0 and vol[-1] == -0.5


def test_a_coplanar_neighbourhood_takes_the_identity_branch(restated):
    """one open-boundary layer: every bond lies in z = 0, det V is exactly 0, V^-1 is the identity and F = W^T"""
    grid = np.stack(np.meshgrid(np.arange(6.0), np.arange(6.0), indexing="ij"), -1).reshape(-1, 2) * 2.5
    pos = np.column_stack([grid + np.random.default_rng(3).normal(0, 0.1, grid.shape), np.zeros(len(grid))])
    box = mp.Box(np.diag([20.0, 20.0, 20.0]), [0, 0, 0])
    ref = mp.System(pos=pos, box=box)
    moved = pos * np.array([1.02, 0.97, 1.0])
    cur = mp.System(pos=moved, box=box)
    strain = mp.AtomicStrain(3.0, ref)
    strain.compute(cur)
    rows, counts = as_numpy(ref.verlet_list), as_numpy(ref.neighbor_number)
    V, W, used = _strain_ref.accumulate(rows, counts, box.box, box.box, box.boundary, *pos.T, *moved.T)
    assert np.array_equal(used, counts) and counts.min() >= 2
    assert _strain_ref.invariants(V, W)[2].all()
    # the same from plain linear algebra: s = (W W^T - I) / 2 per atom
    for i in (0, 7, 35):
        d_ref = pos[rows[i, : counts[i]]] - pos[i]
        d_cur = moved[rows[i, : counts[i]]] - moved[i]
        w = d_cur.T @ d_ref
        s = (w @ w.T - np.eye(3)) / 2.0
        shear = np.sqrt(s[0, 1] ** 2 + s[0, 2] ** 2 + s[1, 2] ** 2
                        + ((s[0, 0] - s[1, 1]) ** 2 + (s[0, 0] - s[2, 2]) ** 2 + (s[1, 1] - s[2, 2]) ** 2) / 6.0)
        assert abs(_columns(cur)[0][i] - shear) < 1e-9 * shear and abs(_columns(cur)[1][i] - np.trace(s) / 3.0) < 1e-9 * abs(np.trace(s))


def test_shuffled_reference_runs_on_the_twin(restated, monkeypatch):
    monkeypatch.setenv("MDAPY_SPATIAL_SORT", "1")
    pos, box = lattice_positions("fcc", A, 5, 5, 5)
    pos = pos + np.random.default_rng(8).normal(0, 0.05, pos.shape)
    moved, cell, _ = _deformed(pos, box, 9)
    order = np.random.default_rng(10).permutation(len(pos))
    for affine in (False, True):
        ref = mp.System(pos=pos[order], box=box)
        strain = mp.AtomicStrain(3.1, ref, affine=affine)
        assert ref._spatial() is not None and ref._twin.shown.mirror is ref.verlet_list
        cur = mp.System(pos=moved[order], box=mp.Box(cell))
        strain.compute(cur)
        want = _direct(strain, cur)  # on the translated rows, in the shuffled numbering
        got = _columns(cur)
        assert np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1])
        # and the plain system, atom for atom (its rows may list the same neighbours in another order: to rounding)
        plain = mp.System(pos=moved, box=mp.Box(cell))
        monkeypatch.setenv("MDAPY_SPATIAL_SORT", "0")
        mp.AtomicStrain(3.1, mp.System(pos=pos, box=box), affine=affine).compute(plain)
        monkeypatch.setenv("MDAPY_SPATIAL_SORT", "1")
        assert np.abs(got[0] - _columns(plain)[0][order]).max() < 1e-12 and np.abs(got[1] - _columns(plain)[1][order]).max() < 1e-12
