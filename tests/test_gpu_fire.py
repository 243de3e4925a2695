"""The FIRE minimizer on the GPU: the kernels of csrc/fire.hip alone against the numpy restatement (tests/_fire_ref.py), whole runs
of the HBM path bit for bit against the restatement driving a second System through the public ``get_force()``, that it relaxes
atoms and cell, and the paths (replica, twin, host path, residency)."""
import math
import os

import numpy as np
import pytest

import _eam_ref
import _fire_ref as R
import mdapy_amd as mp
from mdapy_amd.build_lattice import lattice_positions

pytestmark = pytest.mark.gpu
EPS = np.finfo(np.float64).eps
NICKEL = os.path.join(_eam_ref.GOLDEN, "NiCoCr.lammps.eam.gz")
SIZES = [1, 2, 63, 64, 65, 255, 256, 257, 1023, 1025, 4099, 256 + 3]


def _dev(a):
    from mdapy_amd.devarray import HArray

    return HArray.from_numpy(np.ascontiguousarray(a))


def _host(h):
    return h.dev().cpu().numpy()


def _same_bits(got, want):
    """array_equal that also tells a NaN from a number and counts nothing else as equal"""
    got, want = np.asarray(got, np.float64), np.asarray(want, np.float64)
    return got.shape == want.shape and np.array_equal(got, want, equal_nan=True)


def _draw(n, kind, seed):
    """(v, f): values over twelve orders of magnitude; ``kind``: plain, signed zeros sprinkled in, v all zero, v with one zero"""
    rng = np.random.default_rng(seed)
    make = lambda: rng.standard_normal((n, 3)) * 10.0 ** rng.uniform(-6, 6, (n, 3))
    v, f = make(), make()
    if kind == "signed-zeros":
        for a in (v, f):
            a[rng.random((n, 3)) < 0.2] = 0.0
            a[rng.random((n, 3)) < 0.1] = -0.0
    elif kind == "v-zero":
        v[...] = 0.0
    elif kind == "one-zero":
        v[rng.integers(n), rng.integers(3)] = 0.0
    return v, f


def _any_order_bound(terms, got):
    """|got - exact| <= (n - 1) eps sum |t_i|: what every order of adding n numbers keeps"""
    terms = np.asarray(terms, np.float64).ravel()
    exact = math.fsum(terms.tolist())
    return abs(got - exact) <= (len(terms) - 1) * EPS * math.fsum(np.abs(terms).tolist()) + 0.0


# ---------------------------------------------------------------------------------------------- 1. the kernels alone
@pytest.mark.parametrize("kind", ["plain", "signed-zeros", "v-zero", "one-zero"])
@pytest.mark.parametrize("n", SIZES)
def test_kernels_against_the_restatement(n, kind):
    from mdapy_amd import kernels

    K = kernels.fire
    v0, f = _draw(n, kind, 1000 + n)
    dt, a, mult = 0.0625 + 1e-3, 0.2401, 1.0 / (1.0 - (1.0 - 0.2401) ** 4)
    for use_abc in (False, True):
        for attempt in range(2):  # (twice: the same bits)
            rec_d, rec = _dev(np.zeros(R.RECORD)), np.zeros(R.RECORD)
            vd, fd, v = _dev(v0), _dev(f), v0.copy()
            K.dots(None, fd, rec_d)
            R.dots(None, f, rec)
            assert _same_bits(_host(rec_d), rec)
            K.dots(vd, fd, rec_d)
            R.dots(v, f, rec)
            assert _same_bits(_host(rec_d), rec), (_host(rec_d), rec)
            assert _any_order_bound(R.row_terms(v, f), rec[R.VF]) and _any_order_bound(R.row_terms(f, f), rec[R.FF])
            assert rec[R.FMAX2] == R.row_terms(f, f).max()
            zero_first = attempt == 1
            K.kick(vd, fd, dt, zero_first, rec_d)
            R.kick(v, f, dt, zero_first, rec)
            assert _same_bits(_host(vd), v) and _same_bits(_host(rec_d), rec)
            assert _any_order_bound(R.row_terms(v, v), rec[R.VV])
            K.mix(vd, fd, a, mult, use_abc, dt, rec_d)
            R.mix(v, f, a, mult, use_abc, dt, rec)
            assert _same_bits(_host(vd), v) and _same_bits(_host(rec_d), rec)
            assert rec[R.ZEROS] == float((v == 0.0).sum()) and _any_order_bound(R.row_terms(dt * v, dt * v), rec[R.DRDR])
            norm = np.sqrt(rec[R.DRDR])
            x = np.random.default_rng(n).standard_normal((3, n)) * 10.0
            for mode, maxstep in ((R.MOVE_NORM, norm * (1 + 1e-12)), (R.MOVE_NORM, norm * (1 - 1e-12)), (R.MOVE_NORM, norm),
                                  (R.MOVE_CAP, np.median(np.abs(v)) * dt), (R.MOVE_PLAIN, 0.2)):
                scale = -0.5 * dt if mode == R.MOVE_PLAIN else dt
                for cell in (False, True):
                    atoms = n - 3 if cell and n > 3 else n
                    wd, w = _dev(v), v.copy()
                    dr_d, dr = _dev(np.zeros((n, 3))), np.zeros((n, 3))
                    if cell:
                        u = np.ascontiguousarray(x.T[:atoms])
                        ud = _dev(u)
                        K.move(wd, dr_d, atoms, scale, dt, maxstep, mode, rec_d, unstrained=ud)
                        R.move(w, dr, atoms, scale, dt, maxstep, mode, rec, unstrained=u)
                        assert _same_bits(_host(ud), u)
                    else:
                        cols = [_dev(c[:atoms]) for c in x]
                        outs, want = [_dev(np.zeros(atoms)) for _ in range(3)], [np.zeros(atoms) for _ in range(3)]
                        K.move(wd, dr_d, atoms, scale, dt, maxstep, mode, rec_d, *cols, *outs)
                        R.move(w, dr, atoms, scale, dt, maxstep, mode, rec, *(c[:atoms] for c in x), *want)
                        assert all(_same_bits(_host(o), c) for o, c in zip(outs, want))
                    assert _same_bits(_host(wd), w) and _same_bits(_host(dr_d), dr)
                    if mode == R.MOVE_NORM and np.isfinite(norm) and norm > 0:
                        assert (np.sqrt(R.tree_dot(dr, dr)) <= maxstep * (1 + 1e-9)) and (maxstep >= norm) == _same_bits(dr, dt * v)


@pytest.mark.parametrize("n", SIZES)
def test_row_transform_scatter_and_plain_sum(n):
    from mdapy_amd import kernels

    K = kernels.fire
    rng = np.random.default_rng(n)
    rows = rng.standard_normal((n, 3)) * 10.0 ** rng.uniform(-6, 6, (n, 3))
    m = np.eye(3) + rng.standard_normal((3, 3)) * 0.1
    out_d, out = _dev(np.zeros((n, 3))), np.zeros((n, 3))
    K.rowmat(_dev(rows), m, out_rows=out_d)
    R.rowmat(rows, m, out_rows=out)
    assert _same_bits(_host(out_d), out) and np.allclose(out, rows @ m, rtol=1e-9, atol=1e-9 * np.abs(rows).max())
    cols = [_dev(np.zeros(n)) for _ in range(3)]
    K.rowmat(_dev(rows), m, out_x=cols[0], out_y=cols[1], out_z=cols[2])
    assert all(_same_bits(_host(c), out[:, k]) for k, c in enumerate(cols))
    perm = rng.permutation(n).astype(np.int32)
    back_d, back = _dev(np.zeros((n, 3))), np.zeros((n, 3))
    K.scatter_rows(_dev(rows), _dev(perm), back_d)
    R.scatter_rows(rows, perm, back)
    assert _same_bits(_host(back_d), back) and _same_bits(back[perm], rows)
    rec_d, rec = _dev(np.zeros(R.RECORD)), np.zeros(R.RECORD)
    K.total(_dev(rows[:, 0].copy()), R.ENERGY, rec_d)
    R.total(rows[:, 0], R.ENERGY, rec)
    assert _same_bits(_host(rec_d), rec) and _any_order_bound(rows[:, 0], rec[R.ENERGY])


def test_kernels_refuse_what_they_cannot_do():
    from mdapy_amd import kernels

    with pytest.raises(ValueError):
        kernels.fire.dots(None, _dev(np.zeros((4, 2))), _dev(np.zeros(R.RECORD)))
    with pytest.raises(ValueError):
        kernels.fire.dots(_dev(np.zeros((5, 3))), _dev(np.zeros((4, 3))), _dev(np.zeros(R.RECORD)))
    with pytest.raises(ValueError):
        kernels.fire.total(_dev(np.zeros(4)), R.RECORD, _dev(np.zeros(R.RECORD)))


# ---------------------------------------------------------------------------------------------- 2. whole runs, bit for bit
def _pair(path, pos, box, names):
    out = []
    for _ in range(2):
        s = mp.System(pos=pos, box=box)
        s.set_element(names)
        s.calc = mp.EAM(path)
        out.append(s)
    return out


def _positions(system):
    return np.column_stack([system.data[c].to_numpy() for c in "xyz"])


def _exact(system, steps, **kwargs):
    return R.run(system, steps, fmax=0.0, dot=R.tree_dot, matmul=R.row_times_matrix, keep_unstrained=True, **kwargs)


def _same_state(fire, system, ref, other):
    assert np.array_equal(_positions(system), _positions(other))
    assert np.array_equal(system.box.box, other.box.box)
    assert np.array_equal(np.asarray(fire.v), ref["v"])
    assert (fire.dt, fire.a, fire.Nsteps) == (ref["dt"], ref["a"], ref["Nsteps"])


def _alloy(sheared):
    pos, box, names = _eam_ref.hea(6, ["Co", "Ni", "Cr"], [0.2, 0.3, 0.5], False)
    pos = pos + np.random.default_rng(11).normal(0, 0.1, pos.shape)
    if sheared:
        cell = np.array(box.box if hasattr(box, "box") else box, np.float64).reshape(3, 3)
        tilted = cell.copy()
        tilted[1, 0], tilted[2, 0], tilted[2, 1] = 0.08 * cell[0, 0], -0.05 * cell[0, 0], 0.06 * cell[1, 1]
        pos = np.linalg.solve(cell.T, pos.T).T @ tilted
        box = mp.Box(tilted)
    return pos, box, names


@pytest.mark.parametrize("sheared", [False, True], ids=["orthogonal", "sheared"])
@pytest.mark.parametrize("kwargs,steps", [(dict(), 25), (dict(use_abc=True), 25), (dict(optimize_cell=True), 10),
                                          (dict(optimize_cell=True, use_abc=True), 10)], ids=["fire2", "abc", "fire2-cell", "abc-cell"])
def test_whole_run_bit_for_bit(sheared, kwargs, steps):
    s, t = _pair(NICKEL, *_alloy(sheared))
    fire = mp.FIRE(s, **kwargs)
    assert fire.run(steps, fmax=0, show_process=False) is False and fire._hbm
    _same_state(fire, s, _exact(t, steps, **kwargs), t)
    assert type(s.data["x"]._dev).__name__ == "HArray"  # (the final positions are device-backed columns)


# ---------------------------------------------------------------------------------------------- 3. it relaxes
def _nickel(a, rattle):
    lattice, box = lattice_positions("fcc", a, 4, 4, 4)
    pos = lattice + np.random.default_rng(0).normal(0, rattle, lattice.shape)
    s = mp.System(pos=pos, box=box)
    s.set_element(np.array(["Ni"] * len(pos), dtype=object))
    s.calc = mp.EAM(NICKEL)
    return s, lattice


def _fresh(system):
    s = mp.System(pos=_positions(system), box=system.box)
    s.set_element(np.array(["Ni"] * system.N, dtype=object))
    s.calc = mp.EAM(NICKEL)
    return s


FIRE2_STEPS, ABC_STEPS = 56, 60  # (the step the restatement converges at on the CPU, see the docstring)


@pytest.mark.parametrize("use_abc", [False, True], ids=["fire2", "abc"])
def test_it_relaxes(use_abc, capsys):
    """256 Ni atoms, a = 3.52 A, rattled by 0.05 A.  The numpy restatement with the numpy EAM, on the CPU: FIRE2 converges at step 56
    (uphill at steps 8 and 31), 2.5e-4 A from the lattice, E = -1139.20065 eV; bounds: fourfold.  ABC-FIRE converges at step 60 (uphill at steps 2, 5, 11 and 39), 5.6e-4 A from the lattice,
    E = -1139.20064 eV; twice its step count is allowed, and the same displacement bound of 1e-3 A holds."""
    s, lattice = _nickel(3.52, 0.05)
    start = s.get_energy()
    assert mp.FIRE(s, use_abc=use_abc).run(200, fmax=1e-3) is True
    table = capsys.readouterr().out.splitlines()
    assert table[-1] == "Converged!"
    steps = len(table) - 3  # (header, the step lines 0 .. steps, "Converged!")
    print(f"converged at step {steps}")
    assert steps <= (2 * ABC_STEPS if use_abc else 4 * FIRE2_STEPS)
    assert set(s.calc.results) == {"energies", "forces", "virials", "stress"}
    fresh = _fresh(s)
    for name, getter in (("energies", "get_energies"), ("forces", "get_force"), ("virials", "get_virials"), ("stress", "get_stress")):
        assert np.array_equal(s.calc.results[name], getattr(fresh, getter)()), name  # (results answer for the final frame: the same bits)
    assert np.sqrt((fresh.get_force()**2).sum(axis=1).max()) < 1e-3
    assert fresh.get_energy() < start
    moved = _positions(s) - lattice
    moved -= moved.mean(axis=0)
    assert np.sqrt((moved**2).sum(axis=1)).max() < 4 * 2.5e-4


def test_the_cell_relaxes():
    """the same crystal at a = 3.60 A, rattled by 0.02 A, with optimize_cell.  The CPU restatement converges at step 170 to a box edge of
    14.0265 A (a = 3.50663), off-diagonals 5e-7 A, pressure from -0.075 to -8.7e-5 eV/A^3."""
    s, _ = _nickel(3.60, 0.02)
    fmax = 1e-3
    assert mp.FIRE(s, optimize_cell=True).run(400, fmax=fmax, show_process=False) is True
    fresh = _fresh(s)
    volume, n = fresh.box.volume, fresh.N
    # the cell rows' forces are virial / cell_factor with cell_factor = N, each below fmax, and the deformation gradient is below one
    # (the cell shrank): every stress component is below fmax N / volume
    assert np.abs(fresh.get_stress()).max() < fmax * n / volume
    cell = fresh.box.box
    assert np.abs(cell - np.diag(np.diag(cell))).max() < 1e-5
    got = np.diag(cell).mean() / 4.0
    # the perfect crystal's energy at five lattice constants: E(a) = c2 a^2 + c1 a + c0 around its minimum
    grid = 3.507 + 0.01 * np.arange(-2, 3)
    energy = []
    for a in grid:
        pos, box = lattice_positions("fcc", a, 4, 4, 4)
        p = mp.System(pos=pos, box=box)
        p.set_element(np.array(["Ni"] * len(pos), dtype=object))
        p.calc = mp.EAM(NICKEL)
        energy.append(p.get_energy())
    c2, c1, _ = np.polyfit(grid - 3.507, energy, 2)
    a0 = 3.507 - c1 / (2 * c2)
    inner = np.polyfit(grid[1:4] - 3.507, energy[1:4], 2)
    fit_error = abs(a0 - (3.507 - inner[1] / (2 * inner[0])))  # (the parabola's own error: what the cubic term moves its minimum by)
    # E = c2 (a - a0)^2 and V = 64 a^3: p = -dE/dV = -2 c2 (a - a0) / (192 a^2); |p| below the stress bound allows this much strain
    allowed = (fmax * n / volume) * 192.0 * got**2 / (2.0 * c2)
    print(f"a = {got:.6f}, parabola minimum {a0:.6f} (fit error {fit_error:.2e}), the stress bound allows {allowed:.2e}")
    assert abs(got - a0) <= fit_error + allowed


# ---------------------------------------------------------------------------------------------- 5. the paths
def test_thin_box_runs_on_the_replica():
    path, pos, box, names = _eam_ref.fixture_case(1)
    s, t = _pair(path, pos, box, names)
    fire = mp.FIRE(s)
    fire.run(10, fmax=0, show_process=False)
    _same_state(fire, s, _exact(t, 10), t)
    s.get_force()
    assert "_enlarge_data" in s.__dict__


def test_shuffled_frame_runs_on_the_twin(monkeypatch):
    monkeypatch.setenv("MDAPY_SPATIAL_SORT", "1")
    pos, box, names = _alloy(False)
    order = np.random.default_rng(5).permutation(len(pos))
    s = _pair(NICKEL, pos[order], box, names[order])[0]
    fire = mp.FIRE(s)
    fire.run(10, fmax=0, show_process=False)
    s.get_force()
    assert s._listed_on_twin() is not None
    monkeypatch.setenv("MDAPY_SPATIAL_SORT", "0")
    plain = _pair(NICKEL, pos[order], box, names[order])[0]
    _same_state(fire, s, _exact(plain, 10), plain)


# The host path adds with np.vdot and multiplies with matmul, the HBM path in the fixed order.  Measured on the CPU between
# ``_fire_ref.run`` with np.vdot / matmul and with the tree / the stated row order, under the numpy Lennard-Jones calculator of
# test_fire_host.py (108 atoms, 25 steps; FIRE2, ABC and optimize_cell; rattle 0.02 and 0.08, dt 0.1 and 0.02): the positions
# differ by at most 6.2e-15 at coordinates up to 4.7, i.e. 1.4e-15 of the largest coordinate — rounding is relative, so the
# tolerance is stated that way.  Tenfold margin.
HOST_GAP_RELATIVE = 1.4e-15


def test_host_path_agrees_with_the_hbm_path():
    s, t = _pair(NICKEL, *_alloy(False))
    a, b = mp.FIRE(s), mp.FIRE(t, device=False)
    a.run(25, fmax=0, show_process=False)
    b.run(25, fmax=0, show_process=False)
    assert a._hbm and not b._hbm
    gap = np.abs(_positions(s) - _positions(t)).max()
    print(f"positions of the two paths after 25 steps differ by {gap:.3e}")
    assert (a.dt, a.a, a.Nsteps) == (b.dt, b.a, b.Nsteps) and gap <= 10 * HOST_GAP_RELATIVE * np.abs(_positions(s)).max()


def test_nothing_of_n_elements_crosses_to_the_host_during_a_run(monkeypatch):
    from mdapy_amd import devarray

    s = _pair(NICKEL, *_alloy(False))[0]
    n, seen, armed = s.N, [], []
    numpy_of, as_numpy, update = devarray.HArray.numpy, devarray.as_numpy, mp.System.update_data

    def counted_numpy(self):
        if armed and self.size >= n:
            seen.append(("HArray.numpy", self.shape))
        return numpy_of(self)

    def counted_as_numpy(a):
        if armed and hasattr(a, "_host_arr") and a._host_arr is None and len(a) >= n:  # (a column that lives in HBM only)
            seen.append(("as_numpy", a.name))
        return as_numpy(a)

    def armed_update(self, *args, **kwargs):
        update(self, *args, **kwargs)
        armed.append(True)  # (the end of the first step: its move)

    monkeypatch.setattr(devarray.HArray, "numpy", counted_numpy)
    monkeypatch.setattr(devarray, "as_numpy", counted_as_numpy)
    for module in ("eam", "system", "neighbor", "_twin", "policy"):
        owner = getattr(__import__("mdapy_amd." + module), module)
        if hasattr(owner, "as_numpy"):
            monkeypatch.setattr(owner, "as_numpy", counted_as_numpy)
    monkeypatch.setattr(mp.System, "update_data", armed_update)
    assert mp.FIRE(s).run(10, fmax=0) is False
    armed.clear()
    assert seen == []
