"""The FIRE minimizer on the CPU.

1. the host path (``device=False``) against the restatement of tests/_fire_ref.py with ``np.vdot``, under a numpy Lennard-Jones
   calculator defined here: the same floating-point operations in the same order, so ``array_equal``;
2. the HBM path's driver (``device=True``) with ``kernels.fire`` set to the restatement, ``kernels.eam`` to tests/_eam_ref.py and
   the neighbour build routed to the oracle, against ``_fire_ref.run`` with the fixed-order sums on a second System;
3. the public surface."""
import os
import re

import numpy as np
import pytest

import _eam_ref
import _fire_ref
import mdapy_amd as mp
from mdapy_amd.build_lattice import lattice_positions
from mdapy_amd.calculator import CalculatorMP

EPS = np.finfo(np.float64).eps
# the reference's own table of modes (its tests/test_minimize.py): use_abc, optimize_cell, mask, hydrostatic_strain, constant_volume, scalar_pressure
MODES = [(False, False, None, False, False, 0), (True, False, None, False, False, 0), (False, True, None, False, False, 0),
         (True, True, None, False, False, 0), (False, True, [1, 0, 0, 0, 0, 0], False, False, 0), (False, True, None, True, False, 0),
         (False, True, None, False, True, 0), (False, True, None, False, False, 1)]


def _kwargs(mode):
    use_abc, optimize_cell, mask, hydro, const_v, p = mode
    return dict(use_abc=use_abc, optimize_cell=optimize_cell, mask=mask, hydrostatic_strain=hydro, constant_volume=const_v, scalar_pressure=p)


class LennardJones(CalculatorMP):
    """all pairs, nearest image (through fractional coordinates: any cell), epsilon = sigma = 1, cut and shifted at ``rc``; the sign
    conventions of the EAM: force_i += p d, virial_i -= 0.5 d (p d)^T with d = r_j - r_i, stress = -(V + V^T) / (2 volume)"""

    def __init__(self, rc=2.2):
        self.rc, self.results, self.evaluations = rc, {}, 0

    def _calculate(self, data, box):
        self.evaluations += 1
        pos = np.column_stack([data[c].to_numpy() for c in "xyz"])
        cell = box.box
        d = pos[None, :, :] - pos[:, None, :]
        frac = d @ np.linalg.inv(cell)
        d = (frac - np.round(frac)) @ cell
        r = np.sqrt((d**2).sum(axis=2))
        np.fill_diagonal(r, np.inf)
        inside = r <= self.rc
        with np.errstate(divide="ignore"):
            s6 = np.where(inside, r**-6.0, 0.0)
            rinv = np.where(inside, 1.0 / r, 0.0)
        shift = 4.0 * (self.rc**-12.0 - self.rc**-6.0)
        pair = np.where(inside, 4.0 * (s6 * s6 - s6) - shift, 0.0)
        p = (4.0 * (-12.0 * s6 * s6 + 6.0 * s6) * rinv) * rinv  # (dE/dr) / r
        fp = p[:, :, None] * d
        self.results["energies"] = 0.5 * pair.sum(axis=1)
        self.results["forces"] = fp.sum(axis=1)
        virials = -0.5 * (d[:, :, :, None] * fp[:, :, None, :]).sum(axis=1)
        self.results["virials"] = virials.reshape(len(pos), 9)
        v = virials.sum(axis=0)
        self.results["stress"] = (-0.5 * (v + v.T) / box.volume).ravel()[[0, 4, 8, 5, 2, 1]]

    def _get(self, name, data, box):
        if name not in self.results:
            self._calculate(data, box)
        return self.results[name]

    def get_energies(self, data, box):
        return self._get("energies", data, box)

    def get_energy(self, data, box):
        return self._get("energies", data, box).sum()

    def get_forces(self, data, box):
        return self._get("forces", data, box)

    def get_stress(self, data, box):
        return self._get("stress", data, box)

    def get_virials(self, data, box):
        return self._get("virials", data, box)


def lj_system(cells=3, a=1.58, rattle=0.08, seed=3):
    """an fcc Lennard-Jones crystal (108 atoms), slightly expanded and rattled: forces on every atom and a stress on the cell"""
    pos, box = lattice_positions("fcc", a, cells, cells, cells)
    s = mp.System(pos=pos + np.random.default_rng(seed).normal(0, rattle, pos.shape), box=box)
    s.calc = LennardJones()
    return s


def _positions(system):
    return np.column_stack([system.data[c].to_numpy() for c in "xyz"])


def _same_state(fire, system, ref, other):
    assert np.array_equal(_positions(system), _positions(other))
    assert np.array_equal(system.box.box, other.box.box)
    assert np.array_equal(np.asarray(fire.v), ref["v"])
    assert (fire.dt, fire.a, fire.Nsteps) == (ref["dt"], ref["a"], ref["Nsteps"])


# ---------------------------------------------------------------------------------------------- 1. the host path
@pytest.mark.parametrize("mode", range(len(MODES)))
def test_host_path_is_the_restatement_bit_for_bit(mode):
    kwargs = _kwargs(MODES[mode])
    s, t = lj_system(), lj_system()
    fire = mp.FIRE(s, device=False, **kwargs)
    assert fire.run(5, fmax=0.0, show_process=False) is False
    ref = _fire_ref.run(t, 5, fmax=0.0, **kwargs)
    _same_state(fire, s, ref, t)
    assert fire.ndof == 108 + 3 * kwargs["optimize_cell"] and np.asarray(fire.v).shape == (fire.ndof, 3)
    assert not np.array_equal(_positions(s), _positions(lj_system()))  # (it moved)


@pytest.mark.parametrize("mode", [0, 1, 2])
def test_host_path_through_the_uphill_and_the_speed_up_branches(mode):
    """long enough to go uphill and to pass Nmin good steps in a row (Nmin = 5 here, so that 60 steps show both)"""
    kwargs = dict(_kwargs(MODES[mode]), Nmin=5, dt=0.02, dtmax=0.2)
    s, t = lj_system(), lj_system()
    fire = mp.FIRE(s, device=False, **kwargs)
    fire.run(60, fmax=0.0, show_process=False)
    ref = _fire_ref.run(t, 60, fmax=0.0, **kwargs)
    print(f"mode {mode}: uphill at {ref['uphill']}, faster at {len(ref['faster'])} steps, dt {ref['dt']}, a {ref['a']}, Nsteps {ref['Nsteps']}")
    assert len(ref["uphill"]) >= 1 and len(ref["faster"]) >= 1 and ref["dt"] != kwargs["dt"]
    _same_state(fire, s, ref, t)
    assert s.calc.evaluations == t.calc.evaluations == 60 + len(ref["uphill"])


# What keeping the unstrained positions as the state (the HBM path) changes against solving them back from the
# strained ones in every move (the reference), measured here between the two numpy versions over 10 steps of the Lennard-Jones
# crystal with optimize_cell: 3.6e-15 in the positions (coordinates up to 4.7: a few eps |x|, the solve's own rounding), 8.1e-19
# in the box and 8.7e-13 in v (|v| up to 240 in the first steps of this stiff crystal).  Tenfold margins.  (The gap is rounding fed
# through the dynamics, so it grows with the number of steps: the comparison is made over 10.)
UNSTRAINED_TOLERANCE = dict(positions=3.6e-14, box=8.2e-18, v=8.7e-12)


def test_keeping_unstrained_positions_is_the_same_mathematics():
    kwargs = _kwargs(MODES[2])
    s, t = lj_system(), lj_system()
    kept = _fire_ref.run(s, 10, fmax=0.0, keep_unstrained=True, **kwargs)
    solved = _fire_ref.run(t, 10, fmax=0.0, **kwargs)
    gaps = dict(positions=np.abs(_positions(s) - _positions(t)).max(), box=np.abs(s.box.box - t.box.box).max(),
                v=np.abs(kept["v"] - solved["v"]).max())
    print("keep-unstrained against solve-back after 10 steps:", gaps)
    for name, gap in gaps.items():
        assert gap <= UNSTRAINED_TOLERANCE[name], name
    assert (kept["dt"], kept["a"], kept["Nsteps"]) == (solved["dt"], solved["a"], solved["Nsteps"])


# ---------------------------------------------------------------------------------------------- 2. the HBM path's driver
@pytest.fixture
def restated(oracle_backend, monkeypatch):
    import mdapy_amd.kernels as K

    monkeypatch.setattr(K, "eam", _eam_ref)
    monkeypatch.setattr(K, "fire", _fire_ref)
    return K


def _exact(system, steps, **kwargs):
    return _fire_ref.run(system, steps, fmax=0.0, dot=_fire_ref.tree_dot, matmul=_fire_ref.row_times_matrix, keep_unstrained=True, **kwargs)


def _nickel(a=3.52, rattle=0.05):
    pos, box = lattice_positions("fcc", a, 4, 4, 4)
    pos = pos + np.random.default_rng(0).normal(0, rattle, pos.shape)
    return pos, box, np.array(["Ni"] * len(pos), dtype=object)


def _eam_pair(path, pos, box, names):
    out = []
    for _ in range(2):
        s = mp.System(pos=pos, box=box)
        s.set_element(names)
        s.calc = mp.EAM(path)
        out.append(s)
    return out


NICKEL = os.path.join(_eam_ref.GOLDEN, "NiCoCr.lammps.eam.gz")


@pytest.mark.parametrize("kwargs", [dict(), dict(use_abc=True, optimize_cell=True)], ids=["fire2", "abc-cell"])
def test_device_driver_on_the_crystal(restated, kwargs):
    s, t = _eam_pair(NICKEL, *_nickel())
    fire = mp.FIRE(s, device=True, **kwargs)
    assert fire.run(3, fmax=0.0, show_process=False) is False and fire._hbm
    _same_state(fire, s, _exact(t, 3, **kwargs), t)
    assert s.calc.results == {}


def test_device_driver_on_the_replica_of_a_thin_box(restated):
    path, pos, box, names = _eam_ref.fixture_case(1)
    s, t = _eam_pair(path, pos, box, names)
    fire = mp.FIRE(s, device=True)
    fire.run(3, fmax=0.0, show_process=False)
    assert "_enlarge_data" not in s.__dict__  # (the list is forgotten after the last move; it was a replica's)
    s.get_force()
    assert "_enlarge_data" in s.__dict__
    _same_state(fire, s, _exact(t, 3), t)


def test_device_driver_on_the_twin_of_a_shuffled_frame(restated, monkeypatch):
    monkeypatch.setenv("MDAPY_SPATIAL_SORT", "1")
    pos, box = lattice_positions("fcc", 3.52, 5, 5, 5)  # (17.6 A: wide enough for a twin)
    pos = pos + np.random.default_rng(0).normal(0, 0.05, pos.shape)
    names = np.array(["Ni"] * len(pos), dtype=object)
    s, t = _eam_pair(NICKEL, pos[order := np.random.default_rng(5).permutation(len(pos))], box, names)
    fire = mp.FIRE(s, device=True)
    fire.run(3, fmax=0.0, show_process=False)
    s.get_force()
    assert s._listed_on_twin() is not None
    monkeypatch.setenv("MDAPY_SPATIAL_SORT", "0")
    plain = _eam_pair(NICKEL, pos[order], box, names)[0]  # (the yardstick runs without a twin: the results do not depend on one)
    _same_state(fire, s, _exact(plain, 3), plain)


def test_converged_device_run_leaves_results_for_the_final_frame(restated):
    pos, box, names = _nickel(rattle=0.0)
    s, t = _eam_pair(NICKEL, pos, box, names)
    assert mp.FIRE(s, device=True).run(3, fmax=1e-3, show_process=False) is True  # (a perfect crystal: converged at step 0)
    assert set(s.calc.results) == {"energies", "forces", "virials", "stress"}
    for name in s.calc.results:
        assert np.array_equal(s.calc.results[name], getattr(t, {"energies": "get_energies", "forces": "get_force", "virials": "get_virials",
                                                                "stress": "get_stress"}[name])()), name


# ---------------------------------------------------------------------------------------------- 3. the surface
def test_exported():
    assert mp.FIRE is mp.minimizer.FIRE and "FIRE" in mp.__all__


def test_needs_a_calculator():
    pos, box = lattice_positions("fcc", 1.58, 2, 2, 2)
    with pytest.raises(AssertionError, match="Must assign a calc first."):
        mp.FIRE(mp.System(pos=pos, box=box), device=False).run(1, show_process=False)


def test_device_true_needs_the_array_door():
    with pytest.raises(RuntimeError, match="door"):
        mp.FIRE(lj_system(), device=True).run(1, show_process=False)
    assert mp.FIRE(lj_system()).run(1, fmax=0.0, show_process=False) is False  # (device=None: no door, the host path)


def test_attributes_and_the_voigt_mask():
    s = lj_system()
    plain = mp.FIRE(s)
    assert (plain.dt, plain.a, plain.Nsteps, plain.ndof, plain.orig_box, plain.cell_factor, plain.mask) == (0.1, 0.25, 0, 108, None, None, None)
    cell = mp.FIRE(s, optimize_cell=True, mask=[1, 2, 3, 4, 5, 6])
    assert cell.ndof == 111 and cell.cell_factor == 108.0 and np.array_equal(cell.orig_box, s.box.box)
    assert np.array_equal(cell.mask, [[1, 6, 5], [6, 2, 4], [5, 4, 3]])
    assert np.array_equal(mp.FIRE(s, optimize_cell=True).mask, np.ones((3, 3))) and mp.FIRE(s, optimize_cell=True, cell_factor=7).cell_factor == 7
    forces = cell.get_forces()
    assert forces.shape == (111, 3) and np.array_equal(forces[:108] @ np.eye(3), s.get_force() @ np.linalg.solve(cell.orig_box, s.box.box).T)
    before = _positions(s)
    mp.FIRE(s).update_data_box(np.full((108, 3), 0.25))
    assert np.array_equal(_positions(s), before + 0.25) and s.calc.results == {}


def test_printed_table(capsys):
    s = lj_system()
    energy, stress, largest = s.get_energy(), s.get_stress(), np.sqrt((s.get_force()**2).sum(axis=1).max())
    assert mp.FIRE(s, device=False).run(3, fmax=0.0) is False
    lines = capsys.readouterr().out.splitlines()
    assert lines[0] == f"{'Step':>6} {'Energy':>15} {'fmax':>15} {'pressure':>15}"
    assert lines[1] == f"{0:6d} {energy:15.6f} {largest:15.6f} {-stress[:3].mean():15.6f}"
    for k in (1, 2, 3):
        assert re.fullmatch(rf" {{5}}{k - 1} [ \-\d.]{{15}} [ \-\d.]{{15}} [ \-\d.]{{15}}", lines[k]), lines[k]
    assert lines[4] == "Not converged! Try decrease the fmax or increase steps." and len(lines) == 5
    s = lj_system()
    assert mp.FIRE(s, device=False).run(3, fmax=1e9) is True
    lines = capsys.readouterr().out.splitlines()
    assert len(lines) == 3 and lines[2] == "Converged!"
    # with optimize_cell the table shows the enthalpy: energy + scalar_pressure * volume
    s = lj_system()
    mp.FIRE(s, device=False, optimize_cell=True, scalar_pressure=0.5).run(1, fmax=1e9)
    shown = float(capsys.readouterr().out.splitlines()[1].split()[1])
    assert abs(shown - (energy + 0.5 * s.box.volume)) < 1e-6


def test_results_after_a_run():
    s = lj_system()
    assert mp.FIRE(s, device=False).run(2, fmax=0.0, show_process=False) is False and s.calc.results == {}
    assert mp.FIRE(s, device=False).run(2, fmax=1e9, show_process=False) is True
    assert "forces" in s.calc.results and np.array_equal(s.calc.results["forces"], lj_like(s).get_force())


def lj_like(system):
    fresh = mp.System(pos=_positions(system), box=system.box)
    fresh.calc = LennardJones()
    return fresh


def test_a_second_run_carries_dt_a_and_nsteps_on():
    kwargs = dict(Nmin=2, dt=0.02)
    s, t = lj_system(rattle=0.02), lj_system(rattle=0.02)
    fire = mp.FIRE(s, device=False, **kwargs)
    fire.run(8, fmax=0.0, show_process=False)
    first = (fire.dt, fire.a, fire.Nsteps)
    assert first != (0.02, 0.25, 0)
    fire.run(4, fmax=0.0, show_process=False)
    ref = _fire_ref.run(t, 8, fmax=0.0, **kwargs)
    assert (ref["dt"], ref["a"], ref["Nsteps"]) == first
    ref = _fire_ref.run(t, 4, fmax=0.0, state=ref, **kwargs)  # (v starts from nothing, the three scalars carry on)
    _same_state(fire, s, ref, t)


def test_eam_results_are_what_they_were(restated):
    """the split of ``EAM._calculate_on`` changed nothing: through the System, and on (data, box) of nobody's System"""
    path, pos, box, names = _eam_ref.fixture_case(1)
    s, t = _eam_pair(path, pos, box, names)
    s.get_force()  # (builds the list the yardstick runs on)
    want = _eam_ref.on_system_list(s, s.calc)
    assert np.array_equal(s.get_energies(), want[0]) and np.array_equal(s.get_force(), want[1]) and np.array_equal(s.get_virials(), want[2])
    assert np.array_equal(s.get_stress(), _eam_ref.stress_of(_eam_ref.exact_column_sums(want[2]), s.box.volume))
    loose = mp.EAM(path)
    assert np.array_equal(loose.get_forces(t.data, t.box), want[1]) and loose.get_energy(t.data, t.box) == want[0].sum()
    force, sums, raw = t.calc._calculate_device(t)
    assert np.array_equal(np.asarray(force), want[1]) and np.asarray(force).shape == (len(pos), 3) and t.calc.results == {}
    t.calc._to_results(t, *raw)
    assert np.array_equal(t.calc.results["virials"], want[2]) and np.array_equal(t.calc.results["stress"], s.get_stress())
