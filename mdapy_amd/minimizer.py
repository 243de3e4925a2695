"""``FIRE`` — the drop-in for ``mdapy.minimizer.FIRE`` (src/mdapy/minimizer.py:39-375): the FIRE2 minimizer (Guenole et al.,
Comput. Mater. Sci. 175 (2020) 109584), optionally ABC-FIRE (Echeverri Restrepo and Andric, Comput. Mater. Sci. 218 (2023) 111978),
optionally relaxing the cell with the atoms the way ASE's ``UnitCellFilter`` does: the deformation gradient is three more rows
below the atoms' (Tadmor et al., Phys. Rev. B 59 (1999) 235).

    system.calc = EAM("Ni.eam.alloy")
    FIRE(system, optimize_cell=True).run(steps=1000, fmax=1e-4)

Constructor, ``run``, ``get_forces``, ``update_data_box``, the attributes ``dt a Nsteps v ndof orig_box cell_factor mask`` and the
printed table are the reference's.  One control flow (``run``) drives one of two paths:

* **the host path** is the reference's algorithm in numpy on what ``System.get_force()`` / ``get_stress()`` return: any
  ``CalculatorMP`` will do.
* **the HBM path**  needs a calculator with the array-level door ``_calculate_device`` (``EAM``): positions,
  velocities, forces and the displacement stay in HBM for the whole run, csrc/fire.hip does the arithmetic on them, and the host
  reads a record of a few scalars per step — v . f and max |f_i|^2 to branch and to test convergence, with ``optimize_cell`` also
  the nine virial sums and the cell's three displacement rows.  The 3 x 3 algebra of the cell stays on the host, in the
  reference's expressions.  Sums run in a fixed order (include/mdapy_amd.h "_fire"), the host path's in ``np.vdot``'s: the two
  paths agree to rounding, not to the bit.  With ``optimize_cell`` the HBM path keeps the UNSTRAINED positions as its state
  (``u += dr``, positions = u (I + deform)) where the reference solves them back from the strained ones every step.

``device`` (keyword only, not in the reference): None — the HBM path when the calculator has the door and a GPU is there;
False — the host path; True — the HBM path, an error when the calculator has no door."""
import numpy as np

from . import kernels
from .devarray import HArray, empty, have_gpu, zeros


def _voigt_to_matrix(voigt):
    """[xx, yy, zz, yz, xz, xy] -> the symmetric 3 x 3"""
    xx, yy, zz, yz, xz, xy = voigt
    return np.array([[xx, xy, xz], [xy, yy, yz], [xz, yz, zz]])


def _small(a, start=0, stop=None):
    """rows start .. stop of an array that lives in HBM or on the host, as a host array — for a record, three rows: never N"""
    if isinstance(a, HArray):
        return a.dev()[start:stop].cpu().numpy()
    return np.array(a[start:stop])


def _view(a, start, stop):
    """rows start .. stop of an array, where it lives, sharing its memory"""
    return HArray(a.dev()[start:stop]) if isinstance(a, HArray) else a[start:stop]


def _put(a, start, values):
    """values into the rows from ``start`` on (the three cell rows: 72 bytes up)"""
    if isinstance(a, HArray):
        from .devarray import torch

        a.dev()[start:start + len(values)].copy_(torch().from_numpy(np.ascontiguousarray(values)))
        a.invalidate_host()
    else:
        a[start:start + len(values)] = values


def _column(col):
    """a frame column where the kernels read it"""
    return col.device_array() if have_gpu() else col.to_numpy()


class FIRE:
    def __init__(self, system, dt=0.1, maxstep=0.2, dtmax=1.0, dtmin=2e-3, Nmin=20, finc=1.1, fdec=0.5, astart=0.25, fa=0.99,
                 use_abc=False, optimize_cell=False, mask=None, cell_factor=None, hydrostatic_strain=False, constant_volume=False,
                 scalar_pressure=0.0, *, device=None):
        self.system = system
        self.dt, self.maxstep, self.dtmax, self.dtmin = dt, maxstep, dtmax, dtmin
        self.Nmin, self.finc, self.fdec = Nmin, finc, fdec
        self.astart, self.fa = astart, fa
        self.a = astart
        self.Nsteps = 0
        self.use_abc, self.optimize_cell = use_abc, optimize_cell
        self.scalar_pressure, self.hydrostatic_strain, self.constant_volume = scalar_pressure, hydrostatic_strain, constant_volume
        self.device = device
        self.N = system.N
        self.ndof = self.N + 3 if optimize_cell else self.N
        self.orig_box = self.cell_factor = self.mask = None
        if optimize_cell:
            self.orig_box = system.box.box.copy()
            self.cell_factor = float(self.N) if cell_factor is None else cell_factor
            if mask is None:
                mask = np.ones((3, 3))
            elif len(mask) == 6:  # (read in Voigt order, like a stress)
                mask = _voigt_to_matrix(mask)
            self.mask = np.asarray(mask)

    # ------------------------------------------------------------------ the cell's 3 x 3 algebra: host, both paths
    def _deform_grad(self):
        return np.linalg.solve(self.orig_box, self.system.box.box).T

    def _cell_forces(self, stress, grad):
        """the three cell rows of the extended force from the Voigt stress and the current deformation gradient"""
        volume = self.system.box.volume
        virial = (-_voigt_to_matrix(stress) - np.diag([self.scalar_pressure] * 3)) * volume
        virial = np.linalg.solve(grad, virial.T).T
        if self.hydrostatic_strain:
            third = virial.trace() / 3.0
            virial = np.diag([third] * 3)
        if (self.mask != 1.0).any():
            virial *= self.mask
        if self.constant_volume:
            trace = virial.trace()
            np.fill_diagonal(virial, np.diag(virial) - trace / 3.0)
        return virial / self.cell_factor

    def _new_cell(self, grad, dr_cell):
        """(I + deform, the new box) after the cell rows moved by ``dr_cell``"""
        new_grad = grad + (dr_cell / self.cell_factor)
        deform = (new_grad - np.eye(3)).T * self.mask
        strain = np.eye(3) + deform
        return strain, self.orig_box @ strain

    # ------------------------------------------------------------------ the host path: the reference's two methods
    def get_forces(self):
        """(N, 3) forces; with ``optimize_cell`` (N + 3, 3): the atoms' forces times the deformation gradient, then the cell's rows"""
        forces = self.system.get_force()
        if not self.optimize_cell:
            return forces
        grad = self._deform_grad()
        cell = self._cell_forces(self.system.get_stress(), grad)
        return np.vstack((forces @ grad, cell))

    def update_data_box(self, dr):
        """move the atoms — and with ``optimize_cell`` the cell, by the last three rows — by ``dr``; the calculator's results and the
        neighbour list are forgotten"""
        system = self.system
        frame = system.data
        if not self.optimize_cell:
            moved = {name: frame[name].to_numpy() + dr[:, k] for k, name in enumerate("xyz")}
        else:
            positions = frame.select("x", "y", "z").to_numpy()
            grad = self._deform_grad()
            unstrained = np.linalg.solve(grad, positions.T).T + dr[:self.N]
            strain, box = self._new_cell(grad, dr[self.N:])
            system.update_box(box)
            positions = unstrained @ strain
            moved = {name: positions[:, k] for k, name in enumerate("xyz")}
        system.update_data(frame.with_columns(**moved), True, True)

    # ------------------------------------------------------------------ the HBM path
    def _on_device(self):
        calc = self.system.calc
        door = hasattr(calc, "_calculate_device")
        if self.device is None:
            return door and have_gpu()
        if self.device and not door:
            raise RuntimeError(f"FIRE(device=True): {type(calc).__name__} has no array-level door (_calculate_device); use device=False.")
        return bool(self.device)

    def _device_start(self):
        """the run's state, made before the first force evaluation"""
        self._record = zeros(kernels.fire.RECORD, np.float64)
        self._dr = zeros((self.ndof, 3), np.float64)
        self._raw = None
        if self.optimize_cell:
            self._force = zeros((self.ndof, 3), np.float64)
            positions = self.system.data.select("x", "y", "z").to_numpy()
            unstrained = np.ascontiguousarray(np.linalg.solve(self._deform_grad(), positions.T).T)
            self._unstrained = HArray.from_numpy(unstrained) if have_gpu() else unstrained

    def _device_forces(self):
        """the extended forces of the current frame into ``self._force``, through the calculator's array-level door"""
        system, fire = self.system, kernels.fire
        sums = _view(self._record, fire.VIRIAL, fire.VIRIAL + 9)
        force, _, self._raw = system.calc._calculate_device(system, sums)
        if not self.optimize_cell:
            self._force = force
            return
        stress = system.calc._stress_of_sums(_small(self._record, fire.VIRIAL, fire.VIRIAL + 9), system.box.volume)
        grad = self._deform_grad()
        fire.rowmat(force, grad, out_rows=_view(self._force, 0, self.N))
        _put(self._force, self.N, self._cell_forces(stress, grad))

    def _device_move(self, scale, mode):
        system, fire, n = self.system, kernels.fire, self.N
        frame = system.data
        new = [empty(n, np.float64) for _ in range(3)]
        if not self.optimize_cell:
            fire.move(self.v, self._dr, n, scale, self.dt, self.maxstep, mode, self._record, *(_column(frame[c]) for c in "xyz"), *new)
        else:
            fire.move(self.v, self._dr, n, scale, self.dt, self.maxstep, mode, self._record, unstrained=self._unstrained)
            strain, box = self._new_cell(self._deform_grad(), _small(self._dr, n, n + 3))
            system.update_box(box)
            fire.rowmat(self._unstrained, strain, out_x=new[0], out_y=new[1], out_z=new[2])
        system.update_data(frame.with_columns(x=new[0], y=new[1], z=new[2]), True, True)

    # ------------------------------------------------------------------ the steps, per path
    def _evaluate(self):
        if self._hbm:
            self._device_forces()
        else:
            self._force = self.get_forces()

    def _measure(self, show):
        """(v . f or None before the first kick, max |f_i|^2, (energy, pressure) for the table or None)"""
        moving = self.v is not None
        if not self._hbm:
            f = self._force
            shown = None
            if show:
                stress = self.system.get_stress()
                shown = (self.system.get_energy(), -stress[:3].mean())
            return (np.vdot(f, self.v) if moving else None), (f**2).sum(axis=1).max(), shown
        fire = kernels.fire
        if show:
            energy, real = self._raw[0], self._raw[5]
            fire.total(energy if int(energy.shape[0]) == real else _view(energy, 0, real), fire.ENERGY, self._record)
        fire.dots(self.v if moving else None, self._force, self._record)
        record = _small(self._record)  # the step's one read of the record (with optimize_cell the virial sums were read before)
        shown = None
        if show:
            stress = self.system.calc._stress_of_sums(record[fire.VIRIAL:fire.VIRIAL + 9], self.system.box.volume)
            shown = (record[fire.ENERGY], -stress[:3].mean())
        return (record[fire.VF] if moving else None), record[fire.FMAX2], shown

    def _move(self, scale, uphill):
        if self._hbm:
            fire = kernels.fire
            self._device_move(scale, fire.MOVE_PLAIN if uphill else (fire.MOVE_CAP if self.use_abc else fire.MOVE_NORM))
            return
        if uphill or self.use_abc:
            if self.use_abc and not uphill and np.all(self.v):  # ABC-FIRE: a cap per component, and only when no component is zero
                size = np.abs(self.v)
                with np.errstate(invalid="ignore", divide="ignore"):
                    self.v = np.where(size * self.dt > self.maxstep, (self.maxstep / self.dt) * (self.v / size), self.v)
            dr = scale * self.v
        else:
            dr = scale * self.v
            norm = np.sqrt(np.vdot(dr, dr))
            if norm > self.maxstep:
                dr = self.maxstep * dr / norm
        self.update_data_box(dr)

    def _kick(self, zero_first):
        if self._hbm:
            kernels.fire.kick(self.v, self._force, self.dt, zero_first, self._record)
            return
        if zero_first:
            self.v *= 0.0
        self.v += self.dt * self._force

    def _mix(self, multiplier):
        if self._hbm:
            kernels.fire.mix(self.v, self._force, self.a, multiplier, self.use_abc, self.dt, self._record)
            return
        f = self._force
        mixed = (1.0 - self.a) * self.v + self.a * f / np.sqrt(np.vdot(f, f)) * np.sqrt(np.vdot(self.v, self.v))
        self.v = multiplier * mixed if self.use_abc else mixed

    # ------------------------------------------------------------------ the one control flow
    def run(self, steps, fmax=1e-4, show_process=True):
        """at most ``steps`` steps; True as soon as the largest force (cell rows included) is below ``fmax``.  ``dt``, ``a`` and
        ``Nsteps`` carry on from an earlier run, the velocities start from nothing."""
        system = self.system
        assert system.calc is not None, "Must assign a calc first."
        self.v = None
        self._hbm = self._on_device()
        if self._hbm:
            self._device_start()
        if show_process:
            print(f"{'Step':>6} {'Energy':>15} {'fmax':>15} {'pressure':>15}")
        for step in range(steps):
            self._evaluate()
            vf, largest, shown = self._measure(show_process)
            cfmax = np.sqrt(largest)
            if show_process:
                energy, press = shown
                if self.optimize_cell:
                    energy = energy + self.scalar_pressure * system.box.volume
                print(f"{step:6d} {energy:15.6f} {cfmax:15.6f} {press:15.6f}")
            if cfmax < fmax:
                if self._hbm:  # what the kernels left is the final frame's: the calculator answers for it without running again
                    system.calc._to_results(system, *self._raw)
                if show_process:
                    print("Converged!")
                return True
            reset = False
            if self.v is None:
                self.v = zeros((self.ndof, 3), np.float64) if self._hbm else np.zeros((self.ndof, 3))
            elif vf > 0.0:
                self.Nsteps += 1
                if self.Nsteps > self.Nmin:
                    self.dt = min(self.dt * self.finc, self.dtmax)
                    self.a *= self.fa
            else:  # uphill: half a step back, and start again from rest
                self.Nsteps = 0
                self.dt = max(self.dt * self.fdec, self.dtmin)
                self.a = self.astart
                self._move(-0.5 * self.dt, True)
                self._evaluate()
                reset = True
            self._kick(reset)
            multiplier = 1.0
            if self.use_abc:
                self.a = max(self.a, 1e-10)
                multiplier = 1.0 / (1.0 - (1.0 - self.a) ** (self.Nsteps + 1))
            self._mix(multiplier)
            self._move(self.dt, False)
        system.calc.results = {}
        if show_process:
            print("Not converged! Try decrease the fmax or increase steps.")
        return False
