"""Drop-in for ``mdapy._eam`` (src/eam.cpp:187-217): class ``EAM(rc, dr, drho, F_rho, rho_r, rphi_r)`` whose ``calculate`` has the
reference's name and argument order and ADDS into ``force``, ``virial`` and ``energy`` as the reference does.

The spline coefficients are computed here, on the host, once per object, with exactly the arithmetic of the reference's
``UniformCubicSpline`` constructor (src/spline.h:399-449) — they carry the same bits — as one 32-byte knot (a, b, c, d) per grid
point; the kernels only look them up.  The tables go to HBM at the object's first call with device arrays and stay there.

Extensions (keywords after ``num_t``): ``accumulate=False`` writes the results instead of adding them (the arrays need not be
initialised), ``virial_sum`` (9 f64) receives the column sums of the first ``n_real`` rows of ``virial``, added on the device in
a fixed order."""
import numpy as np

from . import _lib
from .devarray import Call, HArray

f64, i32 = np.float64, np.int32


def spline_knots(h, y):
    """(..., n) tabulated values at spacing h -> (..., n, 4) knots (a, b, c, d) of src/spline.h:399-449, operation for operation"""
    y = np.asarray(y, dtype=f64)
    n = y.shape[-1]
    if not h > 0.0:
        raise ValueError("h must be positive")
    if n < 2:
        raise ValueError("Need at least 2 points for interpolation")
    fp = np.zeros_like(y)
    fp[..., 0] = y[..., 1] - y[..., 0]
    fp[..., n - 1] = y[..., n - 1] - y[..., n - 2]
    if n >= 3:
        fp[..., 1] = 0.5 * (y[..., 2] - y[..., 0])
        fp[..., n - 2] = 0.5 * (y[..., n - 1] - y[..., n - 3])
    if n >= 5:
        fp[..., 2:n - 2] = ((y[..., 0:n - 4] - y[..., 4:n]) + 8.0 * (y[..., 3:n - 1] - y[..., 1:n - 3])) / 12.0
    inv_h = 1.0 / float(h)
    inv_h2 = inv_h * inv_h
    inv_h3 = inv_h2 * inv_h
    knots = np.zeros(y.shape + (4,), f64)
    dy = y[..., 1:] - y[..., :-1]
    knots[..., :-1, 0] = y[..., :-1]
    knots[..., :-1, 1] = fp[..., :-1] * inv_h
    knots[..., :-1, 2] = (3.0 * dy - 2.0 * fp[..., :-1] - fp[..., 1:]) * inv_h2
    knots[..., :-1, 3] = (fp[..., :-1] + fp[..., 1:] - 2.0 * dy) * inv_h3
    knots[..., n - 1, 0] = y[..., n - 1]  # the last slot: a straight line past the table's end
    knots[..., n - 1, 1] = fp[..., n - 1] * inv_h
    return knots


class EAM:
    def __init__(self, rc, dr, drho, F_rho, rho_r, rphi_r):
        self.rc, self.dr, self.drho = float(rc), float(dr), float(drho)
        F_rho, rho_r, rphi_r = (np.asarray(a, dtype=f64) for a in (F_rho, rho_r, rphi_r))
        self.nelem, self.nrho, self.nr = int(F_rho.shape[0]), int(F_rho.shape[1]), int(rho_r.shape[1])
        if rho_r.shape != (self.nelem, self.nr) or rphi_r.shape != (self.nelem, self.nelem, self.nr):
            raise ValueError(f"EAM: tables of shapes {F_rho.shape}, {rho_r.shape}, {rphi_r.shape} do not belong together")
        self._host = tuple(np.ascontiguousarray(spline_knots(h, y)) for h, y in ((self.drho, F_rho), (self.dr, rho_r), (self.dr, rphi_r)))
        self._hbm = None  # the same three tables in HBM, from the first call that has device arrays on

    def _tables(self, on_device):
        if not on_device:
            return self._host
        if self._hbm is None:
            self._hbm = tuple(HArray.from_numpy(t) for t in self._host)
        return self._hbm

    def calculate(self, x, y, z, type_list, box, origin, boundary, verlet_list, distance_list, neighbor_number, force, virial, energy,
                  num_t=1, accumulate=True, n_real=None, virial_sum=None):
        """src/eam.cpp:54 — a type outside 0 .. Nelements-1 contributes nothing and receives nothing (the reference indexes its
        spline vectors with it)"""
        N, M = int(verlet_list.shape[0]), int(verlet_list.shape[1])
        _lib.same_rows("EAM.calculate", N, x=x, y=y, z=z, type_list=type_list, distance_list=distance_list,
                       neighbor_number=neighbor_number, force=force, virial=virial, energy=energy)
        if tuple(distance_list.shape) != (N, M) or tuple(force.shape) != (N, 3) or tuple(virial.shape) != (N, 9):
            raise ValueError(f"EAM.calculate: distance_list {tuple(distance_list.shape)}, force {tuple(force.shape)}, virial "
                             f"{tuple(virial.shape)} for a list of shape {(N, M)}")
        if virial_sum is not None and tuple(virial_sum.shape) != (9,):
            raise ValueError("EAM.calculate: virial_sum holds nine numbers")
        keep, (pb, po, pp) = _lib.host_box(box, origin, boundary)
        c = Call(x, y, z, type_list, verlet_list, distance_list, neighbor_number, force, virial, energy, virial_sum)
        tF, tr, tz = self._tables(c.space == _lib.DEVICE)
        add = bool(accumulate)
        rc_ = _lib.lib().mdh_eam(c.inp(x, f64), c.inp(y, f64), c.inp(z, f64), c.inp(type_list, i32), N, pb, po, pp,
                                 c.inp(verlet_list, i32), c.inp(distance_list, f64), c.inp(neighbor_number, i32), M,
                                 c.inp(tF, f64), c.inp(tr, f64), c.inp(tz, f64), self.nelem, self.nrho, self.drho, self.nr, self.dr,
                                 self.rc, int(add), c.out(energy, f64, upload=add), c.out(force, f64, upload=add),
                                 c.out(virial, f64, upload=add), N if n_real is None else int(n_real),
                                 None if virial_sum is None else c.out(virial_sum, f64, upload=False), c.space, c.stream)
        c.done(rc_)
