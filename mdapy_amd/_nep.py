"""Drop-in for ``mdapy._nepcal`` (src/neppy.cpp): the NEP kernels behind ``mdapy_amd.nep.NEP``.  Where the reference's
``NEPCalculator`` reads the file and builds lists of its own, this shim takes the model as arrays and the list as arguments:

``Model(head, zbl, block)`` — the header words (i32: types T, n_max_radial + 1, basis_size_radial + 1, n_max_angular + 1,
basis_size_angular + 1, l_max 3-, 4-, 5-body, neurons, ZBL mode, the block's length, 0), the three ZBL numbers (inner, outer, factor)
and the f64 block in the order include/mdapy_amd.h states ("_nepcal").  The block goes to HBM at the first call with device arrays
and stays there.

``calculate(x, y, z, types, type_map, box, origin, boundary, rows, dist, counts, model, energy=, force=, virial=, virial_sum=,
descriptor=, latent=, n_real=)`` — every output is optional and WRITTEN, never added to.  ``types`` are places in the file's element
list, ``type_map`` (host) takes them to the model's own types, -1 for a type the model was not compacted for."""
import numpy as np

from . import _lib
from .devarray import Call, HArray

f64, i32 = np.float64, np.int32


class Model:
    def __init__(self, head, zbl, block):
        self.head = np.ascontiguousarray(head, dtype=i32)
        self.zbl = np.ascontiguousarray(zbl, dtype=f64)
        self.block = np.ascontiguousarray(block, dtype=f64)
        if self.head.shape != (12,) or self.zbl.shape != (3,) or self.block.ndim != 1 or int(self.head[10]) != len(self.block):
            raise ValueError("NEP model: 12 header words, 3 ZBL numbers and a block of the length the header states are required")
        T, NR, KR, NA, KA, L3, L4, L5, H = (int(v) for v in self.head[:9])
        self.dim, self.neurons = NR + NA * (L3 + (L4 == 2) + (L5 == 1)), H
        self._hbm = None

    def _block(self, on_device):
        if not on_device:
            return self.block
        if self._hbm is None:
            self._hbm = HArray.from_numpy(self.block)
        return self._hbm


def calculate(x, y, z, types, type_map, box, origin, boundary, rows, dist, counts, model, energy=None, force=None, virial=None,
              virial_sum=None, descriptor=None, latent=None, n_real=None):
    N, M = int(rows.shape[0]), int(rows.shape[1])
    _lib.same_rows("NEP.calculate", N, x=x, y=y, z=z, types=types, dist=dist, counts=counts, energy=energy, force=force, virial=virial,
                   descriptor=descriptor, latent=latent)
    for name, a, shape in (("dist", dist, (N, M)), ("force", force, (N, 3)), ("virial", virial, (N, 9)), ("virial_sum", virial_sum, (9,)),
                           ("descriptor", descriptor, (N, model.dim)), ("latent", latent, (N, model.neurons))):
        if a is not None and tuple(a.shape) != shape:
            raise ValueError(f"NEP.calculate: {name} of shape {tuple(a.shape)} where {shape} is required")
    if virial_sum is not None and virial is None:
        raise ValueError("NEP.calculate: virial_sum needs virial")
    type_map = np.ascontiguousarray(type_map, dtype=i32)
    keep, (pb, po, pp) = _lib.host_box(box, origin, boundary)
    c = Call(x, y, z, types, rows, dist, counts, energy, force, virial, virial_sum, descriptor, latent)
    block = model._block(c.space == _lib.DEVICE)
    out = lambda a: None if a is None else c.out(a, f64, upload=False)
    rc_ = _lib.lib().mdh_nep(c.inp(x, f64), c.inp(y, f64), c.inp(z, f64), c.inp(types, i32), N, type_map.ctypes.data, len(type_map),
                             pb, po, pp, c.inp(rows, i32), c.inp(dist, f64), c.inp(counts, i32), M, c.inp(block, f64),
                             model.head.ctypes.data, model.zbl.ctypes.data, N if n_real is None else int(n_real), out(energy), out(force),
                             out(virial), out(virial_sum), out(descriptor), out(latent), c.space, c.stream)
    c.done(rc_)


def calculate_charge(x, y, z, types, type_map, box, origin, boundary, rows, dist, counts, model, kcell, rc_coulomb, energy=None, force=None,
                     virial=None, virial_sum=None, charge=None, bec=None, descriptor=None, latent=None, n_real=None, max_kpoints=1 << 24):
    """``calculate`` for a charge model (``mdh_nep_charge``): ``model`` holds the block of ``QNEP._model_arrays`` (the last header word
    the charge mode), ``kcell`` (3, 3, host) is the cell whose reciprocal vectors the k-space sum runs over — the real cell, where the
    list is a replica's —, ``rc_coulomb`` the model's largest radial cutoff (alpha = pi / rc_coulomb); ``charge`` (N,) and ``bec``
    (N, 9) are further outputs.  The call may hold up to ``max_kpoints`` k-points (48 B each)."""
    N, M = int(rows.shape[0]), int(rows.shape[1])
    _lib.same_rows("NEP.calculate_charge", N, x=x, y=y, z=z, types=types, dist=dist, counts=counts, energy=energy, force=force, virial=virial,
                   charge=charge, bec=bec, descriptor=descriptor, latent=latent)
    for name, a, shape in (("dist", dist, (N, M)), ("force", force, (N, 3)), ("virial", virial, (N, 9)), ("virial_sum", virial_sum, (9,)),
                           ("charge", charge, (N,)), ("bec", bec, (N, 9)), ("descriptor", descriptor, (N, model.dim)),
                           ("latent", latent, (N, model.neurons))):
        if a is not None and tuple(a.shape) != shape:
            raise ValueError(f"NEP.calculate_charge: {name} of shape {tuple(a.shape)} where {shape} is required")
    if virial_sum is not None and virial is None:
        raise ValueError("NEP.calculate_charge: virial_sum needs virial")
    type_map = np.ascontiguousarray(type_map, dtype=i32)
    kcell = np.ascontiguousarray(kcell, dtype=f64)
    if kcell.shape != (3, 3):
        raise ValueError("NEP.calculate_charge: kcell of shape (3, 3) is required")
    keep, (pb, po, pp) = _lib.host_box(box, origin, boundary)
    c = Call(x, y, z, types, rows, dist, counts, energy, force, virial, virial_sum, charge, bec, descriptor, latent)
    block = model._block(c.space == _lib.DEVICE)
    out = lambda a: None if a is None else c.out(a, f64, upload=False)
    rc_ = _lib.lib().mdh_nep_charge(c.inp(x, f64), c.inp(y, f64), c.inp(z, f64), c.inp(types, i32), N, type_map.ctypes.data, len(type_map),
                                    pb, po, pp, c.inp(rows, i32), c.inp(dist, f64), c.inp(counts, i32), M, c.inp(block, f64),
                                    model.head.ctypes.data, model.zbl.ctypes.data, kcell.ctypes.data, float(rc_coulomb), int(max_kpoints),
                                    N if n_real is None else int(n_real), out(energy), out(force), out(virial), out(virial_sum), out(charge),
                                    out(bec), out(descriptor), out(latent), c.space, c.stream)
    c.done(rc_)
