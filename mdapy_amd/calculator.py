"""``CalculatorMP`` — the abstract base of the static calculators (src/mdapy/calculator.py:23-174): what ``System.calc`` accepts.

A calculator answers five questions about a frame ``(data, box)`` — per-atom energies, their sum, forces, the stress in Voigt
order and per-atom virials — and keeps what it computed in ``results`` until the System that owns it clears that dict (a new
``calc``, ``update_data(..., reset_calculator=True)``)."""
from abc import ABC, abstractmethod


def _asked(answer):
    """an abstract ``get_*(self, data, box)`` whose docstring says what it answers"""
    def getter(self, data, box):
        raise NotImplementedError
    getter.__doc__ = answer
    return abstractmethod(getter)


class CalculatorMP(ABC):
    results = {}  # (the reference's class-level default; every calculator instance assigns its own)
    get_energies = _asked("(N,) f64: the potential energy of every atom")
    get_energy = _asked("the total potential energy")
    get_forces = _asked("(N, 3) f64: the force on every atom")
    get_stress = _asked("(6,) f64: the stress in Voigt order [xx, yy, zz, yz, xz, xy]")
    get_virials = _asked("(N, 9) f64: the virial tensor of every atom, row-major")
