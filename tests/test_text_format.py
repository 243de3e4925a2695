"""The field formatter of csrc/text_format.hpp, compiled for the host (``mdh_debug_format_double`` / ``_float`` / ``_int64``),
against Python's own ``format(x, ".10f")`` and ``str(int)``: bytes, no tolerance.  No GPU needed; tests/test_gpu_text_format.py
sends the same values through the kernels."""
import ctypes
import math
import struct

import numpy as np
import pytest

from _format_cases import SPECIAL, int_classes, random_bit_patterns, tie_values, uniform_values
from mdapy_amd import _lib


@pytest.fixture(scope="module")
def hooks():
    L = _lib.lib()
    buf = ctypes.create_string_buffer(64)
    at = ctypes.addressof(buf)

    def text(n):
        return None if n < 0 else buf.raw[:n].decode()

    return {"double": lambda v: text(L.mdh_debug_format_double(float(v), at)),
            "float": lambda v: text(L.mdh_debug_format_float(ctypes.c_float(v), at)),
            "int": lambda v: text(L.mdh_debug_format_int64(int(v), at))}


@pytest.mark.parametrize("values", [tie_values, lambda: np.array(SPECIAL), random_bit_patterns, uniform_values],
                         ids=["ties", "special", "random-bits", "uniform"])
def test_doubles_equal_format(hooks, values):
    got_all = values()
    assert len(got_all) >= 18
    wrong = [(v, hooks["double"](v), format(v, ".10f")) for v in got_all.tolist() if hooks["double"](v) != format(v, ".10f")]
    assert not wrong, wrong[:5]


def test_ties_are_ties():
    """(the tie class is what it claims: ten decimals leave exactly one half)"""
    from fractions import Fraction

    for v in tie_values()[::97].tolist():
        assert (Fraction(v) * 10 ** 10) % 1 == Fraction(1, 2)


def test_sign_of_zero_and_of_what_rounds_to_zero(hooks):
    assert hooks["double"](-0.0) == "-0.0000000000"
    assert hooks["double"](-1e-12) == "-0.0000000000"
    assert hooks["double"](4.99999999995e-11) == "0.0000000000"
    assert hooks["double"](5e-11) == format(5e-11, ".10f") == "0.0000000001"  # (5e-11 as a double lies above the tie)
    assert hooks["double"](9.99999999995) == format(9.99999999995, ".10f")


def test_non_finite_and_refused(hooks):
    assert hooks["double"](float("nan")) == "NaN"
    assert hooks["double"](-float("nan")) == "NaN"
    assert hooks["double"](float("inf")) == "inf"
    assert hooks["double"](-float("inf")) == "-inf"
    for v in (float(2 ** 64), -float(2 ** 64), 1e30, -1e30, 1.7976931348623157e308):
        assert hooks["double"](v) is None
    big = math.nextafter(float(2 ** 64), 0.0)
    assert hooks["double"](big) == format(big, ".10f") and len(hooks["double"](-big)) == 32


def test_float32_through_exact_promotion(hooks):
    rng = np.random.default_rng(13)
    vals = np.concatenate([rng.standard_normal(20000).astype(np.float32) * np.float32(100), rng.integers(0, 2 ** 32, 20000, dtype=np.uint64).astype(np.uint32).view(np.float32),
                           np.array([1e-45, -1e-45, 1.1754942e-38, 1e-40, 0.1, -0.0, 16777217.0, 1.8e19, 3.4028235e38, np.inf, -np.inf, np.nan], np.float32)])
    for v in vals.tolist():  # (tolist gives the float32's value as a Python float: the exact promotion)
        bits = struct.unpack("<f", struct.pack("<f", v))[0] if v == v else v
        if v != v:
            want = "NaN"
        elif math.isinf(v):
            want = "inf" if v > 0 else "-inf"
        elif abs(v) >= 2.0 ** 64:
            want = None
        else:
            want = format(bits, ".10f")
        assert hooks["float"](v) == want, v


def test_integers(hooks):
    for v in int_classes():
        assert hooks["int"](v) == str(v)
