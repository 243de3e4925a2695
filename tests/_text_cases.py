"""Awkward decimal fields for the text tokenizer's number converter (csrc/text_parse.hpp), one seeded list shared by the host
test (test_text_parse.py, through the host compile of the converter) and the GPU test (test_gpu_text.py, through the kernels).

``cases()`` returns ``[(class tag, field), ...]``, always the same list.  Everything the tests expect of a field is worked out
here from its spelling alone, with ``float()`` as the only converter: how many significant digits it has, whether a converter
that keeps 19 of them can still decide it, and which kind of not-a-number it is."""
import random
import re
import struct
from fractions import Fraction

# the spellings test_text_parse.py has always listed, with the class the converter must give each: 0 decided, 1 handed back
# (nan / inf and hex spellings: the host's float() decides), 2 not a number at all
LISTED = (("nan", 1), ("inf", 1), ("-inf", 1), ("abc", 2), ("1.5x", 1), ("1.5y", 2), ("", 2), ("1e", 2), ("0x10", 1), ("--1", 2))
MORE_NON_NUMBERS = ("NaN", "+Infinity", "-INF", "+nan", "0X1p3", "1e+", ".", "1.2.3", "1_0", "e5", "1e5.0", "1,5", "1d5")

SWEEP_SIGNIFICANDS = ("1", "5", "9999999999999999999", "1844674407370955161", "18446744073709551615", "4940656458412465442",
                      "17976931348623157", "22250738585072014")

_DECIMAL = re.compile(r"[+-]?(?:([0-9]+)\.?([0-9]*)|\.([0-9]+))(?:[eE]([+-]?[0-9]+))?\Z")
_DECIMAL_HEAD = re.compile(r"[+-]?(?:[0-9]+\.?[0-9]*|\.[0-9]+)(?:[eE][+-]?[0-9]+)?")


def bits(v):
    return struct.pack("<d", v)


def parts(s):
    """(digits, exponent) with |value| = int(digits) * 10**exponent, or None when ``s`` is no decimal number"""
    m = _DECIMAL.match(s)
    if not m:
        return None
    whole, frac = (m.group(1), m.group(2)) if m.group(1) is not None else ("", m.group(3))
    return whole + frac, int(m.group(4) or 0) - len(frac)


def significant_digits(s):
    """digits between the first and the last non-zero one (0 for a zero)"""
    return len(parts(s)[0].strip("0"))


def kind_of(s):
    """'number', 'naninf' (sign, then n or i: float() decides), 'hex' (a number, then x) or 'bad'"""
    if parts(s) is not None:
        return "number"
    if re.match(r"[+-]?[nNiI]", s):
        return "naninf"
    m = _DECIMAL_HEAD.match(s)
    if m and s[m.end():m.end() + 1] in ("x", "X"):
        return "hex"
    return "bad"


def decided_with_19_digits(s):
    """what a converter may do that keeps the first 19 significant digits w and knows only whether anything non-zero follows:
    the value lies strictly between w and w + 1 units, so it is decided exactly when both ends round to the same double"""
    digits, q = parts(s)
    lead = digits.lstrip("0")
    if len(lead) <= 19 or not lead[19:].strip("0"):
        return True
    w, q = int(lead[:19]), q + len(lead) - 19
    lo, hi = "%de%d" % (w, q), "%de%d" % (w + 1, q)
    return bits(float(lo)) == bits(float(hi))


def _spell(n, k):
    """n / 2**k exactly: (digits without trailing zeros, decimal exponent)"""
    d, q = n * 5 ** k, -k
    while d % 10 == 0:
        d //= 10
        q += 1
    return str(d), q


def _plain(digits, q):
    if q >= 0:
        return digits + "0" * q
    if -q < len(digits):
        return digits[:q] + "." + digits[q:]
    return "0." + "0" * (-q - len(digits)) + digits


def _halfway(rng, out):
    """(2m + 1) * 2**(e - 1), m a 53-bit significand: every e at which that has at most 19 significant digits.  Odd
    multiples of 5**j keep the digit count down while e grows, which is what takes the decimal exponent up to 23."""
    seen = set()
    for e1 in range(-8, 100):  # e - 1
        for j in range(0, 24):
            for _ in range(3):
                lo, hi = ((1 << 53) + 1 + 5 ** j - 1) // 5 ** j, ((1 << 54) - 1) // 5 ** j
                if lo > hi:
                    continue
                c = rng.randrange(lo, hi + 1) | 1
                if c > hi:
                    continue
                odd = c * 5 ** j  # = 2m + 1
                assert odd & 1 and (1 << 53) < odd < (1 << 54)
                f = Fraction(odd) * Fraction(2) ** e1
                digits, q = _spell(f.numerator, f.denominator.bit_length() - 1)
                if len(digits) > 19 or (e1, digits) in seen:
                    continue
                seen.add((e1, digits))
                pad = 19 - len(digits)
                for tag, d19 in (("halfway", int(digits) * 10 ** pad), ("halfway+", int(digits) * 10 ** pad + 1), ("halfway-", int(digits) * 10 ** pad - 1)):
                    d, qq = str(d19), q - pad
                    while d.endswith("0"):
                        d, qq = d[:-1], qq + 1
                    out.append((tag, _plain(d, qq)))
                    out.append((tag, "%se%d" % (d, qq)))


def _subnormal(rng, out):
    for field in (0, 1, 2):
        for _ in range(300):
            v = struct.unpack("<d", struct.pack("<Q", (rng.getrandbits(1) << 63) | (field << 52) | rng.getrandbits(52)))[0]
            out.extend((("subnormal", repr(v)), ("subnormal", "%.17e" % v), ("subnormal", "%.18e" % v)))
    for v in (5e-324, 2.2250738585072009e-308, 2.2250738585072014e-308, 4.4501477170144023e-308):
        out.extend((("subnormal", repr(v)), ("subnormal", "%.17e" % v), ("subnormal", "%.18e" % v)))


def _zeros(rng, out):
    for z in (1, 2, 7, 18, 19, 20, 21, 39, 40):
        for _ in range(4):
            ddd = str(rng.randrange(1, 10 ** rng.randrange(1, 18)))
            for tail in ("", "e-300", "e-330", "e-%d" % (300 + z), "e300", "e%d" % (308 - z), "e%d" % (300 + z), "e5"):
                out.append(("zeros", "0." + "0" * z + ddd + tail))
                out.append(("zeros", "0" * z + ddd + "." + "0" * z + tail))
                out.append(("zeros", ddd + "0" * z + tail))
                out.append(("zeros", ddd + "." + "0" * z + tail))
                out.append(("zeros", "-" + "0" * z + "." + "0" * z + ddd + "0" * z + tail))
    for z in (1, 19, 20, 40):
        out.extend((("zeros", "0" * z), ("zeros", "0." + "0" * z), ("zeros", "-" + "0" * z + ".e5"), ("zeros", "." + "0" * z + "e-5")))


def _sweep(out):
    for w in SWEEP_SIGNIFICANDS:
        for q in range(-345, 312):
            out.append(("sweep", "%se%d" % (w, q)))


def _earlier(out):
    """the cases test_text_parse.py generated before this module existed, in the same order from the same seeds"""
    for s in ["0", "-0", "0.0", "1", "-1.5", "3.615", "1e22", "1e23", "9007199254740993", "9007199254740992.5", "0.1", "1e-5",
              "123456789012345678", "1234567890123456789", "4.9e-324", "2.4703282292062327e-324", "2.4703282292062328e-324",
              "1.7976931348623157e308", "1.7976931348623159e308", "1e309", "1e-400", "2.2250738585072011e-308", "2.2250738585072014e-308",
              "+7.25", ".5", "5.", "1E5", "1e+5", "00012.500", "8.5e0", "0.000001", "123456.789e-3", "1.0000000000000002"]:
        out.append(("basic", s))
    rng = random.Random(5)
    for _ in range(60000):
        kind = rng.randrange(6)
        if kind == 0:  # shortest round-trip spelling of a random double
            v = struct.unpack("<d", struct.pack("<Q", rng.getrandbits(64)))[0]
            if v != v or v in (float("inf"), float("-inf")):
                continue
            out.append(("repr", repr(v)))
        elif kind == 1:
            out.append(("g6", "%.6g" % rng.uniform(-500, 500)))
        elif kind == 2:
            out.append(("f15", "%.15f" % rng.uniform(-500, 500)))
        elif kind == 3:
            out.append(("int19", "%de%d" % (rng.randrange(10 ** 19), rng.randrange(-340, 300))))
        elif kind == 4:  # exactly halfway between two doubles, and its neighbours
            m = rng.randrange(1 << 52, 1 << 53)
            out.append(("half53", str(2 * m + 1) + rng.choice(["", "e-1", "e0"])))
        else:
            out.append(("e17", "%.17e" % rng.lognormvariate(0, 40)))
    rng = random.Random(9)
    for _ in range(20000):
        digits = "".join(rng.choice("0123456789") for _ in range(rng.randrange(20, 40)))
        out.append(("long", digits[:3] + "." + digits[3:] + rng.choice(["", "e-7", "e12"])))
    for s in ("1.00000000000000011102230246251565404", "9007199254740993.000000000000000001", "9007199254740993.0000000000000000000"):
        out.append(("long-listed", s))


_CASES = None


def cases():
    global _CASES
    if _CASES is None:
        out = []
        _earlier(out)
        rng = random.Random(2021)
        _halfway(rng, out)
        _subnormal(rng, out)
        _zeros(rng, out)
        _sweep(out)
        for s in ("-0", "-0.0", "+.5", "5.", "1E5", "1e+05", "1e00000000000000000005", "1e-99999999", "-0e0", "-0.0e-400", "+0", "-1e-400",
                  "1e99999999", "-1e400", "1e-00000000000000000005", "0e99999999"):
            out.append(("spelling", s))
        for s, _ in LISTED:
            out.append(("non-number", s))
        for s in MORE_NON_NUMBERS:
            out.append(("non-number", s))
        _CASES = out
    return list(_CASES)


NEW_CLASSES = ("halfway", "halfway+", "halfway-", "subnormal", "zeros", "sweep", "spelling")
