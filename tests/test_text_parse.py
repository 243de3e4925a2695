"""Input side, host checks: the decimal -> double converter of the HIP tokenizer (text_parse.hpp, compiled
for the host as well) against Python's float() — which is what the reference's readers return for every field
(src/mdapy/load_save.py:159-175) — and the generated table of powers of five against exact integer arithmetic."""
import ctypes
import struct

import _text_cases as C
from mdapy_amd import _lib


def _conv(s):
    out = ctypes.c_double(0.0)
    b = s.encode()
    rc = _lib.lib().mdh_debug_parse_double(b, len(b), ctypes.byref(out))
    return rc, out.value


def _same(a, b):
    return struct.pack("<d", a) == struct.pack("<d", b)


def test_power_of_five_table_is_exact():
    L = _lib.lib()
    out = (ctypes.c_uint64 * 2)()
    for q in list(range(-342, 309, 7)) + [-342, -28, -27, -1, 0, 1, 27, 28, 55, 308]:
        if q >= 0:
            c = 5 ** q
            while c < (1 << 127):
                c *= 2
            while c >= (1 << 128):
                c //= 2
        else:
            p = 5 ** -q
            z = 0
            while (1 << z) < p:
                z += 1
            b = z + 127 if q >= -27 else 2 * z + 128
            c = (1 << b) // p + 1
            while c >= (1 << 128):
                c //= 2
        assert L.mdh_debug_text_pow5(q, out) == 0
        assert (int(out[0]) << 64) | int(out[1]) == c, q


def _by_class(*tags):
    return [s for tag, s in C.cases() if tag in tags]


def test_fields_round_exactly_like_float():
    cases = _by_class("basic", "repr", "g6", "f15", "int19", "half53", "e17")
    assert len(cases) > 59000
    redo = 0
    for s in cases:
        rc, v = _conv(s)
        if rc == 1:
            redo += 1
            continue
        assert rc == 0, s
        assert _same(v, float(s)), (s, v, float(s))
    assert redo == 0  # at most 19 significant digits everywhere above: always decided


def test_long_fields_are_decided_or_handed_back():
    cases = _by_class("long")
    assert len(cases) == 20000
    decided = 0
    for s in cases:
        rc, v = _conv(s)
        assert rc in (0, 1)
        if rc == 0:
            decided += 1
            assert _same(v, float(s)), s
    assert decided > 19000
    assert _conv("1.00000000000000011102230246251565404")[0] == 1  # 36 digits, exactly between two doubles
    for s in ("9007199254740993.000000000000000001", "9007199254740993.0000000000000000000"):  # just above / exactly on a halfway point
        rc, v = _conv(s)
        assert rc == 1 or _same(v, float(s))
    for s, want in C.LISTED:
        assert _conv(s)[0] == want, s
    for s in C.MORE_NON_NUMBERS:
        assert _conv(s)[0] == {"naninf": 1, "hex": 1, "bad": 2}[C.kind_of(s)], s


def test_halfway_subnormal_zero_padded_and_swept_fields():
    """the classes of _text_cases.py that reach what plain coordinates never do: exact halfway points with decimal exponents
    -4 .. 23 (the round-to-even branch) and their neighbours one unit of the 19th digit away, the subnormal band, zeros that
    are not significant digits, eight significands against every decimal exponent from underflow to overflow, and spellings of
    sign and exponent.  Bit for bit float() (the sign of -0.0 included); a field is handed back only when it has more than
    19 significant digits and the first 19 leave the rounding open."""
    per_class = {}
    exps = set()
    for tag, s in C.cases():
        if tag not in C.NEW_CLASSES:
            continue
        per_class[tag] = per_class.get(tag, 0) + 1
        rc, v = _conv(s)
        if C.significant_digits(s) <= 19:
            assert rc == 0, (tag, s)
        else:
            assert rc == (0 if C.decided_with_19_digits(s) else 1), (tag, s)
        if rc == 0:
            assert _same(v, float(s)), (tag, s, v, float(s))
        if tag == "halfway" and "e" in s:
            exps.add(int(s.split("e")[1]))
    assert set(per_class) == set(C.NEW_CLASSES) and per_class["halfway"] > 500 and per_class["sweep"] == 8 * 657
    assert exps >= set(range(-4, 24))  # the decimal exponents at which a 19-digit significand can lie exactly halfway
    for s, want in (("-0", -0.0), ("-0.0", -0.0), ("+.5", 0.5), ("5.", 5.0), ("1E5", 1e5), ("1e+05", 1e5), ("1e00000000000000000005", 1e5),
                    ("1e-99999999", 0.0)):
        rc, v = _conv(s)
        assert rc == 0 and _same(v, want), s


def test_every_case_of_the_shared_list_agrees_with_float():
    """the whole list, as the GPU test feeds it to the kernels: 0 mismatches, nothing of <= 19 significant digits handed back"""
    mismatches, handed_back_short = [], []
    for tag, s in C.cases():
        rc, v = _conv(s)
        kind = C.kind_of(s)
        if kind != "number":
            assert rc == (2 if kind == "bad" else 1), s
            continue
        if rc == 0 and not _same(v, float(s)):
            mismatches.append(s)
        if rc != 0 and C.significant_digits(s) <= 19:
            handed_back_short.append(s)
        assert rc == (0 if C.decided_with_19_digits(s) else 1), s
    assert not mismatches, (len(mismatches), mismatches[:20])
    assert not handed_back_short, handed_back_short[:20]
