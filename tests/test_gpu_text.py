"""The device tokenizer (csrc/text.hip: k_count_lines, k_line_starts, k_parse_rows; text_parse.hpp compiled for the device)
against plain Python.

The reference is restated here in a few lines: ``text.split(b"\\n")`` for the rows, the device's blank set ``b" \\t\\r"`` for the
fields, ``float()`` / ``int()`` for the numbers and little-endian packing of up to 8 bytes for the strings.  It never calls the
library's host converter.  Every comparison is of bit patterns: the converter's contract is correct rounding, so there is no
tolerance.  The one cap — under 5 % of the 20-39-digit fields handed back — is the host test's (test_text_parse.py).

``mdh_parse_table`` is called directly, with device text and device columns, where ``status4`` and the raw ``redo`` list are the
subject; ``_text.parse_table`` where the patched result is.  The columns start out filled with a sentinel, so a field the
kernel must not store (short rows, rows the text does not have) is checked as well."""
import ctypes
import io
import re
import struct

import numpy as np
import pytest

import _text_cases as C

pytestmark = pytest.mark.gpu

FLOAT, INT, STR, SKIP = 0, 1, 2, 3
SENT64, SENT32 = 0x5A5A5A5A5A5A5A5A, 0x5A5A5A5A
BLOCK = 4096  # bytes of text per workgroup of k_count_lines / k_line_starts
_FIELD = re.compile(rb"[^ \t\r]+")
_INT = re.compile(rb"[+-]?[0-9]+\Z")


@pytest.fixture(autouse=True)
def _need_gpu():
    from mdapy_amd import _lib

    if _lib.device_count() < 1:
        pytest.fail("test_gpu_text needs a HIP device")


# ---- the restatement
def _lines(text):
    lines = text.split(b"\n")
    if lines[-1] == b"":
        lines.pop()
    return lines


def _float_field(tok):
    """(bits or None when handed back, not a number at all)"""
    s = tok.decode("latin-1")
    kind = C.kind_of(s)
    if kind != "number":
        return None, kind == "bad"
    if not C.decided_with_19_digits(s):
        return None, False
    return struct.unpack("<q", struct.pack("<d", float(s)))[0], False


def _expect(text, nrows, kinds):
    """what mdh_parse_table must leave: per column the stored bit patterns (the sentinel where nothing may be stored) and which
    of them are pinned down (a handed-back field's slot is not), the hand-back list {row * ncol + column: (offset, length)} and
    status4 = (handed back, rows missing or short, not numbers, lines present)"""
    ncol = len(kinds)
    cols = [None if k == SKIP else np.full(nrows, SENT32 if k == INT else SENT64, np.int64) for k in kinds]
    care = [None if k == SKIP else np.ones(nrows, bool) for k in kinds]
    redo, short, bad = {}, 0, 0
    lines = _lines(text)
    at = 0
    for r, line in enumerate(lines[:nrows]):
        fields = list(_FIELD.finditer(line))[:ncol]
        for c, m in enumerate(fields):
            tok, k, v = m.group(), kinds[c], None
            if k == FLOAT:
                v, isbad = _float_field(tok)
                bad += isbad
            elif k == INT:
                if _INT.match(tok) and -2 ** 31 <= int(tok) < 2 ** 31:
                    v = int(tok)
                bad += tok in (b"+", b"-")
            elif k == STR:
                if len(tok) <= 8:
                    v = int.from_bytes(tok, "little")
                    v -= (v >> 63) << 64
            else:
                continue
            if v is None:
                redo[r * ncol + c] = (at + m.start(), min(len(tok), 65535))
                care[c][r] = False
            else:
                cols[c][r] = v
        short += len(fields) < ncol
        at += len(line) + 1
    short += max(0, nrows - len(lines))
    return cols, care, redo, (len(redo), short, bad, len(lines))


def _patched(text, nrows, kinds):
    """what _text.parse_table returns for a text it accepts: float() / int() / the token itself, None for a skipped column"""
    rows = [[m.group() for m in _FIELD.finditer(line)] for line in _lines(text)[:nrows]]
    out = []
    for c, k in enumerate(kinds):
        col = [r[c] for r in rows]
        out.append(None if k == SKIP else [float(t) for t in col] if k == FLOAT else [int(t) for t in col] if k == INT else [t.decode() for t in col])
    return out


# ---- the device side
def _upload(text, shift=0):
    """the text in HBM, its first byte ``shift`` bytes past a 16-byte boundary"""
    import torch

    buf = torch.zeros(len(text) + 32, dtype=torch.uint8, device="cuda")
    shift += (-buf.data_ptr()) % 16
    if text:
        buf[shift:shift + len(text)] = torch.frombuffer(bytearray(text), dtype=torch.uint8).cuda()
    view = buf[shift:shift + len(text)]
    assert len(text) == 0 or view.data_ptr() % 16 == shift % 16
    return buf, view


def _raw(view, nbytes, nrows, kinds, redo_cap):
    """mdh_parse_table on device text -> (columns as bit patterns, redo rows actually listed, status4)"""
    import torch

    from mdapy_amd import _lib
    from mdapy_amd.devarray import current_stream_ptr

    ncol = len(kinds)
    cols = [None if k == SKIP else torch.full((max(nrows, 1),), SENT32 if k == INT else SENT64, dtype=torch.int32 if k == INT else torch.int64, device="cuda")
            for k in kinds]
    ptrs = (ctypes.c_void_p * ncol)(*[None if c is None else c.data_ptr() for c in cols])
    kind_arr = np.asarray(kinds, dtype=np.int32)
    redo = torch.full((2 * max(redo_cap, 1),), -1, dtype=torch.int64, device="cuda")
    status = np.full(4, -7, dtype=np.int64)
    rc = _lib.lib().mdh_parse_table(int(view.data_ptr()) if nbytes else int(redo.data_ptr()), nbytes, _lib.DEVICE, nrows, ncol, kind_arr.ctypes.data, ptrs,
                                    redo.data_ptr(), redo_cap, status.ctypes.data, _lib.DEVICE, current_stream_ptr())
    _lib.check(rc)
    torch.cuda.synchronize()
    got = [None if c is None else c.cpu().numpy().astype(np.int64) for c in cols]
    return got, redo.cpu().numpy().reshape(-1, 2), tuple(int(v) for v in status)


def _check(text, nrows, kinds, shift=0, expect=None, bad=True):
    want_cols, care, want_redo, want_status = expect or _expect(text, nrows, kinds)
    keep, view = _upload(text, shift)
    got, redo, status = _raw(view, len(text), nrows, kinds, max(len(want_redo), 1))
    if len(text) == 0 or nrows == 0:
        want_status = (0, 0, 0, 0)  # no kernel runs; the caller (parse_table) turns lines < nrows into its error
    assert status[:2] == want_status[:2] and status[3] == want_status[3], (status, want_status)
    if bad:
        assert status[2] == want_status[2], (status, want_status)
    for c, (g, w) in enumerate(zip(got, want_cols)):
        if w is None:
            continue
        g = g[:nrows]
        wrong = np.flatnonzero((g != w) & care[c])
        assert wrong.size == 0, (c, wrong[:5], [hex(int(v) & (2 ** 64 - 1)) for v in g[wrong[:5]]], [hex(int(v) & (2 ** 64 - 1)) for v in w[wrong[:5]]])
    listed = {int(w): (int(p) >> 16, int(p) & 0xFFFF) for w, p in redo[:status[0]]}
    assert listed == want_redo
    assert (redo[status[0]:] == -1).all()
    del keep
    return got, listed, status


# ---- 2a  the converter
_TABLE = {}


def _case_table():
    """the whole case list as rows of 8 FLOAT columns (the empty spelling cannot be a field) + what the device must make of it"""
    if not _TABLE:
        fields = [(tag, s) for tag, s in C.cases() if s]
        while len(fields) % 8:
            fields.append(("basic", "0"))
        text = "".join(" ".join(s for _, s in fields[i:i + 8]) + "\n" for i in range(0, len(fields), 8)).encode()
        _TABLE.update(fields=fields, text=text, nrows=len(fields) // 8, expect=_expect(text, len(fields) // 8, [FLOAT] * 8))
    return _TABLE


def test_converter_on_device_rounds_like_float():
    """every field the device decides has float()'s bits (the sign of -0.0 included); what it hands back is exactly the fields
    whose first 19 significant digits leave the rounding open, the nan / inf and hex spellings and the not-a-numbers, each with
    its row * ncol + column, byte offset and length; status4[2] counts the not-a-numbers alone"""
    T = _case_table()
    fields, text, nrows = T["fields"], T["text"], T["nrows"]
    assert nrows > 12000 and 2 << 20 < len(text) < 5 << 20
    _, listed, status = _check(text, nrows, [FLOAT] * 8, expect=T["expect"])
    kinds = [C.kind_of(s) for _, s in fields]
    assert status[2] == kinds.count("bad") > 10
    back = set(listed)
    for i, ((tag, s), kind) in enumerate(zip(fields, kinds)):
        if kind != "number":
            assert i in back, s
        elif C.significant_digits(s) <= 19:
            assert i not in back, (tag, s)  # 19 digits fit the 64-bit significand: always decided
    long_ones = [i for i, (tag, _) in enumerate(fields) if tag == "long"]
    assert len(long_ones) == 20000
    assert sum(i in back for i in long_ones) < 0.05 * len(long_ones)  # the host test's cap: more than 19 000 of 20 000 decided


def test_converter_fields_patched_by_parse_table():
    """the same table through _text.parse_table (the fields float() itself rejects replaced): after the hand-backs are patched
    every finite field and every infinity has float()'s bits, and the nans stand where they were spelled"""
    import torch

    from mdapy_amd import _text

    T = _case_table()

    def accepted(s):
        try:
            float(s)
            return "_" not in s
        except ValueError:
            return False

    fields = [s if accepted(s) else "0" for _, s in T["fields"]]
    assert sum(f in ("nan", "NaN", "+nan") for f in fields) == 3 and "-inf" in fields and "+Infinity" in fields
    text = "".join(" ".join(fields[i:i + 8]) + "\n" for i in range(0, len(fields), 8)).encode()
    keep, view = _upload(text)
    cols, lines = _text.parse_table(view, T["nrows"], [FLOAT] * 8, redo_cap=len(fields))
    torch.cuda.synchronize()
    assert lines == T["nrows"]
    got = np.column_stack([c.numpy() for c in cols]).ravel()
    want = np.array([float(s) for s in fields])
    nan = np.isnan(want)
    assert nan.sum() == 3 and np.array_equal(np.isnan(got), nan)
    wrong = np.flatnonzero((got.view(np.int64) != want.view(np.int64)) & ~nan)
    assert wrong.size == 0, [(fields[i], got[i], want[i]) for i in wrong[:10]]


# ---- 2b  integers
INT_SPELLINGS = ("0", "-0", "+0", "+7", "2147483647", "-2147483648", "2147483648", "-2147483649", "4294967296", "4294967297", "-4294967296", "-4294967297",
                 "123456789012345678901234567890", "-123456789012345678901234567890", "0" * 40 + "5", "-" + "0" * 40 + "5", "0" * 40 + "2147483648",
                 "3.0", "1e3", "-", "+", "12a", "9223372036854775807", "18446744073709551616", "18446744073709551617", "-18446744071562067968",
                 "2147483647", "-2147483647", "99999999999", "1_0", "٣")


def test_int32_fields_at_their_boundaries():
    """a field is decided exactly when it is [+-]?[0-9]+ and fits int32, and then holds int(field); everything else — one past
    either end, values that wrap to something small modulo 2^32 or 2^64, 3.0, 1e3, a bare sign, 12a — is handed back"""
    text = "".join(s + "\n" for s in INT_SPELLINGS).encode()
    cols, care, redo, status = expect = _expect(text, len(INT_SPELLINGS), [INT])
    decided = {s for r, s in enumerate(INT_SPELLINGS) if care[0][r]}
    assert decided == {"0", "-0", "+0", "+7", "2147483647", "-2147483648", "0" * 40 + "5", "-" + "0" * 40 + "5", "-2147483647"}
    assert cols[0][4] == 2 ** 31 - 1 and cols[0][5] == -2 ** 31 and cols[0][14] == 5 and cols[0][15] == -5
    _check(text, len(INT_SPELLINGS), [INT], expect=expect, bad=False)
    two = "".join(f"{s} {t}\n" for s, t in zip(INT_SPELLINGS, reversed(INT_SPELLINGS))).encode()
    _check(two, len(INT_SPELLINGS), [INT, INT], bad=False)


# ---- 2c  strings
STR_TOKENS = ("H", "Cu", "abc", "abcd", "abcde", "abcdef", "abcdefg", "abcdefgh", "abcdefghi", "Unobtainium", "Å", "ÅÅÅÅ", "abcdefÅ", "ÅÅÅÅa", "abcdefgÅ", "é",
              "日本", "日本語", "\x7f" * 8, "a" * 100, "-1.5", "0", "ÿ" * 4)


def test_strings_pack_little_endian_up_to_eight_bytes():
    """tokens of 1 to 8 bytes pack little-endian (multi-byte UTF-8 included; a last byte >= 0x80 makes the int64 code negative),
    9 bytes and more are handed back; through parse_table the object array is the tokens"""
    import torch

    from mdapy_amd import _text

    text = "".join(s + "\n" for s in STR_TOKENS).encode()
    n = len(STR_TOKENS)
    cols, care, redo, status = expect = _expect(text, n, [STR])
    assert [len(s.encode()) > 8 for s in STR_TOKENS] == [not ok for ok in care[0]]
    assert cols[0][STR_TOKENS.index("ÅÅÅÅ")] < 0 and cols[0][STR_TOKENS.index("abcdefÅ")] < 0 and cols[0][1] == 0x7543
    _check(text, n, [STR], expect=expect)
    keep, view = _upload(text)
    got, lines = _text.parse_table(view, n, [STR])
    torch.cuda.synchronize()
    assert lines == n and list(got[0]) == list(STR_TOKENS) and got[0].dtype == object


@pytest.mark.parametrize("ncol", [1, 64])
def test_column_counts_one_and_sixty_four_with_skipped_columns(ncol):
    """ncol = 1 and the maximum of 64, kinds cycling through all four: a SKIP column comes back as None and the columns next to
    it hold what stands in their own fields"""
    import torch

    from mdapy_amd import _text

    rng = np.random.default_rng(64 + ncol)
    kinds = [[FLOAT, SKIP, STR, INT][c % 4] for c in range(ncol)] if ncol > 1 else [STR]
    n = 300
    make = {FLOAT: lambda: repr(float(rng.normal() * 10.0 ** int(rng.integers(-30, 30)))), INT: lambda: str(int(rng.integers(-2 ** 31, 2 ** 31))),
            STR: lambda: STR_TOKENS[int(rng.integers(len(STR_TOKENS)))], SKIP: lambda: "skipped" + "x" * int(rng.integers(0, 9))}
    text = "".join(" ".join(make[k]() for k in kinds) + "\n" for _ in range(n)).encode()
    _check(text, n, kinds)
    keep, view = _upload(text)
    got, lines = _text.parse_table(view, n, kinds)
    torch.cuda.synchronize()
    want = _patched(text, n, kinds)
    assert lines == n
    for k, g, w in zip(kinds, got, want):
        if k == SKIP:
            assert g is None
        elif k == STR:
            assert list(g) == w
        else:
            a = g.numpy()
            assert a.dtype == (np.float64 if k == FLOAT else np.int32) and a.tobytes() == np.array(w, dtype=a.dtype).tobytes()


# ---- 2d  the row splitter
KINDS3 = [INT, FLOAT, STR]


def _rows(n, seed, crlf=0.0, wide=False):
    """n rows 'id x name' with the blanks files have: runs of spaces and tabs, blanks before the first and after the last field"""
    rng = np.random.default_rng(seed)
    names = ("Cu", "Zr", "H", "Unobtainium", "abcdefgh")
    rows = []
    for i in range(n):
        gap = [(" ", "\t", "  ", " \t ", "   ")[int(rng.integers(5))] for _ in range(2)]
        lead = ("", "", " ", "\t", "  ")[int(rng.integers(5))]
        tail = ("", "", " ", " \t", " extra fields 7")[int(rng.integers(5))]
        if wide:
            gap[int(rng.integers(2))] = " " * int(rng.integers(200, 1400))
        rows.append((lead + str(i + 1) + gap[0] + repr(float(rng.uniform(-500, 500))) + gap[1] + names[int(rng.integers(5))] + tail
                     + ("\r" if rng.random() < crlf else "")).encode())
    return rows


def _pad(rows, nbytes):
    """blanks after the last row so far, so that with its newline the text is ``nbytes`` long"""
    have = sum(len(r) + 1 for r in rows)
    assert have <= nbytes
    rows[-1] += b" " * (nbytes - have)


SIZES = (15, 16, 17, 31, 32, 33, 4095, 4096, 4097, 4111, 4112, 4113, 8191, 8192, 8193)
_ALIGN = {}


def _align_text():
    if not _ALIGN:
        text = b"\n".join(_rows(400, 1, crlf=0.3)) + b"\n"
        assert len(text) > max(SIZES)
        _ALIGN["text"] = text
        for nbytes in SIZES:
            cut = text[:nbytes]
            nrows = len(_lines(cut))
            _ALIGN[nbytes] = (cut, nrows, _expect(cut, nrows, KINDS3))
    return _ALIGN


@pytest.mark.parametrize("shift", range(16))
def test_every_alignment_of_the_text_base(shift):
    """newline_count16 takes one 16-byte load per lane when the address allows it and single bytes otherwise: every alignment of
    the base, sizes one below, on and above one and two blocks and a multiple of 16 (the cut goes through the middle of a row)"""
    A = _align_text()
    for nbytes in SIZES:
        cut, nrows, expect = A[nbytes]
        _check(cut, nrows, KINDS3, shift=shift, expect=expect)


def test_newlines_and_rows_at_block_edges():
    """a newline as the last byte of a block and another as the first byte of the next (the empty row between them is a short
    row), a row that straddles an edge, and a one-byte text"""
    rows = _rows(60, 2)
    _pad(rows, BLOCK)  # the newline of row 59 is byte 4095
    rows.append(b"")  # its own newline is byte 4096
    rows += _rows(50, 3)
    text = b"\n".join(rows) + b"\n"
    assert text[BLOCK - 1:BLOCK + 1] == b"\n\n"
    _, _, status = _check(text, len(rows), KINDS3)
    assert status[1] == 1 and status[3] == 111
    rows = _rows(60, 4)
    _pad(rows, BLOCK - 7)
    rows += [b"7777 -1.25e-3 Zr"] + _rows(70, 5)  # bytes 4089 .. 4104
    _pad(rows, 2 * BLOCK - 3)
    rows += [b"8888\t2.5\tabcdefgh", b"1 2 3"]  # bytes 8189 ..
    for last in (b"\n", b""):
        text = b"\n".join(rows) + last
        got, _, status = _check(text, len(rows), KINDS3)
        assert got[0][60] == 7777 and got[0][131] == 8888 and status[1] == 0
    for text in (b"\n", b"5", b"5\n", b" ", b"\r\n"):
        _check(text, 1, [INT])
        _check(text, 3, [INT])


def test_rows_longer_than_a_block():
    """blocks without a newline: a row of more than 4096 bytes and one of more than 8192, padded with blanks or with extra fields
    beyond ncol, between ordinary rows"""
    rows = _rows(5, 6)
    rows.append(b"101 " + b" " * 5000 + b"1.5" + b"\t" * 300 + b"Cu")
    rows += _rows(3, 7)
    rows.append(b"102 2.5 Zr " + b" ".join(b"%d" % k for k in range(2500)))
    rows.append(b" " * 9000 + b"103 3.5 H")
    rows.append(b"104 4.5 He" + b" " * 9000)
    rows.append(b" " * 4096)
    rows += _rows(3, 8)
    assert len(rows[5]) > BLOCK and len(rows[9]) > 2 * BLOCK and len(rows[10]) > 2 * BLOCK
    for last in (b"\n", b""):
        got, _, status = _check(b"\n".join(rows) + last, len(rows), KINDS3)
        assert list(got[0][[5, 9, 10, 11]]) == [101, 102, 103, 104] and status[1] == 1


@pytest.mark.parametrize("nrows", [1, 255, 256, 257, 513])
def test_one_character_rows_and_more_than_one_block_of_rows(nrows):
    """k_parse_rows gives a row to a lane, 256 to a block: 257 and 513 rows, here of one character each"""
    digits = "".join(str((7 * i) % 10) + "\n" for i in range(nrows)).encode()
    got, _, _ = _check(digits, nrows, [INT])
    assert list(got[0][:nrows]) == [(7 * i) % 10 for i in range(nrows)]
    _check(digits, nrows, [STR])
    _check(digits, nrows, KINDS3)  # every row is short
    _check(digits[:-1], nrows, [FLOAT])


def test_text_beyond_the_first_block_of_the_prefix_scan():
    """just over 4 MiB: more than 1024 blocks of newline counts, so their prefix sum is carried from one scan block into the
    next; every row is compared, the first to begin past the 4 MiB mark by name"""
    rows = _rows(6000, 9, crlf=0.1, wide=True)
    text = b"\n".join(rows) + b"\n"
    assert 1024 * BLOCK + 8 * BLOCK < len(text) < 6 << 20
    starts = np.cumsum([0] + [len(r) + 1 for r in rows])
    first = int(np.searchsorted(starts, 1024 * BLOCK))
    assert 100 < first < len(rows) - 10
    got, _, status = _check(text, len(rows), KINDS3)
    assert list(got[0][first - 1:first + 2]) == [first, first + 1, first + 2] and status[3] == len(rows)


def test_line_ends_blanks_and_trailing_blank_lines():
    """CRLF throughout, tabs and runs of blanks, a last row with and without its newline, blank lines after the table"""
    rows = _rows(40, 10, crlf=1.0)
    for tail in (b"\r\n", b"", b"\r", b"\r\n\r\n\r\n", b"\n\n\n", b"\n \n\t\r\n"):
        text = b"\n".join(rows) + tail
        _, _, status = _check(text, 40, KINDS3)
        assert status[1] == 0 and status[3] == len(_lines(text))
    text = b"\n".join(_rows(40, 11)) + b"\n"
    _, _, status = _check(text, 40, KINDS3)
    assert status[1] == 0 and status[3] == 40


def test_more_and_fewer_lines_than_rows():
    """more lines than rows (the next frame's header follows): the first nrows rows are parsed and status4[3] is the number of
    lines present; fewer lines, a short row, a blank line in the middle and a whitespace-only line: status4[1] counts each"""
    rows = _rows(30, 12)
    more = b"\n".join(rows) + b"\nITEM: TIMESTEP\n100\nITEM: NUMBER OF ATOMS\n30\n"
    _, names, status = _check(more, 30, KINDS3)  # (handed back: the names of more than 8 bytes)
    assert status[1] == 0 and status[3] == 34
    _, _, status = _check(more, 10, KINDS3)
    assert status[1] == 0 and status[3] == 34
    _, listed, status = _check(more, 32, KINDS3)  # 'ITEM: TIMESTEP' is a row with two fields, neither an int nor a float; '100' is short
    assert status[1] == 2 and status[2] == 1 and set(listed) - set(names) == {30 * 3, 30 * 3 + 1}
    text = b"\n".join(rows) + b"\n"
    _, _, status = _check(text, 37, KINDS3)
    assert status[1] == 7 and status[3] == 30
    _, _, status = _check(text[:-1], 31, KINDS3)
    assert status[1] == 1 and status[3] == 30
    odd = list(rows)
    odd[4] = b"5 1.5"
    odd[11] = b""
    odd[17] = b" \t \r"
    odd[29] = b"30"
    _, _, status = _check(b"\n".join(odd) + b"\n", 30, KINDS3)
    assert status[1] == 4 and status[3] == 30
    _, _, status = _check(b"\n".join(odd), 33, KINDS3)
    assert status[1] == 7 and status[3] == 30


def test_empty_text_and_no_rows_touch_nothing():
    """nbytes = 0 and nrows = 0 return at once: status all zero, the columns and the hand-back list as they were; parse_table
    turns the missing rows into its 'expected N atom rows' error"""
    from mdapy_amd import _text

    text = b"\n".join(_rows(5, 13)) + b"\n"
    got, listed, status = _check(b"", 5, KINDS3)
    assert status == (0, 0, 0, 0) and not listed and all((g == (SENT32 if k == INT else SENT64)).all() for g, k in zip(got, KINDS3))
    got, listed, status = _check(text, 0, KINDS3)
    assert status == (0, 0, 0, 0) and not listed and all((g == (SENT32 if k == INT else SENT64)).all() for g, k in zip(got, KINDS3))
    keep, view = _upload(b"")
    with pytest.raises(ValueError, match="expected 5 atom rows"):
        _text.parse_table(view, 5, KINDS3)


# ---- 2e  the double-buffered upload
class _Source(io.BytesIO):
    def __init__(self, data):
        super().__init__(data)
        self.reads = 0

    def readinto(self, view):
        self.reads += 1
        return super().readinto(view)


@pytest.mark.parametrize("chunk", [4096, 1000])
def test_stream_to_device_hands_over_between_its_two_buffers(chunk):
    """a few hundred KB through 4096- and 1000-byte pinned buffers — hundreds of hand-overs — with the size known, unknown, too
    small (the file grew), too large, and an empty source: the tensor holds the source's bytes and the stated total"""
    from mdapy_amd import _text

    data = np.random.default_rng(chunk).integers(0, 256, 300_001, dtype=np.uint8).tobytes()
    for nbytes in (len(data), None, len(data) - 12_345, 5, 0, len(data) + 777, 2 * len(data)):
        src = _Source(data)
        got, total = _text.stream_to_device(src, nbytes, chunk=chunk)
        assert total == len(data) and got.numel() == total and got.is_cuda and got.element_size() == 1
        assert got.cpu().numpy().tobytes() == data
        assert src.reads > len(data) // chunk
    for nbytes in (0, None, 100):
        got, total = _text.stream_to_device(io.BytesIO(b""), nbytes, chunk=chunk)
        assert total == 0 and got.numel() == 0
    tail = io.BytesIO(data)
    tail.seek(len(data) - 2500)  # from where the source stands, not from its start
    got, total = _text.stream_to_device(tail, 2500, chunk=chunk)
    assert total == 2500 and got.cpu().numpy().tobytes() == data[-2500:]


# ---- the hand-back of a token longer than its length field
def test_a_token_longer_than_the_length_field_comes_back_whole():
    """redo packs a token's length into 16 bits (65 535 = that long or longer): parse_table finds the end of such a token itself
    and returns all of it, a 70 000-byte name as well as one of exactly 65 535 and of 65 536 bytes"""
    import torch

    from mdapy_amd import _text

    names = ["Cu", "n" * 70_000, "Zr", "m" * 65_535, "k" * 65_536, "j" * 65_534, "Unobtainium", "q" * 70_001]
    for last in ("\n", ""):
        text = ("\n".join(f"{i + 1} {0.5 * i!r} \t{nm} \t" for i, nm in enumerate(names)) + last)
        if not last:
            text = text.rstrip(" \t")  # the long token ends with the text
        text = text.encode()
        _check(text, len(names), KINDS3)
        keep, view = _upload(text)
        got, lines = _text.parse_table(view, len(names), KINDS3)
        torch.cuda.synchronize()
        assert [len(s) for s in got[2]] == [len(s) for s in names] and list(got[2]) == names
        assert list(got[0].numpy()) == list(range(1, len(names) + 1))
    # as a number: float() of the whole token, not of its first zeros (34 digits just above a halfway point: handed back)
    field = "0" * 70_000 + "9007199254740993.000000000000000001"
    text = ("1 " + field + " Cu\n2 " + "0" * 70_000 + "1.5 Zr\n").encode()
    _, listed, _ = _check(text, 2, KINDS3)
    assert listed == {1: (2, 65535)}
    keep, view = _upload(text)
    got, _ = _text.parse_table(view, 2, KINDS3)
    assert got[1].numpy().tobytes() == np.array([float(field), 1.5]).tobytes() and float(field) == 9007199254740994.0


# ---- device and host readers on files that are merely odd
DUMP_HEAD = "ITEM: TIMESTEP\n7\nITEM: NUMBER OF ATOMS\n{n}\nITEM: BOX BOUNDS pp pp pp\n0 10\n0 10\n0 10\nITEM: ATOMS id type x y z element\n"
DUMP_ROWS = ["1 1 0.1 2.5e-3 -7 Cu", "2 2 1.5 -0.0 +3.25 Zr", "3 1 0.30000000000000004 4.9e-324 1e22 Unobtainium", "4 2 9.5 8.25 7.125 H"]
XYZ_HEAD = '{n}\nLattice="10 0 0 0 10 0 0 0 10" Properties=species:S:1:pos:R:3:label:S:1:charge:I:1 pbc="T T F"\n'
XYZ_ROWS = ["Cu 0.5 1.25 2 abcdefgh 1", "Zr 3.0000000000000004 4 5 abcdefghi -2", "Å 6 7.125 8.0625 ÅÅÅÅ 3", "H 1 2 3 ÅÅÅÅa 4"]


def _outcome(path, monkeypatch, device):
    import mdapy_amd.load_save as LS

    with monkeypatch.context() as m:
        if device:
            m.setattr(LS, "DEVICE_MIN_BYTES", 0)
        else:
            m.setattr(LS, "have_gpu", lambda: False)
        try:
            return LS.read_file(path), None
        except Exception as e:  # noqa: BLE001 — the type is what is compared
            return None, e


def _agree(tmp_path, monkeypatch, name, text):
    """the frame of both readers when they accept the file (checked to be the same), else the exception type both raise"""
    from _readers import same

    p = tmp_path / name
    p.write_bytes(text.encode())
    dev, dev_err = _outcome(str(p), monkeypatch, True)
    host, host_err = _outcome(str(p), monkeypatch, False)
    assert type(dev_err) is type(host_err), (name, dev_err, host_err)
    if dev_err is not None:
        return type(dev_err)
    same(dev, host)
    return dev


def test_device_and_host_readers_agree_on_odd_files(tmp_path, monkeypatch):
    """same frame — dtypes and bits — or the same exception type from the device tokenizer and the host's.  What is right is
    what the reference does (load_save.py:141-175, :824-845): the table is the next n lines; rows are split at any white space;
    a row with too few fields, a blank one included, is an error; int('3.0') is an error; the conversion of '1_0' is
    numpy's from a string, which like float() reads 10."""
    head = DUMP_HEAD.format(n=4)
    ok = "\n".join(DUMP_ROWS) + "\n"
    for name, text in (("crlf", (head + ok).replace("\n", "\r\n")), ("blank-tail", head + ok + "\n\n\n"), ("blank-tail-crlf", (head + ok + "\n\n").replace("\n", "\r\n")),
                       ("space-tail", head + ok + "  \t "), ("space-tail-nl", head + ok + "   \n"), ("no-last-newline", head + ok[:-1])):
        fr = _agree(tmp_path, monkeypatch, name + ".dump", text)
        assert list(fr[0]["id"].to_numpy()) == [1, 2, 3, 4] and list(fr[0]["element"].to_numpy()) == ["Cu", "Zr", "Unobtainium", "H"], name
        assert fr[0]["z"].to_numpy().tobytes() == np.array([-7.0, 3.25, 1e22, 7.125]).tobytes(), name
    # a blank or whitespace-only line among the n rows: a row without fields
    for name, rows in (("blank-mid", DUMP_ROWS[:2] + [""] + DUMP_ROWS[2:]), ("space-mid", DUMP_ROWS[:2] + [" \t"] + DUMP_ROWS[2:]),
                       ("blank-first", [""] + DUMP_ROWS), ("space-last-counted", DUMP_ROWS[:3] + ["   "]), ("short-string", DUMP_ROWS[:3] + ["4 2 9.5 8.25 7.125"]),
                       ("short-number", DUMP_ROWS[:3] + ["4 2"])):
        assert _agree(tmp_path, monkeypatch, name + ".dump", head + "\n".join(rows) + "\n") is ValueError, name
    for spelling, error in (("3.0", ValueError), ("1e3", ValueError), ("12a", ValueError), ("2147483648", OverflowError), ("-2147483649", OverflowError)):
        assert _agree(tmp_path, monkeypatch, "id.dump", head + ok.replace("3 1 0.3", spelling + " 1 0.3")) is error, spelling
    fr = _agree(tmp_path, monkeypatch, "id-ends.dump", head + ok.replace("3 1 0.3", "+2147483647 -0 0.3").replace("1 1 0.1", "-2147483648 0007 0.1"))
    assert list(fr[0]["id"].to_numpy()) == [-2 ** 31, 2, 2 ** 31 - 1, 4] and list(fr[0]["type"].to_numpy()) == [7, 2, 0, 2]
    fr = _agree(tmp_path, monkeypatch, "underscore.dump", head + ok.replace("9.5", "1_0"))
    assert fr[0]["x"].to_numpy()[3] == 10.0
    xyz = XYZ_HEAD.format(n=4) + "\n".join(XYZ_ROWS) + "\n"
    for name, text in (("names", xyz), ("names-crlf", xyz.replace("\n", "\r\n")), ("names-tail", xyz + "\n \n")):
        fr = _agree(tmp_path, monkeypatch, name + ".xyz", text)
        assert list(fr[0]["label"].to_numpy()) == ["abcdefgh", "abcdefghi", "ÅÅÅÅ", "ÅÅÅÅa"] and list(fr[0]["element"].to_numpy()) == ["Cu", "Zr", "Å", "H"]
        assert fr[0]["charge"].dtype == np.int32 and list(fr[0]["charge"].to_numpy()) == [1, -2, 3, 4]
    assert _agree(tmp_path, monkeypatch, "blank.xyz", XYZ_HEAD.format(n=4) + "\n".join(XYZ_ROWS[:2] + [""] + XYZ_ROWS[2:]) + "\n") is ValueError
