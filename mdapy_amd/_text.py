"""Backend shim of the text tokenizer (csrc/text.hip): bytes of an atom table -> typed columns in HBM.

Two pieces: :func:`stream_to_device` moves a file's bytes into HBM through two pinned buffers (the next chunk is read from
the file while the previous one crosses PCIe), :func:`parse_table` runs ``mdh_parse_table`` on the resident text and
patches the few fields the device hands back (``float()`` / ``int()`` on the host — the reference's own conversion).
:func:`scan_sections` finds the section lines of a LAMMPS data file in the resident text (``mdh_scan_sections``).

And of its inverse, the formatter (csrc/text_format.hip): typed columns in HBM -> the bytes of a text table.
:func:`format_table` / :func:`format_chunks` run ``mdh_format_table`` (the whole table, or pieces of rows made on demand),
:func:`stream_from_device` moves text from HBM into a file through two pinned buffers, :func:`format_table_host` writes the
same bytes in plain Python, and :func:`shift_rotate` is what the writers do to positions first."""
import ctypes
import re

import numpy as np

from . import _lib
from .devarray import HArray, current_stream_ptr, torch

FLOAT, INT, STR, SKIP = 0, 1, 2, 3


class RedoOverflow(OverflowError):
    """more fields need the host converter than the hand-back buffer holds (a column of long strings, of nan): the caller
    reads the table with the host tokenizer instead"""

    def __init__(self, n):
        super().__init__(f"{n} fields need the host converter")
        self.n = n

_NP = {FLOAT: np.float64, INT: np.int32, STR: np.int64}
CHUNK = 32 << 20


def stream_to_device(f, nbytes=None, chunk=CHUNK):
    """read ``f`` (binary file object, positioned at the first byte wanted) to its end into one uint8 tensor in HBM.
    ``nbytes``: the size when known (one allocation); otherwise the pieces are concatenated at the end."""
    t = torch()
    pinned = [t.empty(chunk, dtype=t.uint8).pin_memory() for _ in range(2)]
    busy = [None, None]
    side = t.cuda.Stream()
    cur = t.cuda.current_stream()
    pieces, total = [], 0
    whole = t.empty(int(nbytes), dtype=t.uint8, device="cuda") if nbytes is not None else None
    side.wait_stream(cur)  # `whole` may be a block the current stream has only just released: the copies wait for that work
    k = 0
    while True:
        if busy[k] is not None:
            busy[k].synchronize()  # the copy out of this pinned buffer is done
        view = memoryview(pinned[k].numpy())
        got = f.readinto(view)
        if not got:
            break
        if whole is not None and total + got > whole.numel():  # the file grew: fall back to pieces
            pieces, whole = [whole[:total]], None
        with t.cuda.stream(side):
            if whole is not None:
                whole[total:total + got].copy_(pinned[k][:got], non_blocking=True)
            else:
                piece = pinned[k][:got].to("cuda", non_blocking=True)
                piece.record_stream(cur)  # allocated under the side stream, consumed (and freed) on the current one
                pieces.append(piece)
            ev = t.cuda.Event()
            ev.record(side)
        busy[k] = ev
        total += got
        k ^= 1
    side.synchronize()
    t.cuda.current_stream().wait_stream(side)
    if whole is not None:
        return whole[:total], total
    if not pieces:
        return t.empty(0, dtype=t.uint8, device="cuda"), 0
    return (pieces[0] if len(pieces) == 1 else t.cat(pieces)), total


def parse_table(text, nrows, kinds, redo_cap=1 << 16):
    """``text``: uint8 tensor in HBM holding the rows.  Returns (columns, lines_present): per kind an HArray (f64 / i32), a
    numpy object array of strings, or None for skipped columns."""
    t = torch()
    ncol = len(kinds)
    nbytes = int(text.numel())
    cols = [None if k == SKIP else HArray.empty((nrows,), _NP[k]) for k in kinds]
    ptrs = (ctypes.c_void_p * ncol)(*[None if c is None else c.data_ptr() for c in cols])
    kind_arr = np.asarray(kinds, dtype=np.int32)
    redo = HArray.empty((2 * redo_cap,), np.int64)
    status = np.zeros(4, dtype=np.int64)
    rc = _lib.lib().mdh_parse_table(int(text.data_ptr()), nbytes, _lib.DEVICE, int(nrows), ncol, kind_arr.ctypes.data, ptrs,
                                    redo.data_ptr(), int(redo_cap), status.ctypes.data, _lib.DEVICE, current_stream_ptr())
    _lib.check(rc)
    nredo, short, bad, lines = (int(v) for v in status)
    if lines < nrows and not short:  # (no kernel ran — an empty body — or the count fell short without a row noticing)
        short = nrows - lines
    if short:
        raise ValueError(f"expected {nrows} atom rows with {ncol} fields each; {short} rows are missing or too short")
    if nredo > redo_cap:
        raise RedoOverflow(nredo)
    long_strings = {}
    if nredo:
        # the fields the device handed back (strings over 8 bytes, nan / inf, integers spelled 3.0, 20-digit mantissas):
        # their bytes in ONE copy to the host, float() / int() there, the values back with one indexed write per column
        todo = redo.dev()[: 2 * nredo].cpu().numpy().reshape(-1, 2)
        where = todo[:, 0].astype(np.int64)
        off = (todo[:, 1] >> 16).astype(np.int64)
        ln = (todo[:, 1] & 0xFFFF).astype(np.int64)
        span = np.where(ln == 0xFFFF, 0, ln)  # (0xFFFF: that long or longer — those are fetched one by one, below)
        starts = np.concatenate([[0], np.cumsum(span)])[:-1]
        idx = (np.repeat(off - starts, span) + np.arange(int(span.sum()))).clip(max=max(nbytes - 1, 0))
        blob = text[t.from_numpy(idx).to(text.device)].cpu().numpy().tobytes()
        rows_of, vals_of = {}, {}
        for q in range(nredo):
            r, c = divmod(int(where[q]), ncol)
            raw = _long_token(text, int(off[q]), nbytes) if ln[q] == 0xFFFF else blob[int(starts[q]): int(starts[q] + span[q])]
            tok = raw.decode()
            if kinds[c] == STR:
                long_strings.setdefault(c, {})[r] = tok
            else:  # float() / int() raise ValueError for what they reject, as the reference's conversion does
                val = float(tok) if kinds[c] == FLOAT else int(tok)
                if kinds[c] == INT and not -2 ** 31 <= val < 2 ** 31:
                    raise OverflowError(f"Python integer {val} out of bounds for int32")
                rows_of.setdefault(c, []).append(r)
                vals_of.setdefault(c, []).append(val)
        for c, rows in rows_of.items():
            dev = cols[c].dev()
            dev[t.as_tensor(rows, dtype=t.int64, device=dev.device)] = t.as_tensor(vals_of[c], dtype=dev.dtype, device=dev.device)
    out = [_unpack_strings(col, long_strings.get(c)) if k == STR else col for c, (k, col) in enumerate(zip(kinds, cols))]
    return out, lines


def _word_table(words):
    raw = [str(w).encode() for w in words]
    return (ctypes.c_char_p * len(raw))(*raw), len(raw)


def scan_sections(text, words):
    """``text``: uint8 tensor in HBM (mdh_scan_sections) or ``bytes`` (the host twin of the scan, mdh_debug_scan_sections — no
    device needed).  Returns ({word: byte offset of the first line whose first token is that word}, lines of the text); a word
    that starts no line is left out."""
    table, n = _word_table(words)
    first = np.full(max(n, 1), -1, dtype=np.int64)
    lines = ctypes.c_int64(0)
    if isinstance(text, (bytes, bytearray, memoryview)):
        raw = bytes(text)
        rc = _lib.lib().mdh_debug_scan_sections(raw, len(raw), table, n, first.ctypes.data, ctypes.addressof(lines))
    else:
        rc = _lib.lib().mdh_scan_sections(int(text.data_ptr()), int(text.numel()), _lib.DEVICE, table, n, first.ctypes.data,
                                          ctypes.addressof(lines), current_stream_ptr())
    _lib.check(rc)
    return {str(w): int(o) for w, o in zip(words, first) if o >= 0}, int(lines.value)


# ---------------------------------------------------------------------------------------------------------------------
# the output side (csrc/text_format.hip): typed columns in HBM -> the bytes of a text table, and those bytes -> a file
# ---------------------------------------------------------------------------------------------------------------------
F64, F32, I32, I64, CODED = 0, 1, 2, 3, 4
FORMAT_ROWS = 1 << 20  # rows formatted per call when a table is streamed to a file: what bounds the text held in HBM
_NP_OF = {F64: np.float64, F32: np.float32, I32: np.int32, I64: np.int64, CODED: np.int32}
_WIDEST = {F64: 32, F32: 32, I32: 11, I64: 20}  # bytes of the longest field of a kind (text_format.hpp)
_TYPICAL = {F64: 16, F32: 16, I32: 8, I64: 12}  # first guess of a capacity; a guess too small is answered with the need


class Unformattable(ValueError):
    """fields the device does not format (a finite |x| >= 2^64): the caller formats the whole table on the host"""

    def __init__(self, n):
        super().__init__(f"{n} fields need the host formatter")
        self.n = n


def check_names(names):
    """names of a coded-string column as the kernels copy them out: no quoting, so none may hold what a reader splits at"""
    out = [str(n) for n in names]
    for n in out:
        if any(ch in n for ch in " \t\"'\r\n"):
            raise ValueError(f"string value {n!r} holds a blank, a quote or a line break: it cannot be written without CSV quoting")
    return out


def _dev(col, kind):
    """the column as a contiguous 1-D torch tensor in HBM of the kind's dtype"""
    t = torch()
    want = np.dtype(_NP_OF[kind])
    if isinstance(col, HArray):
        col = col.dev()
    if isinstance(col, t.Tensor):
        if str(col.dtype).replace("torch.", "") != want.name or col.dim() != 1:
            raise TypeError(f"format_table: a column of kind {kind} must be a 1-D {want.name} array")
        return col.contiguous() if col.is_cuda else col.contiguous().cuda()
    a = np.asarray(col)
    if a.dtype != want or a.ndim != 1:
        raise TypeError(f"format_table: a column of kind {kind} must be a 1-D {want.name} array, got {a.dtype}")
    return HArray.from_numpy(a).dev()


def _prepare(columns, kinds, names):
    """(device tensors, kinds, checked names, bytes of the longest possible row); every code is checked against its table here,
    on the host, before anything is launched"""
    ncol = len(kinds)
    if ncol < 1 or len(columns) != ncol:
        raise ValueError("format_table: one kind per column, at least one column")
    if any(k not in _NP_OF for k in kinds):
        raise ValueError("format_table: column kind must be 0 (f64), 1 (f32), 2 (i32), 3 (i64) or 4 (coded string)")
    names = list(names) if names is not None else [None] * ncol
    tens = [_dev(c, k) for c, k in zip(columns, kinds)]
    nrows = int(tens[0].numel())
    if any(int(x.numel()) != nrows for x in tens):
        raise ValueError("format_table: columns differ in length")
    longest = ncol
    for c, k in enumerate(kinds):
        if k != CODED:
            longest += _WIDEST[k]
            continue
        if not names[c]:
            raise ValueError(f"format_table: column {c} is a coded string and needs its table of names")
        names[c] = check_names(names[c])
        longest += max(len(n.encode()) for n in names[c])
        if nrows:
            lo, hi = HArray(tens[c])._min_max_i32()
            if lo < 0 or hi >= len(names[c]):
                raise ValueError(f"format_table: column {c} holds code {lo if lo < 0 else hi}, outside its table of {len(names[c])} names")
    return tens, list(kinds), names, longest


def _format(tens, kinds, names, capacity=None, want_rows=False):
    """one mdh_format_table call over 1-D tensors of equal length (at least one row); the text, trimmed to its length"""
    t = torch()
    ncol, nrows = len(kinds), int(tens[0].numel())
    keep = []
    blobs = (ctypes.c_char_p * ncol)()
    offsets = (ctypes.c_void_p * ncol)()
    counts = np.zeros(ncol, dtype=np.int32)
    for c, k in enumerate(kinds):
        if k == CODED:
            raw = [n.encode() for n in names[c]]
            off = np.concatenate([[0], np.cumsum([len(b) for b in raw])]).astype(np.int32)
            blob = b"".join(raw) + b"\0"
            keep += [off, blob]
            blobs[c], offsets[c], counts[c] = blob, off.ctypes.data, len(raw)
    ptrs = (ctypes.c_void_p * ncol)(*[int(x.data_ptr()) for x in tens])
    kind_arr = np.asarray(kinds, dtype=np.int32)
    if capacity is None:
        per_row = ncol + sum(max(len(n.encode()) for n in names[c]) if k == CODED else _TYPICAL[k] for c, k in enumerate(kinds))
        capacity = nrows * per_row + 64
    row_end = t.empty(nrows, dtype=t.int64, device="cuda")
    status = np.zeros(3, dtype=np.int64)
    while True:
        text = t.empty(int(capacity), dtype=t.uint8, device="cuda")
        rc = _lib.lib().mdh_format_table(nrows, ncol, kind_arr.ctypes.data, ptrs, blobs, offsets, counts.ctypes.data, int(text.data_ptr()),
                                         int(capacity), int(row_end.data_ptr()), status.ctypes.data, _lib.DEVICE, current_stream_ptr())
        _lib.check(rc)
        total, bad, need = (int(v) for v in status)
        if bad:
            raise Unformattable(bad)
        if not need:
            return (text[:total], row_end) if want_rows else text[:total]
        capacity = need  # (the guess was too small: nothing was written, the exact size is known now)


def format_table(columns, kinds, names=None, capacity=None, want_rows=False):
    """``columns``: HArrays / ROCm tensors / numpy arrays of equal length, ``kinds[c]`` one of F64, F32, I32, I64, CODED,
    ``names[c]`` the strings a CODED column's int32 codes stand for.  Returns the table's text — fields joined by one blank,
    floats as ``format(v, ".10f")``, rows ended by a line feed — as one uint8 tensor in HBM (``want_rows``: and the int64 end
    offset of every row).  ``Unformattable`` when a field cannot be formatted on the device; ``ValueError`` for a code outside
    its table, a name that would need quoting, or a table too long for one call (``format_chunks`` takes any length)."""
    tens, kinds, names, _ = _prepare(columns, kinds, names)
    if not tens[0].numel():
        empty = torch().empty(0, dtype=torch().uint8, device="cuda")
        return (empty, torch().empty(0, dtype=torch().int64, device="cuda")) if want_rows else empty
    return _format(tens, kinds, names, capacity, want_rows)


def format_chunks(columns, kinds, names=None, rows=None):
    """the same text in pieces of ``rows`` rows (default FORMAT_ROWS; fewer when the 32-bit row offsets of one call demand it),
    each formatted when the consumer asks for it: the columns keep their full length in HBM, the text held there is a few pieces"""
    tens, kinds, names, longest = _prepare(columns, kinds, names)
    nrows = int(tens[0].numel())
    rows = max(1, min(int(FORMAT_ROWS if rows is None else rows), (2 ** 31 - 1) // longest))
    guess = None
    for a in range(0, nrows, rows):
        b = min(nrows, a + rows)
        text = _format([x[a:b] for x in tens], kinds, names, guess)
        guess = int(int(text.numel()) / (b - a) * rows * 1.02) + 64  # (rows of a table are much alike: the next piece fits, or asks once more)
        yield text


def stream_from_device(text, f, chunk=CHUNK):
    """write ``text`` — one uint8 tensor in HBM, or an iterable of them (``format_chunks``) — to the binary file object ``f``
    through two pinned buffers: a piece crosses PCIe while the one before it goes to the file, and the next piece of an iterable
    is asked for (formatted) while both are under way.  Returns the number of bytes written."""
    t = torch()
    pieces = [text] if isinstance(text, t.Tensor) else text
    pinned = [t.empty(int(chunk), dtype=t.uint8).pin_memory() for _ in range(2)]
    side = t.cuda.Stream()
    pending, k, total = None, 0, 0

    def drain(p):
        p[2].synchronize()  # the copy into this pinned buffer is done
        f.write(memoryview(pinned[p[0]].numpy())[: p[1]])

    for piece in pieces:
        n = int(piece.numel())
        ready = t.cuda.Event()
        ready.record(t.cuda.current_stream())  # what made the piece has been enqueued on the current stream
        piece.record_stream(side)  # (read under the side stream: its block is not handed out again before that is over)
        for at in range(0, n, int(chunk)):
            got = min(int(chunk), n - at)
            with t.cuda.stream(side):
                side.wait_event(ready)
                pinned[k][:got].copy_(piece[at:at + got], non_blocking=True)
                ev = t.cuda.Event()
                ev.record(side)
            if pending is not None:
                drain(pending)
            pending, k, total = (k, got, ev), k ^ 1, total + got
    if pending is not None:
        drain(pending)
    return total


_HOST_ROWS = 1 << 18


def _host_fields(col, kind, names):
    a = col.numpy() if hasattr(col, "numpy") and not isinstance(col, np.ndarray) else np.asarray(col)
    if kind == CODED:
        return np.asarray(names, dtype=object)[np.asarray(a)].tolist()
    if a.dtype.kind == "f":
        with np.errstate(invalid="ignore"):  # (a signalling NaN of a narrower type: still "NaN")
            wide = a.astype(np.float64)
        out = list(map("%.10f".__mod__, wide.tolist()))  # (exact and round-half-even, like format(v, ".10f"))
        if np.isnan(a).any():
            out = ["NaN" if s in ("nan", "-nan") else s for s in out]
        return out
    return list(map(str, a.tolist()))


def format_table_host(columns, kinds, names=None, f=None):
    """the host formatter, same contract and same bytes as the kernels' — for a machine without a GPU, for small tables, and for
    the whole of a table in which the device met a field it does not format (here every finite double is formatted).  Plain
    Python: I/O plumbing, not a compute path.  Columns are numpy arrays of any integer or float dtype.  Returns the bytes, or
    writes them to ``f`` piece by piece and returns their number."""
    ncol = len(kinds)
    names = list(names) if names is not None else [None] * ncol
    for c, k in enumerate(kinds):
        if k == CODED:
            names[c] = check_names(names[c])
            codes = np.asarray(columns[c])
            if codes.size and (codes.min() < 0 or codes.max() >= len(names[c])):
                raise ValueError(f"format_table: column {c} holds a code outside its table of {len(names[c])} names")
    nrows = len(columns[0]) if ncol else 0
    parts, total = [], 0
    for a in range(0, nrows, _HOST_ROWS):
        fields = [_host_fields(col[a:a + _HOST_ROWS], k, nm) for col, k, nm in zip(columns, kinds, names)]
        piece = ("\n".join(map(" ".join, zip(*fields))) + "\n").encode()
        total += len(piece)
        if f is None:
            parts.append(piece)
        else:
            f.write(piece)
    return b"".join(parts) if f is None else total


def shift_rotate(x, y, z, origin, matrix=None):
    """three new columns: positions minus ``origin``, then (``matrix`` given) times the 3x3 matrix, as
    ``((x - o0) m_0k + (y - o1) m_1k) + (z - o2) m_2k`` — in HBM (mdh_shift_rotate) when the columns are HArrays, in numpy with
    the same expression, hence the same bits, when they are numpy arrays"""
    o = np.ascontiguousarray(np.asarray(origin, dtype=np.float64).reshape(3))
    m = None if matrix is None else np.ascontiguousarray(np.asarray(matrix, dtype=np.float64).reshape(3, 3))
    if isinstance(x, HArray):
        n = len(x)
        out = [HArray.empty((n,), np.float64) for _ in range(3)]
        if n:
            _lib.check(_lib.lib().mdh_shift_rotate(x.data_ptr(), y.data_ptr(), z.data_ptr(), n, o.ctypes.data, None if m is None else m.ctypes.data,
                                                   out[0].data_ptr(), out[1].data_ptr(), out[2].data_ptr(), _lib.DEVICE, current_stream_ptr()))
        return out
    a, b, c = np.asarray(x) - o[0], np.asarray(y) - o[1], np.asarray(z) - o[2]
    if m is None:
        return [a, b, c]
    return [(a * m[0, k] + b * m[1, k]) + c * m[2, k] for k in range(3)]


_TOKEN_END = re.compile(rb"[ \t\r\n]")  # the kernel's blanks and the end of the row


def _long_token(text, off, nbytes):
    """the token that starts at byte ``off`` and is too long for the hand-back list's 16-bit length: all of it, up to the
    next blank, the end of the row or the end of the text, read in growing pieces"""
    got, want = b"", 1 << 17
    while True:
        got += text[off + len(got): min(off + want, nbytes)].cpu().numpy().tobytes()
        end = _TOKEN_END.search(got)
        if end or off + len(got) >= nbytes:
            return got[: end.start()] if end else got
        want *= 2


def _unpack_strings(packed, long_ones=None):
    """int64 of up to 8 little-endian characters -> numpy object array of str (unique codes decoded once)"""
    codes = packed.numpy()
    uniq, inv = np.unique(codes, return_inverse=True)
    names = np.array([int(u).to_bytes(8, "little", signed=True).rstrip(b"\0").decode() for u in uniq], dtype=object)
    out = names[inv]
    if long_ones:
        for r, tok in long_ones.items():
            out[r] = tok
    return out
