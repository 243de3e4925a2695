"""The device formatter (csrc/text_format.hip: k_format_measure, the scan, k_format_write; text_format.hpp compiled for the
device) against the restatement in tests/_write_ref.py — ``format(v, ".10f")``, ``str(int)``, ``" ".join``.  Bytes, no tolerance.

``mdh_format_table`` is called directly on device columns.  The text buffer and the row ends start out filled with a sentinel,
so that what the kernels must not touch — everything beyond the table, and everything when the table cannot be written — is
checked as well."""
import ctypes

import numpy as np
import pytest

import _format_cases as V
import _write_ref as R

pytestmark = pytest.mark.gpu

F64, F32, I32, I64, CODED = 0, 1, 2, 3, 4
SENTINEL = 0xA5
NAMES = ["H", "Cu", "Unobtainium1"]  # 1, 2 and 12 bytes


@pytest.fixture(autouse=True)
def _need_gpu():
    from mdapy_amd import _lib

    if _lib.device_count() < 1:
        pytest.fail("test_gpu_text_format needs a HIP device")


def call(columns, kinds, names=None, nrows=None, capacity=None, slack=96, ncol=None, null_column=False):
    """mdh_format_table on device copies of ``columns``; (return code, the whole text buffer, row ends, status)"""
    import torch

    from mdapy_amd import _lib

    ncol = len(kinds) if ncol is None else ncol
    nrows = len(columns[0]) if nrows is None else nrows
    dev = [torch.from_numpy(np.ascontiguousarray(c)).cuda() for c in columns]
    ptrs = (ctypes.c_void_p * max(len(kinds), 1))(*[None if null_column else int(d.data_ptr()) for d in dev])
    blobs = (ctypes.c_char_p * max(len(kinds), 1))()
    offsets = (ctypes.c_void_p * max(len(kinds), 1))()
    counts = np.zeros(max(len(kinds), 1), np.int32)
    keep = []
    for c, k in enumerate(kinds):
        if k == CODED and names is not None and names[c] is not None:
            raw = [n.encode() for n in names[c]]
            off = np.concatenate([[0], np.cumsum([len(b) for b in raw])]).astype(np.int32)
            keep += [off, b"".join(raw)]
            blobs[c], offsets[c], counts[c] = keep[-1], off.ctypes.data, len(raw)
    if capacity is None:
        capacity = len(expected(columns, kinds, names)) + slack
    text = torch.full((max(capacity, 1) + 32,), SENTINEL, dtype=torch.uint8, device="cuda")
    ends = torch.full((max(nrows, 1),), -7, dtype=torch.int64, device="cuda")
    status = np.full(3, -1, np.int64)
    kind_arr = np.asarray(kinds if len(kinds) else [0], dtype=np.int32)
    rc = _lib.lib().mdh_format_table(nrows, ncol, kind_arr.ctypes.data, ptrs, blobs, offsets, counts.ctypes.data, int(text.data_ptr()), capacity,
                                     int(ends.data_ptr()), status.ctypes.data, _lib.DEVICE, None)
    torch.cuda.synchronize()
    return rc, text.cpu().numpy(), ends.cpu().numpy(), status


def expected(columns, kinds, names) -> bytes:
    return R.table([np.asarray(names[c], dtype=object)[col] if k == CODED else col for c, (col, k) in enumerate(zip(columns, kinds))])


def check_written(columns, kinds, names=None):
    want = expected(columns, kinds, names)
    rc, text, ends, status = call(columns, kinds, names)
    assert rc == 0
    assert status.tolist() == [len(want), 0, 0]
    assert text[: len(want)].tobytes() == want
    assert (text[len(want):] == SENTINEL).all()  # not a byte beyond the table
    line_ends = np.flatnonzero(np.frombuffer(want, np.uint8) == 10) + 1
    assert np.array_equal(ends, line_ends)
    return want


def wide_column(n, rng):
    return np.array([0.5, -123456789.25, 1.8e19])[rng.integers(0, 3, n)]


def twelve_columns(n, rng):
    cols = [wide_column(n, rng), rng.uniform(-200, 200, n), rng.standard_normal(n) * 1e-9, rng.standard_normal(n).astype(np.float32),
            (rng.standard_normal(n) * 1e15).astype(np.float32), rng.integers(-99, 100, n).astype(np.int32),
            rng.integers(-2 ** 31, 2 ** 31, n).astype(np.int32), rng.integers(-2 ** 63, 2 ** 63 - 1, n, dtype=np.int64),
            rng.integers(0, 10, n).astype(np.int64), rng.integers(0, 3, n).astype(np.int32), np.full(n, 2, np.int32),
            (np.arange(n) % 3).astype(np.int32)]
    kinds = [F64, F64, F64, F32, F32, I32, I32, I64, I64, CODED, CODED, CODED]
    names = [None] * 9 + [NAMES, NAMES, NAMES[::-1]]
    return cols, kinds, names


@pytest.mark.parametrize("nrows", [1, 63, 64, 65, 257, 4097])
def test_one_column(nrows):
    rng = np.random.default_rng(nrows)
    check_written([wide_column(nrows, rng)], [F64])  # (rows of 13, 24 and 32 bytes: a workgroup's span fits its LDS image)


@pytest.mark.parametrize("nrows", [1, 63, 64, 65, 257, 4097])
def test_twelve_columns_every_kind(nrows):
    rng = np.random.default_rng(100 + nrows)
    cols, kinds, names = twelve_columns(nrows, rng)
    want = check_written(cols, kinds, names)
    if nrows >= 257:  # (256 rows of these are more than the 32 KB image holds: the fields go straight to HBM)
        assert want.index(b"\n", 0) > 0 and len(want) / nrows > 140


def test_capacity_exact_and_one_byte_short():
    rng = np.random.default_rng(7)
    cols, kinds, names = twelve_columns(4097, rng)
    want = expected(cols, kinds, names)
    rc, text, ends, status = call(cols, kinds, names, capacity=len(want))
    assert rc == 0 and status.tolist() == [len(want), 0, 0] and text[: len(want)].tobytes() == want and (text[len(want):] == SENTINEL).all()
    rc, text, ends, status = call(cols, kinds, names, capacity=len(want) - 1)
    assert rc == 0 and status.tolist() == [len(want), 0, len(want)]
    assert (text == SENTINEL).all() and (ends == -7).all()  # nothing is written


def test_one_unformattable_value_stops_everything():
    rng = np.random.default_rng(8)
    cols, kinds, names = twelve_columns(4097, rng)
    cols[1][2345] = 1e30
    rc, text, ends, status = call(cols, kinds, names, capacity=4097 * 400)
    assert rc == 0 and status[1] == 1 and status[2] == 0
    assert (text == SENTINEL).all() and (ends == -7).all()
    cols[9][17] = 3  # a code outside its table is not formattable either (and is never used as an index)
    cols[10][4000] = -1
    rc, text, ends, status = call(cols, kinds, names, capacity=4097 * 400)
    assert rc == 0 and status[1] == 3 and (text == SENTINEL).all()


def test_value_classes_through_the_kernel():
    """the device compilation of text_format.hpp agrees with format() on everything the host compilation is pinned on"""
    vals = np.concatenate([V.value_classes(), np.array([np.nan, np.inf, -np.inf])])
    want = check_written([vals], [F64])
    assert want.count(b"\n") == len(vals) >= 220_000
    f32 = np.concatenate([np.random.default_rng(13).integers(0, 2 ** 32, 50_000, dtype=np.uint64).astype(np.uint32).view(np.float32),
                          np.array([1e-45, -1e-45, 1.1754942e-38, 1e-40, 0.1, -0.0, 16777217.0, 1.8e19], np.float32)])
    f32 = f32[~(np.isfinite(f32) & (np.abs(f32) >= np.float32(2.0 ** 64)))]  # (what is refused has its own test)
    check_written([f32], [F32])
    ints = np.array(V.int_classes(), dtype=np.int64)
    check_written([ints], [I64])
    small = ints[(ints >= -2 ** 31) & (ints < 2 ** 31)].astype(np.int32)
    check_written([small, ints[: len(small)]], [I32, I64])


def test_argument_errors_before_any_device_work():
    from mdapy_amd import _lib

    col = [np.zeros(4)]
    for kwargs in (dict(nrows=0), dict(nrows=-1), dict(ncol=0), dict(ncol=65), dict(null_column=True)):
        rc, text, ends, status = call(col, [F64], capacity=64, **kwargs)
        assert rc == _lib.ERR_ARG and (text == SENTINEL).all()
    for kinds in ([5], [-1]):
        rc, text, ends, status = call(col, kinds, capacity=64)
        assert rc == _lib.ERR_ARG and (text == SENTINEL).all()
    rc, text, ends, status = call([np.zeros(4, np.int32)], [CODED], names=None, capacity=64)  # a coded column without its names
    assert rc == _lib.ERR_ARG
    with pytest.raises(ValueError, match="mdh_format_table"):
        _lib.check(rc)


def test_python_shim():
    from mdapy_amd import _text
    from mdapy_amd.devarray import HArray

    rng = np.random.default_rng(9)
    cols, kinds, names = twelve_columns(1000, rng)
    text, ends = _text.format_table([HArray.from_numpy(c) for c in cols], kinds, names, want_rows=True)
    want = expected(cols, kinds, names)
    assert text.cpu().numpy().tobytes() == want and int(ends[-1]) == len(want)
    assert b"".join(t.cpu().numpy().tobytes() for t in _text.format_chunks(cols, kinds, names, rows=333)) == want
    bad = [c.copy() for c in cols]
    bad[11][5] = 3
    with pytest.raises(ValueError, match="column 11 holds code 3, outside its table of 3 names"):
        _text.format_table(bad, kinds, names)
    bad = [c.copy() for c in cols]
    bad[0][999] = -1e300
    with pytest.raises(_text.Unformattable):
        _text.format_table(bad, kinds, names)
    with pytest.raises(ValueError, match="blank, a quote or a line break"):
        _text.format_table(cols, kinds, [None] * 9 + [NAMES, NAMES, ["a b", "c", "d"]])
