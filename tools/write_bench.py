"""Times the output side (mdapy_amd/load_save.py writers, _text.py, csrc/text_format.hip); profiles/text_format.md is written
from what it prints.

The table is the bench's headline system — 10 061 824 atoms, columns ``id type x y z`` plus one int label — in HBM.  Measured,
each after a warm-up and repeated (min / median / max are printed):
  * ``write_dump`` to a file on local disk, end to end;
  * its parts on their own: formatting all pieces (no copy), copying the text down through the pinned buffers (no file), writing
    the bytes to the file (no GPU);
  * one piece of 2^20 rows formatted with the workgroup's span built in LDS and with every field stored straight to HBM,
    alternating (``mdh_debug_set_format_variant``);
  * host formatter against device path for small tables (columns on the host, as a System built from arrays has them): the row
    count where the device path starts to win sets ``load_save.DEVICE_MIN_ROWS``;
  * the tests' plain-Python restatement on 10^6 rows, scaled to the whole table: what a user without these writers faces.
Kernel times come from a separate ``rocprofv3 --kernel-trace --stats -- python tools/write_bench.py --only-write`` run.

Usage: python tools/write_bench.py [--atoms 10061824] [--repeats 5] [--out FILE.json] [--only-write]"""
import argparse
import json
import os
import statistics
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))


def spread(samples):
    return {"min": min(samples), "median": statistics.median(samples), "max": max(samples), "n": len(samples)}


def table(n, seed=0):
    rng = np.random.default_rng(seed)
    edge = (n / 0.0847) ** (1.0 / 3.0)  # fcc copper's number density
    return {"id": np.arange(1, n + 1, dtype=np.int32), "type": rng.integers(1, 4, n).astype(np.int32), "x": rng.uniform(0, edge, n),
            "y": rng.uniform(0, edge, n), "z": rng.uniform(0, edge, n), "cna": rng.integers(0, 5, n).astype(np.int32)}, edge


class Null:
    def write(self, b):
        return len(b)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--atoms", type=int, default=10_061_824)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--out", default=None, help="also keep the result as JSON in this file")
    ap.add_argument("--only-write", action="store_true")
    args = ap.parse_args()

    import torch

    import mdapy_amd.load_save as LS
    from mdapy_amd import _lib, _text
    from mdapy_amd.box import Box
    from mdapy_amd.devarray import HArray
    from mdapy_amd.frame import Frame

    if _lib.device_count() < 1:
        raise SystemExit("write_bench needs a HIP device")
    sync = torch.cuda.synchronize
    cols, edge = table(args.atoms)
    frame = Frame({k: HArray.from_numpy(v) for k, v in cols.items()})
    box = Box(np.diag([edge] * 3))
    tmp = tempfile.mkdtemp(prefix="write_bench_")
    path = os.path.join(tmp, "big.dump")
    warm = Frame({k: HArray.from_numpy(v[: 1 << 20]) for k, v in cols.items()})
    LS.write_dump(path, warm, box, 0)
    out = {"atoms": args.atoms}

    whole = []
    for _ in range(1 if args.only_write else args.repeats):
        sync()
        t = time.perf_counter()
        LS.write_dump(path, frame, box, 0)
        whole.append(time.perf_counter() - t)
    out["file_bytes"] = os.path.getsize(path)
    out["write_dump_s"] = spread(whole)
    if args.only_write:
        print(json.dumps(out))
        return

    specs = [LS._column_spec(frame[c], True) for c in frame.columns]
    a, k, nm = [s[0] for s in specs], [s[1] for s in specs], [s[2] for s in specs]
    fmt, down, disk = [], [], []
    pieces = None
    for _ in range(args.repeats):
        sync()
        t = time.perf_counter()
        pieces = list(_text.format_chunks(a, k, nm))
        sync()
        fmt.append(time.perf_counter() - t)
    for _ in range(args.repeats):
        sync()
        t = time.perf_counter()
        _text.stream_from_device(pieces, Null())
        down.append(time.perf_counter() - t)
    host = b"".join(p.cpu().numpy().tobytes() for p in pieces)
    text_bytes = len(host)
    del pieces
    for _ in range(args.repeats):
        t = time.perf_counter()
        with open(path, "wb") as f:
            f.write(host)
        disk.append(time.perf_counter() - t)
    del host
    out.update(text_bytes=text_bytes, format_all_pieces_s=spread(fmt), copy_down_s=spread(down), file_write_s=spread(disk),
               format_GBps=text_bytes / statistics.median(fmt) / 1e9, copy_down_GBps=text_bytes / statistics.median(down) / 1e9,
               file_write_GBps=text_bytes / statistics.median(disk) / 1e9)

    # the two ways to place the bytes, alternating, on one piece of 2^20 rows
    tens, kinds, names, _ = _text._prepare([x.dev()[: 1 << 20] for x in a], k, nm)
    ab = {0: [], 1: []}
    for rep in range(2 * args.repeats + 2):
        v = rep & 1
        _lib.check(_lib.lib().mdh_debug_set_format_variant(v))
        sync()
        t = time.perf_counter()
        _text._format(tens, kinds, names)
        sync()
        if rep >= 2:
            ab[v].append(time.perf_counter() - t)
    _lib.check(_lib.lib().mdh_debug_set_format_variant(0))
    out["piece_2p20_rows_lds_image_s"] = spread(ab[0])
    out["piece_2p20_rows_straight_to_hbm_s"] = spread(ab[1])

    # host formatter against device path, small tables with their columns on the host
    cross = []
    for n in (1 << 10, 1 << 12, 1 << 14, 1 << 15, 1 << 16, 1 << 17, 1 << 18, 1 << 20):
        small, e = table(n, seed=n)
        b = Box(np.diag([e] * 3))
        row = {"rows": n}
        for label, rows in (("host_s", 1 << 62), ("device_s", 0)):
            LS.DEVICE_MIN_ROWS = rows
            got = []
            for rep in range(args.repeats + 1):
                fr = Frame(small)  # (a new frame: no HBM mirror from the last repeat)
                sync()
                t = time.perf_counter()
                LS.write_dump(path, fr, b, 0)
                if rep:
                    got.append(time.perf_counter() - t)
            row[label] = spread(got)
        cross.append(row)
    out["host_against_device"] = cross

    import _write_ref as R

    million, e = table(1_000_000, seed=5)
    t = time.perf_counter()
    R.dump(million, Box(np.diag([e] * 3)), 0)
    one = time.perf_counter() - t
    out["restatement_1e6_rows_s"] = one
    out["restatement_scaled_s"] = one * args.atoms / 1e6

    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(out, f, indent=1)
    print(json.dumps(out, indent=1))


if __name__ == "__main__":
    main()
