"""Times the LAMMPS data-file reader (mdapy_amd/load_save.py ``read_data``, _text.py, csrc/text.hip ``k_scan_sections``,
csrc/order.hip ``mdh_match_ids``); profiles/data_reader.md is written from what it prints.

The table is the bench's headline system — 10 061 824 atoms — written by the package's own formatter as
  * an atomic file (``id type x y z``),
  * a charge file with image flags (``id type q x y z ix iy iz``),
  * an atomic file with a Velocities section in shuffled order,
and as a dump with the atomic file's rows.  Measured for each data file, after a warm-up and repeated (min / median / max):
  * ``read_data`` end to end, and inside one such read its parts, each bracketed by a device synchronisation: the stream into
    HBM, the section scan, the Atoms table, the Velocities table, the id match, the three gathers;
  * the Atoms table tokenised as a view of the text tensor (it starts wherever the header ends) against an aligned copy of the
    same bytes, and the copy itself: what ``load_save.DATA_ALIGN_TABLES`` is set from;
  * ``read_dump`` on the same rows, and the host reader (once: it takes tens of seconds).

Usage: python tools/data_reader_bench.py [--atoms 10061824] [--repeats 5] [--no-host] [--out FILE.json]"""
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


def spread(samples):
    return {"min": min(samples), "median": statistics.median(samples), "max": max(samples), "n": len(samples)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--atoms", type=int, default=10_061_824)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--no-host", action="store_true")
    ap.add_argument("--out", default=None, help="also keep the result as JSON in this file")
    args = ap.parse_args()

    import torch

    import mdapy_amd.load_save as LS
    from mdapy_amd import _lib, _text, kernels
    from mdapy_amd.box import Box
    from mdapy_amd.devarray import HArray
    from mdapy_amd.frame import Column, Frame

    if _lib.device_count() < 1:
        raise SystemExit("data_reader_bench needs a HIP device")
    sync = torch.cuda.synchronize
    n = args.atoms
    rng = np.random.default_rng(0)
    edge = (n / 0.0847) ** (1.0 / 3.0)  # fcc copper's number density
    box = Box(np.diag([edge] * 3))
    host = {"id": np.arange(1, n + 1, dtype=np.int32), "type": rng.integers(1, 4, n).astype(np.int32), "q": rng.choice([-1.0, 0.0, 1.0], n)}
    host.update({c: rng.uniform(0, edge, n) for c in "xyz"})
    host.update({c: rng.integers(-2, 3, n).astype(np.int32) for c in ("ix", "iy", "iz")})
    host.update({c: rng.normal(0, 2.0, n) for c in ("vx", "vy", "vz")})
    frame = Frame({k: HArray.from_numpy(v) for k, v in host.items()})
    shuffle = HArray.from_numpy(rng.permutation(n).astype(np.int32))
    tmp = tempfile.mkdtemp(prefix="data_reader_bench_")
    paths = {k: os.path.join(tmp, k + (".dump" if k == "dump" else ".data")) for k in ("atomic", "atomic_no_elements", "charge_image", "atomic_velocities", "dump", "warm")}

    def head(op, style):
        op.write(f"# LAMMPS data file\n\n{n} atoms\n3 atom types\n\n0.0 {edge} xlo xhi\n0.0 {edge} ylo yhi\n0.0 {edge} zlo zhi\n\n".encode())
        op.write(f"Masses\n\n1 26.9815 # Al\n2 63.546 # Cu\n3 55.845 # Fe\n\nAtoms # {style}\n\n".encode())

    atomic = frame.select(["id", "type", "x", "y", "z"])
    LS.write_data(paths["atomic"], atomic, box, element_list=["Al", "Cu", "Fe"])
    LS.write_data(paths["atomic_no_elements"], atomic, box)
    LS.write_dump(paths["dump"], atomic, box, 0)
    with open(paths["charge_image"], "wb") as op:
        head(op, "charge")
        LS._write_table(op, [frame[c] for c in ("id", "type", "q", "x", "y", "z", "ix", "iy", "iz")])
    with open(paths["atomic_velocities"], "wb") as op:
        head(op, "atomic")
        LS._write_table(op, [frame[c] for c in ("id", "type", "x", "y", "z")])
        op.write(b"\nVelocities\n\n")
        LS._write_table(op, [Column(c, kernels.order.permute(frame[c].device_array(), shuffle)) for c in ("id", "vx", "vy", "vz")])
    small = Frame({k: HArray.from_numpy(v[: 1 << 18]) for k, v in host.items()})
    LS.write_data(paths["warm"], small.select(["id", "type", "x", "y", "z", "vx", "vy", "vz"]), box)
    del frame, atomic, small, shuffle
    LS.read_data(paths["warm"])
    kernels.order.permute(HArray.from_numpy(host["x"][:1000]), HArray.from_numpy(np.arange(1000, dtype=np.int32)[::-1].copy()))
    ids = HArray.from_numpy(host["id"][:1000])
    kernels.order.match_ids(ids, HArray.from_numpy(host["id"][:1000][::-1].copy()))
    del host

    out = {"atoms": n}
    parts = {}

    def timed(label, fn):
        def wrapper(*a, **k):
            sync()
            t = time.perf_counter()
            r = fn(*a, **k)
            sync()
            parts.setdefault(label, []).append(time.perf_counter() - t)
            return r
        return wrapper

    for name in ("atomic", "atomic_no_elements", "charge_image", "atomic_velocities"):
        path = paths[name]
        row = {"file_bytes": os.path.getsize(path)}
        whole = []
        for _ in range(args.repeats):
            sync()
            t = time.perf_counter()
            got = LS.read_data(path)
            sync()
            whole.append(time.perf_counter() - t)
            assert isinstance(got[0]["x"]._dev, HArray) and got[0].shape[0] == n
            del got
        row["read_data_s"] = spread(whole)
        # the parts, inside reads of their own (every part bracketed by a synchronisation, so their sum exceeds a plain read)
        real = (_text.stream_to_device, _text.scan_sections, _text.parse_table, kernels.order.match_ids, kernels.order.permute, LS._element_column)
        runs = []
        try:
            _text.stream_to_device, _text.scan_sections = timed("stream", real[0]), timed("scan", real[1])
            _text.parse_table = timed("table", real[2])
            kernels.order.match_ids, kernels.order.permute = timed("match", real[3]), timed("gather", real[4])
            LS._element_column = timed("element", real[5])
            for _ in range(args.repeats):
                parts.clear()
                LS.read_data(path)
                run = {"stream": parts["stream"][0], "scan": parts["scan"][0], "atoms_table": parts["table"][0]}
                if "element" in parts:
                    run["element_column"] = parts["element"][0]
                if len(parts["table"]) > 1:
                    run.update(velocities_table=parts["table"][1], match=sum(parts.get("match", [0.0])), gather=sum(parts.get("gather", [0.0])))
                runs.append(run)
        finally:
            _text.stream_to_device, _text.scan_sections, _text.parse_table, kernels.order.match_ids, kernels.order.permute, LS._element_column = real
        row["parts_s"] = {k: spread([r[k] for r in runs]) for k in runs[0]}
        # the Atoms table as a view of the text tensor against an aligned copy of it
        src = LS._DeviceText(path)
        found = src.sections()
        _, first, line = LS._first_data(src, found["Atoms"])
        end = min([o for o in found.values() if o > first] + [src.nbytes])
        ncol = len(line.split())
        names = ["id", "type"] + (["q"] if ncol in (6, 9) else []) + ["x", "y", "z"] + (["ix", "iy", "iz"] if ncol > 6 else [])
        kinds = [LS.INT if c in ("id", "type", "ix", "iy", "iz") else LS.FLOAT for c in names]
        view = src.text[first:end]
        ab = {"view": [], "aligned_copy": [], "copy": []}
        for rep in range(2 * args.repeats + 2):
            sync()
            t = time.perf_counter()
            text = view.clone() if rep & 1 else view
            sync()
            t1 = time.perf_counter()
            _text.parse_table(text, n, kinds)
            sync()
            if rep >= 2:
                ab["aligned_copy" if rep & 1 else "view"].append(time.perf_counter() - t1)
                if rep & 1:
                    ab["copy"].append(t1 - t)
            del text
        row["atoms_table_at"] = {"offset": first, "offset_mod_16": (int(src.text.data_ptr()) + first) % 16, "bytes": end - first}
        row["atoms_table_view_s"], row["atoms_table_aligned_copy_s"], row["copy_s"] = spread(ab["view"]), spread(ab["aligned_copy"]), spread(ab["copy"])
        del src, view
        if not args.no_host:
            LS.have_gpu = lambda: False
            try:
                t = time.perf_counter()
                LS.read_data(path)
                row["host_reader_s"] = time.perf_counter() - t
            finally:
                from mdapy_amd.devarray import have_gpu

                LS.have_gpu = have_gpu
        out[name] = row
        print(name, json.dumps(row), flush=True)

    dump = []
    for _ in range(args.repeats + 1):
        sync()
        t = time.perf_counter()
        got = LS.read_dump(paths["dump"])
        sync()
        dump.append(time.perf_counter() - t)
        del got
    out["read_dump_same_rows"] = {"file_bytes": os.path.getsize(paths["dump"]), "read_dump_s": spread(dump[1:])}
    for p in paths.values():
        os.remove(p)
    os.rmdir(tmp)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(out, f, indent=1)
    print(json.dumps(out, indent=1))


if __name__ == "__main__":
    main()
