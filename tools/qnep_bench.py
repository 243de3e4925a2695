"""Times the charge-aware NEP calculator (QNEP) on the first water frame of tests/golden/qnep/train.xyz.gz (384 atoms, 15.36 A) replicated
2, 4 and 6 times per axis — 3 072, 24 576 and 82 944 atoms — under the two fixture models (mode 1: Ewald, mode 2: k-space alone).
One JSON line per figure:

  resources  VGPRs / LDS / scratch of the kernels of csrc/nep_charge.hip and csrc/nep.hip (hipcc -Rpass-analysis=kernel-resource-usage); --isa-only
             stops here
  case       per size and mode: the whole call of the raw shim on the list in HBM (median, best, worst of --calls after a warm-up),
             its passes' own times from the library's event pairs (mdh_prof_*; k_nep_pair runs twice a call, once for the forces and
             once for the BEC: its figure is the mean of the two), the number of k-points and the (atom, k-point) terms per second of
             the two k-space kernels

--write replaces the block between the two qnep_bench marks of profiles/qnep.md with a table of what was measured.

Usage: python tools/qnep_bench.py [--repeats 2 4 6] [--calls 3] [--isa-only] [--write]"""
import argparse
import ctypes
import json
import os
import re
import subprocess
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
GOLDEN = os.path.join(ROOT, "tests", "golden", "qnep")
BEGIN, END = "<!-- qnep_bench:begin -->", "<!-- qnep_bench:end -->"


def resources():
    """both units: csrc/nep.hip holds the shared kernels (their charge instantiations carry a 1 as the last template argument)"""
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    keys = {"VGPRs": "vgprs", "ScratchSize [bytes/lane]": "scratch_bytes_per_lane", "Occupancy [waves/SIMD]": "waves_per_simd",
            "LDS Size [bytes/block]": "lds_bytes"}
    table, name = {}, None
    for unit in ("nep_charge", "nep"):
        src = os.path.join(ROOT, "mdapy_amd", "csrc", unit + ".hip")
        with tempfile.TemporaryDirectory() as tmp:
            done = subprocess.run([hipcc, "-O3", "-std=c++17", "--offload-arch=gfx950", "-ffp-contract=off", "--cuda-device-only", "-c",
                                   "-Rpass-analysis=kernel-resource-usage", src, "-o", os.path.join(tmp, unit + ".o")],
                                  stderr=subprocess.PIPE, text=True, check=True)
        for line in done.stderr.splitlines():
            m = re.search(r"remark:\s+(.*?):\s+(\S+) \[-Rpass", line)
            if not m:
                continue
            if m.group(1) == "Function Name":
                marks = re.findall(r"L[ib](\d+)E", m.group(2))
                name = re.sub(r"^_ZN3mdhL?\d+(k_\w+?)(I|E).*$", r"\1", m.group(2)) + (f"<{', '.join(marks)}>" if marks else "")
                if unit == "nep" and (not marks or marks[-1] != "1"):
                    name = None  # (the charge-free instantiations: tools/nep_bench.py)
                else:
                    table[name] = {}
            elif name and m.group(1) in keys:
                table[name][keys[m.group(1)]] = int(m.group(2))
    return table


def table_of(res, cases):
    lines = ["Kernel resources (template arguments: lanes per atom, triclinic, charge / add / first):", "",
             "| kernel | VGPRs | scratch B/lane | waves/SIMD | LDS B/block |", "|---|---|---|---|---|"]
    for name, r in res.items():
        lines.append(f"| `{name}` | {r.get('vgprs')} | {r.get('scratch_bytes_per_lane')} | {r.get('waves_per_simd')} | {r.get('lds_bytes')} |")
    passes = ["k_nep_descriptor", "k_nepq_sfactor", "k_nepq_atoms", "k_nepq_real", "k_nep_pair", "k_nep_gather", "k_nepq_bec"]
    lines += ["", "Per-pass times in ms (the whole call: median of the laps):", "",
              "| atoms | mode | k-points | call | " + " | ".join(p[2:] for p in passes) + " | sfactor terms/s | atoms terms/s |",
              "|---|---|---|---|" + "---|" * (len(passes) + 2)]
    for c in cases:
        ms = c["kernel_ms"]
        lines.append(f"| {c['atoms']} | {c['mode']} | {c['kpoints']} | {c['call']['ms']:.2f} | "
                     + " | ".join(f"{ms[p]:.3f}" if p in ms else "-" for p in passes)
                     + f" | {c['terms_per_s'].get('k_nepq_sfactor', 0):.3g} | {c['terms_per_s'].get('k_nepq_atoms', 0):.3g} |")
    return "\n".join(lines)


def main():
    p = argparse.ArgumentParser()
    p.add_argument("--repeats", type=int, nargs="+", default=[2, 4, 6])
    p.add_argument("--calls", type=int, default=3)
    p.add_argument("--isa-only", action="store_true")
    p.add_argument("--write", action="store_true")
    args = p.parse_args()
    res = resources()
    print(json.dumps({"resources": res}), flush=True)
    if args.isa_only:
        return
    import torch

    import mdapy_amd as mp
    from mdapy_amd import _lib, kernels
    from mdapy_amd.devarray import HArray

    if not torch.cuda.is_available():
        raise RuntimeError("qnep_bench needs a HIP device")
    L = _lib.lib()
    frame = mp.Trajectory(os.path.join(GOLDEN, "train.xyz.gz"), verbose=False)[0]
    pos0 = frame.data.select("x", "y", "z").to_numpy()
    names0 = np.asarray(frame.data["element"].to_numpy()).astype(str)
    cell0 = np.array(frame.box.box, float)
    up = lambda a: HArray(torch.from_numpy(np.ascontiguousarray(a)).cuda())

    def timed(fn):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        return 1e3 * (time.perf_counter() - t0)

    def kernel_times(fn):
        torch.cuda.synchronize()
        L.mdh_prof_reset()
        L.mdh_prof_enable(1)
        fn()
        torch.cuda.synchronize()
        L.mdh_prof_enable(0)
        buf = ctypes.create_string_buffer(1 << 16)
        L.mdh_prof_report(buf, len(buf))
        out = {}
        for line in buf.value.decode().strip().splitlines():
            name, count, total = line.split()
            out[name] = float(total) / int(count)
        return out

    cases = []
    for r in args.repeats:
        shifts = np.array([(i, j, k) for i in range(r) for j in range(r) for k in range(r)], float) @ cell0
        pos = (pos0[None, :, :] + shifts[:, None, :]).reshape(-1, 3)
        names, cell, n = np.tile(names0, r ** 3), cell0 * r, len(pos0) * r ** 3
        for mode in (1, 2):
            calc = mp.QNEP(os.path.join(GOLDEN, f"nep_mode{mode}.txt.gz"))
            s = mp.System(pos=pos, box=mp.Box(cell))
            s.set_element(names)
            s.build_neighbor(calc.rc)
            types = up(np.array([calc.element_list.index(e) for e in names], np.int32))
            cols = [up(pos[:, k]) for k in range(3)]
            model = calc._model((0, 1))
            out = {name: HArray.empty(shape, np.float64) for name, shape in
                   (("energy", (n,)), ("force", (n, 3)), ("virial", (n, 9)), ("virial_sum", (9,)), ("charge", (n,)), ("bec", (n, 9)))}
            raw = lambda: kernels.nep.calculate_charge(*cols, types, np.arange(2, dtype=np.int32), cell, np.zeros(3), np.ones(3, np.int32),
                                                       s.verlet_list, s.distance_list, s.neighbor_number, model, cell, calc.rc, n_real=n, **out)
            raw()  # warm-up
            ms = [timed(raw) for _ in range(max(args.calls, 1))]
            kms = kernel_times(raw)
            alpha = np.pi / calc.rc
            b = 2.0 * np.pi * np.linalg.inv(cell).T
            top = [int(alpha * np.linalg.norm(cell[i])) for i in range(3)]
            grid = np.stack(np.meshgrid(np.arange(0, top[0] + 1), np.arange(-top[1], top[1] + 1), np.arange(-top[2], top[2] + 1),
                                        indexing="ij"), -1).reshape(-1, 3)
            half = (grid[:, 0] > 0) | ((grid[:, 0] == 0) & (grid[:, 1] > 0)) | ((grid[:, 0] == 0) & (grid[:, 1] == 0) & (grid[:, 2] > 0))
            nk = int((((grid[half] @ b) ** 2).sum(1) < (2.0 * np.pi * alpha) ** 2).sum())
            case = {"atoms": n, "mode": mode, "kpoints": nk, "row_width": int(s.verlet_list.shape[1]),
                    "call": {"ms": float(np.median(ms)), "ms_best": float(np.min(ms)), "ms_worst": float(np.max(ms)), "calls": len(ms)},
                    "kernel_ms": kms, "max_abs_charge": float(np.abs(out["charge"].numpy()).max())}
            case["terms_per_s"] = {k: n * nk / (kms[k] * 1e-3) for k in ("k_nepq_sfactor", "k_nepq_atoms") if k in kms}
            cases.append(case)
            print(json.dumps(case), flush=True)
            del s, out, cols, types
    if args.write:
        path = os.path.join(ROOT, "profiles", "qnep.md")
        text = open(path).read() if os.path.exists(path) else f"# QNEP\n\n{BEGIN}\n{END}\n"
        head, rest = text.split(BEGIN, 1)
        tail = rest.split(END, 1)[1]
        with open(path, "w") as f:
            f.write(head + BEGIN + "\n" + table_of(res, cases) + "\n" + END + tail)


if __name__ == "__main__":
    main()
