"""Times the Lindemann index (mdapy_amd/_lindemann.py) on random-walk trajectories resident in HBM: F = 200 frames of N = 1000,
4000 and 16000 atoms.  One JSON line per figure:

  isa        VALU instructions of one pass of each kernel's frame loop, from the ISA hipcc emits for csrc/lindemann.hip, and per
             pair-frame (a thread's pass covers 16 pairs); needs no device
  global     compute_global (no tables): N (N - 1) / 2 pairs x F frames
  all        compute_all (no tables, the library's choice of segments): N^2 ordered pairs x F frames, diagonal included — what
             the kernel computes; the reference's serial loop does half of that and stores it twice
  segments   compute_all with the segment count forced, at every N
  numpy      the restatement of tests/_lindemann_ref.py at N = 1000, on the host (the only CPU yardstick a machine without the
             reference's binary has); its fsum sums are part of it

Medians of --calls calls after a warm-up call, best and worst beside them; every timed call ends in a device synchronise.

Usage: python tools/lindemann_bench.py [--frames 200] [--atoms 1000 4000 16000] [--calls 5] [--isa-only] [--no-numpy]"""
import argparse
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
TILE, MICRO = 64, 4


def isa_counts():
    """{kernel: VALU instructions in the innermost loop that takes the 16 square roots of a thread's micro-tile}"""
    src = os.path.join(ROOT, "mdapy_amd", "csrc", "lindemann.hip")
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    with tempfile.TemporaryDirectory() as tmp:
        out = os.path.join(tmp, "lindemann.s")
        subprocess.check_call([hipcc, "-O3", "-std=c++17", "--offload-arch=gfx950", "-ffp-contract=off", "--cuda-device-only", "-S",
                               src, "-o", out], stderr=subprocess.DEVNULL)
        lines = open(out).read().splitlines()
    found = {}
    starts = [(k, m.group(1)) for k, line in enumerate(lines) for m in [re.match(r"^(_ZN3mdh\w+):", line)] if m]
    for (begin, name), end in zip(starts, [k for k, _ in starts[1:]] + [len(lines)]):
        body = lines[begin:end]
        labels = {m.group(1): k for k, line in enumerate(body) for m in [re.match(r"^(\.LBB\w+):", line)] if m}
        best = None
        for k, line in enumerate(body):
            m = re.match(r"\s+s_cbranch_\w+ (\.LBB\w+)", line) or re.match(r"\s+s_branch (\.LBB\w+)", line)
            if m and labels.get(m.group(1), k) < k:  # a backward branch closes a loop
                loop = body[labels[m.group(1)]:k]
                roots = sum("v_rsq_f64" in x for x in loop)
                if roots >= MICRO * MICRO and (best is None or len(loop) < len(best)):
                    best = loop
        if best is not None:
            valu = sum(bool(re.match(r"\s+v_", x)) for x in best)
            short = re.sub(r"^_ZN3mdh\d+", "", name).split("E")[0]
            found[short] = {"valu_per_pass": valu, "valu_per_pair_frame": valu / (MICRO * MICRO),
                            "roots": sum("v_rsq_f64" in x for x in best), "reciprocals": sum("v_rcp_f64" in x for x in best)}
    return found


def main():
    p = argparse.ArgumentParser()
    p.add_argument("--frames", type=int, default=200)
    p.add_argument("--atoms", type=int, nargs="+", default=[1000, 4000, 16000])
    p.add_argument("--calls", type=int, default=5)
    p.add_argument("--isa-only", action="store_true")
    p.add_argument("--no-numpy", action="store_true")
    args = p.parse_args()
    print(json.dumps({"isa": isa_counts()}), flush=True)
    if args.isa_only:
        return
    import torch

    from mdapy_amd import _lindemann
    from mdapy_amd.devarray import HArray

    if not torch.cuda.is_available():
        raise RuntimeError("lindemann_bench needs a HIP device")

    def timed(fn):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        return time.perf_counter() - t0

    def laps(fn, pair_frames):
        fn()  # warm-up
        s = [timed(fn) for _ in range(max(args.calls, 1))]
        return {"ms": 1e3 * float(np.median(s)), "ms_best": 1e3 * float(np.min(s)), "ms_worst": 1e3 * float(np.max(s)), "calls": len(s),
                "pair_frames": pair_frames, "pair_frames_per_s": pair_frames / float(np.median(s))}

    F = args.frames
    for N in args.atoms:
        rng = np.random.default_rng(N)
        host = np.cumsum(rng.choice([-1.0, 0.0, 1.0], size=(F, N, 3)), axis=0)
        pos = HArray.from_numpy(host)
        frame, atom = HArray.empty(F, np.float64), HArray.empty((F, N), np.float64)
        blocks = -(-N // TILE)
        value = {}
        out = laps(lambda: value.update(v=_lindemann.compute_global(pos, None, None, 1)), N * (N - 1) // 2 * F)
        print(json.dumps({"mode": "global", "N": N, "F": F, "tiles": blocks * (blocks + 1) // 2, "value": value["v"], **out}), flush=True)
        out = laps(lambda: _lindemann.compute_all(pos, None, None, frame, atom), N * N * F)
        last = float(np.asarray(frame)[-1])
        print(json.dumps({"mode": "all", "N": N, "F": F, "i_blocks": blocks, "segments": "library", "last_frame": last, **out}), flush=True)
        for segments in (1, 2, 4, 8, 16, 32):
            if segments > blocks:
                break
            out = laps(lambda: _lindemann.compute_all(pos, None, None, frame, atom, segments=segments), N * N * F)
            print(json.dumps({"mode": "all", "N": N, "F": F, "i_blocks": blocks, "segments": segments, **out}), flush=True)
        if N == 1000 and not args.no_numpy:
            sys.path.insert(0, os.path.join(ROOT, "tests"))
            import _lindemann_ref

            t0 = time.perf_counter()
            want = _lindemann_ref.restate(host)
            s = time.perf_counter() - t0
            print(json.dumps({"mode": "numpy restatement (both modes in one pass, host)", "N": N, "F": F, "ms": 1e3 * s, "value": want.trj,
                              "last_frame": float(want.frame[-1])}), flush=True)


if __name__ == "__main__":
    main()
