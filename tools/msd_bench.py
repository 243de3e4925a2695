"""Times the mean squared displacement (mdapy_amd/_msd.py) on lattice-walk trajectories resident in HBM, at (frames, atoms) =
(200, 1000), (200, 16 000), (200, 1 000 000), (2000, 16 000) and (10 000, 4000).  One JSON line per figure:

  isa        VALU instructions of one pass of the window kernel's unrolled chunk (64 pair-frames per lane: 8 time origins x 8
             lags), from the ISA hipcc emits for csrc/msd.hip, and per pair-frame; needs no device
  window     window mode with the table: N F (F + 1) / 2 pair-frames (a pair-frame is one term |r[t+m, i] - r[t, i]|^2)
  window_msd window mode, ``msd`` only
  direct     direct mode with the table: N F terms, F N 32 bytes moved
  direct_msd direct mode, ``msd`` only (F N 24 bytes read): with ``window_msd`` an upper bound on what k_msd_rows, the second
             kernel of every call that wants ``msd``, can cost
  fft        the S1 - 2 S2 formula with numpy's double FFT on the host (tests/_msd_ref.py fft_window), at the shapes of --fft (the yardstick a machine without
             the reference's optional pyfftw has); it is not a result anybody should use (it cancels), only a time

Medians of --calls calls after a warm-up call, best and worst beside them; every timed call ends in a device synchronise.

Usage: python tools/msd_bench.py [--shapes 200x1000 ...] [--calls 5] [--isa-only] [--fft 200x1000 2000x16000]"""
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
CHUNK, LAGS = 8, 8  # csrc/msd.hip MSD_C, MSD_LW: terms per lane in one pass of the unrolled chunk
SHAPES = ["200x1000", "200x16000", "200x1000000", "2000x16000", "10000x4000"]
RATE = 39.3e12  # f64 VALU lane-operations per second (profiles/lindemann.md)


def isa_counts():
    """the basic block of k_msd_window with the most f64 adds — the unchecked chunk — and what it holds"""
    src = os.path.join(ROOT, "mdapy_amd", "csrc", "msd.hip")
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    with tempfile.TemporaryDirectory() as tmp:
        out = os.path.join(tmp, "msd.s")
        subprocess.check_call([hipcc, "-O3", "-std=c++17", "--offload-arch=gfx950", "-ffp-contract=off", "--cuda-device-only", "-S",
                               src, "-o", out], stderr=subprocess.DEVNULL)
        lines = open(out).read().splitlines()
    begin = next(k for k, line in enumerate(lines) if re.match(r"^_ZN3mdh\d+k_msd_window\w*:", line))
    end = next(k for k in range(begin, len(lines)) if lines[k].startswith(".Lfunc_end"))
    blocks, current = [], []
    for line in lines[begin:end]:
        if re.match(r"^\.LBB\w+:", line) or re.match(r"\s+s_c?branch", line):
            blocks.append(current)
            current = []
        elif re.match(r"\s+[a-z]", line):
            current.append(line.split()[0])
    blocks.append(current)
    best = max(blocks, key=lambda b: sum(op == "v_add_f64" for op in b))
    valu = sum(op.startswith("v_") for op in best)
    terms = CHUNK * LAGS
    return {"k_msd_window": {"valu_per_pass": valu, "valu_per_pair_frame": valu / terms, "v_add_f64": sum(op == "v_add_f64" for op in best),
                             "v_mul_f64": sum(op == "v_mul_f64" for op in best), "v_fma_f64": sum(op == "v_fma_f64" for op in best),
                             "lds_reads": sum(op.startswith("ds_read") for op in best), "instructions": len(best),
                             "pair_frames_per_s_at_the_vector_rate": RATE / (valu / terms)}}


def shape(text):
    F, N = text.lower().split("x")
    return int(F), int(N)


def main():
    p = argparse.ArgumentParser()
    p.add_argument("--shapes", nargs="+", default=SHAPES)
    p.add_argument("--fft", nargs="*", default=["200x1000", "2000x16000"])
    p.add_argument("--calls", type=int, default=5)
    p.add_argument("--isa-only", action="store_true")
    args = p.parse_args()
    print(json.dumps({"isa": isa_counts()}), flush=True)
    if args.isa_only:
        return
    import torch

    from mdapy_amd import _msd
    from mdapy_amd.devarray import HArray

    if not torch.cuda.is_available():
        raise RuntimeError("msd_bench needs a HIP device")

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

    for F, N in [shape(s) for s in args.shapes]:
        gen = torch.Generator(device="cuda").manual_seed(1000 * F + N)
        steps = torch.randint(-1, 2, (F, N, 3), generator=gen, device="cuda", dtype=torch.int8)
        pos = HArray(torch.cumsum(steps.to(torch.float64), dim=0).contiguous())
        del steps
        table, mean = HArray.empty((F, N), np.float64), HArray.empty(F, np.float64)
        window_terms = N * F * (F + 1) // 2
        out = laps(lambda: _msd.window(pos, table, mean), window_terms)
        kept = np.array(mean)
        print(json.dumps({"mode": "window", "F": F, "N": N, "msd_last": float(kept[-1]), "msd_mid": float(kept[F // 2]), **out}), flush=True)
        out = laps(lambda: _msd.window(pos, None, mean), window_terms)
        print(json.dumps({"mode": "window_msd", "F": F, "N": N, "same_bits_as_with_the_table": bool(np.array_equal(np.array(mean), kept)), **out}), flush=True)
        out = laps(lambda: _msd.direct(pos, table, mean), N * F)
        print(json.dumps({"mode": "direct", "F": F, "N": N, "msd_last": float(np.array(mean)[-1]), "bytes": F * N * 32,
                          "bytes_per_s": F * N * 32 / (out["ms"] * 1e-3), **out}), flush=True)
        out = laps(lambda: _msd.direct(pos, None, mean), N * F)
        print(json.dumps({"mode": "direct_msd", "F": F, "N": N, "bytes": F * N * 24, "bytes_per_s": F * N * 24 / (out["ms"] * 1e-3), **out}), flush=True)
        if f"{F}x{N}" in args.fft:
            sys.path.insert(0, os.path.join(ROOT, "tests"))
            import _msd_ref

            host = pos.dev().cpu().numpy()
            t0 = time.perf_counter()
            fft_mean = _msd_ref.fft_window(host).mean(axis=1)
            s = time.perf_counter() - t0
            print(json.dumps({"mode": "fft (numpy, host)", "F": F, "N": N, "ms": 1e3 * s, "msd_last": float(fft_mean[-1]),
                              "worst_difference_from_the_device_msd": float(np.abs(fft_mean - kept).max())}), flush=True)
            del host
        del pos, table, mean
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
