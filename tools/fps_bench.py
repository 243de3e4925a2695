"""Times farthest-point sampling and the PCA kernels (mdapy_amd/_sample.py) on tables resident in HBM, and writes profiles/fps.md.

  fps        N x 30 tables of uniform random numbers: 10^5 rows with 100 picks, 10^6 rows with 1000 picks, and 4 x 10^6 rows with
             50 picks (960 MB: beyond the 256 MiB Infinity Cache, the one whose bytes per second say something about HBM), on the
             grid path and — where it takes the table — on the one-workgroup path.  A pass reads 8 N D bytes and reads and writes
             16 N bytes of minima: that floor over the time per pass is the rate given.
  ceiling    the read-only stream rate of this device, measured here as tools/ceilings.py measures it (torch's sum over 2 GiB of
             float64): what the rate of a pass is compared with — not a data-sheet figure
  crossover  both paths on N x 30 tables from 128 to 32768 rows, 65 picks: the time per pick of each, and the largest table for
             which one workgroup is not slower — what FPS_BLOCK_AUTO_ELEMS in csrc/sample.hip is taken from
  pca        mdh_pca_moments and mdh_pca_project (3 components) on the first two tables
  numpy      the baseline, in the same process on the same machine: the restatement of the reference's loop (tests/_fps_ref.py
             fps_norm) — in full at 10^5 rows, its first --numpy-picks picks at 10^6 rows, scaled to 1000 (every pass costs the
             same) — and numpy's own centring, covariance and projection

Medians of --calls calls after a warm-up call; every timed call ends in a device synchronise (the sampling call reads its picks back).

Usage: python tools/fps_bench.py [--calls 3] [--numpy-picks 20] [--out profiles/fps.md] [--quick]"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
D = 30


def pass_bytes(N, columns):
    return 8 * N * columns + 16 * N


def main():
    p = argparse.ArgumentParser()
    p.add_argument("--calls", type=int, default=3)
    p.add_argument("--numpy-picks", type=int, default=20)
    p.add_argument("--out", default=os.path.join(ROOT, "profiles", "fps.md"))
    p.add_argument("--quick", action="store_true", help="small tables only: a rehearsal of the tool, not a measurement")
    args = p.parse_args()
    import torch

    import _fps_ref
    from mdapy_amd import _sample
    from mdapy_amd.devarray import HArray

    if not torch.cuda.is_available():
        raise RuntimeError("fps_bench needs a HIP device")

    def timed(fn):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        return time.perf_counter() - t0

    def laps(fn):
        fn()  # warm-up
        s = [timed(fn) for _ in range(max(args.calls, 1))]
        return float(np.median(s)), float(np.min(s)), float(np.max(s))

    lines = ["# Farthest-point sampling and PCA: tools/fps_bench.py", "",
             f"Device: {torch.cuda.get_device_name(0)}.  Medians of {args.calls} calls after a warm-up call (best - worst in brackets).", ""]

    def say(record, text):
        print(json.dumps(record), flush=True)
        lines.append(text)

    # ---- the read-only stream rate of this device (the method of tools/ceilings.py)
    n = 1 << (22 if args.quick else 28)
    a = torch.empty(n, dtype=torch.float64, device="cuda")
    a.fill_(1.0)
    med, _, _ = laps(lambda: a.sum())
    ceiling = n * 8 / med
    del a
    say({"mode": "ceiling", "bytes": n * 8, "ms": 1e3 * med, "TB_per_s": ceiling / 1e12},
        f"Read-only stream rate measured in this process (torch `sum` over {n * 8 / 2**30:.2f} GiB of float64, as `tools/ceilings.py`): "
        f"**{ceiling / 1e12:.2f} TB/s**.")
    lines.append("")

    # ---- sampling
    cases = [(2000, 20), (20000, 30)] if args.quick else [(100_000, 100), (1_000_000, 1000), (4_000_000, 50)]
    lines += ["## fps_sample", "",
              "| rows x columns | picks | path | ms per call | us per pass | floor bytes per pass | TB/s | of the stream rate | numpy ms | ratio |",
              "|---|---|---|---|---|---|---|---|---|---|"]
    tables = {}
    for N, picks_n in cases:
        host = np.random.default_rng(N).random((N, D))
        X = HArray.from_numpy(host)
        tables[N] = (host, X)
        picks = np.empty(picks_n, np.int32)
        numpy_ms, note = None, ""
        if N <= 1_000_000:
            part = picks_n if N <= 100_000 else min(picks_n, max(args.numpy_picks, 2))
            t0 = time.perf_counter()
            want = _fps_ref.fps_norm(part, host, 0)
            numpy_ms = 1e3 * (time.perf_counter() - t0) * (picks_n - 1) / (part - 1)
            note = "" if part == picks_n else f" (from {part} picks)"
        for path in ("grid", "block"):
            if path == "block" and not _sample.block_path_takes(N, D):
                continue
            med, best, worst = laps(lambda: _sample.fps(X, picks_n, 0, picks, _path=path))
            same = None if numpy_ms is None else bool(np.array_equal(picks[:len(want)], want))  # (roots may tie where squares do not)
            per_pass = med / (picks_n - 1)
            rate = pass_bytes(N, D) / per_pass
            ratio = None if numpy_ms is None else numpy_ms / (1e3 * med)
            say({"mode": "fps", "N": N, "D": D, "picks": picks_n, "path": path, "ms": 1e3 * med, "ms_best": 1e3 * best, "ms_worst": 1e3 * worst,
                 "us_per_pass": 1e6 * per_pass, "floor_bytes_per_pass": pass_bytes(N, D), "TB_per_s": rate / 1e12,
                 "share_of_stream_rate": rate / ceiling, "numpy_ms": numpy_ms, "ratio": ratio, "same_picks_as_numpy": same},
                f"| {N} x {D} | {picks_n} | {path} | {1e3 * med:.2f} ({1e3 * best:.2f} - {1e3 * worst:.2f}) | {1e6 * per_pass:.1f} | "
                f"{pass_bytes(N, D)} | {rate / 1e12:.2f} | {100 * rate / ceiling:.0f} % | "
                + ("not timed | |" if numpy_ms is None else f"{numpy_ms:.0f}{note} | {ratio:.0f} x |"))
        if N > 1_000_000:
            del tables[N]
    lines += ["", "The time per pass holds the launch, the ticket and the last workgroup's reduction besides the stream; tables up to "
              "10^6 x 30 (240 MB) fit the Infinity Cache, so only the 4 x 10^6-row rate is an HBM rate.", ""]

    # ---- where one workgroup stops being the faster one
    lines += ["## The two paths on small tables (65 picks)", "", "| rows x columns | entries | grid us per pick | one workgroup us per pick |",
              "|---|---|---|---|"]
    cross = 0
    sweep = [128, 256, 512, 1024, 2048, 4096] if args.quick else [128, 256, 512, 1024, 2048, 4096, 8192, 16384, 32768]
    for N in sweep:
        X = HArray.from_numpy(np.random.default_rng(N).random((N, D)))
        picks = np.empty(65, np.int32)
        per = {}
        for path in ("grid", "block"):
            per[path] = laps(lambda: _sample.fps(X, 65, 0, picks, _path=path))[0] / 64
        if per["block"] <= per["grid"]:
            cross = N * D
        say({"mode": "crossover", "N": N, "D": D, "grid_us_per_pick": 1e6 * per["grid"], "block_us_per_pick": 1e6 * per["block"]},
            f"| {N} x {D} | {N * D} | {1e6 * per['grid']:.1f} | {1e6 * per['block']:.1f} |")
    say({"mode": "crossover", "largest_entries_where_block_is_not_slower": cross},
        f"\nThe largest table of the sweep on which one workgroup is not slower: **{cross} entries** (a call's fixed costs — the "
        "copies of the picks, the synchronise — are in both columns).")
    lines.append("")

    # ---- PCA
    lines += ["## PCA kernels", "", "| rows x columns | kernel | ms | floor bytes | TB/s | numpy ms | ratio |", "|---|---|---|---|---|---|---|"]
    for N in [c[0] for c in cases[:2]]:
        host, X = tables[N]
        mean, cov = HArray.empty(D, np.float64), HArray.empty((D, D), np.float64)
        comp = HArray.from_numpy(np.linalg.qr(np.random.default_rng(1).normal(size=(D, 3)))[0])
        out = HArray.empty((N, 3), np.float64)
        t0 = time.perf_counter()
        centred = host - host.mean(axis=0)
        np.cov(centred.T)
        numpy_moments = time.perf_counter() - t0
        t0 = time.perf_counter()
        np.dot(centred, np.asarray(comp))
        numpy_project = time.perf_counter() - t0
        med, best, worst = laps(lambda: _sample.moments(X, mean, cov))
        floor = 2 * 8 * N * D  # the table is read twice: the means, then the centred products
        say({"mode": "pca_moments", "N": N, "D": D, "ms": 1e3 * med, "ms_best": 1e3 * best, "ms_worst": 1e3 * worst, "TB_per_s": floor / med / 1e12,
             "numpy_ms": 1e3 * numpy_moments},
            f"| {N} x {D} | moments | {1e3 * med:.3f} ({1e3 * best:.3f} - {1e3 * worst:.3f}) | {floor} | {floor / med / 1e12:.2f} | "
            f"{1e3 * numpy_moments:.1f} | {numpy_moments / med:.0f} x |")
        med, best, worst = laps(lambda: _sample.project(X, mean, comp, out))
        floor = 8 * N * D + 8 * N * 3
        say({"mode": "pca_project", "N": N, "D": D, "C": 3, "ms": 1e3 * med, "ms_best": 1e3 * best, "ms_worst": 1e3 * worst,
             "TB_per_s": floor / med / 1e12, "numpy_ms": 1e3 * numpy_project},
            f"| {N} x {D} | project (3) | {1e3 * med:.3f} ({1e3 * best:.3f} - {1e3 * worst:.3f}) | {floor} | {floor / med / 1e12:.2f} | "
            f"{1e3 * numpy_project:.1f} | {numpy_project / med:.0f} x |")
    lines += ["", "numpy's figures are the host's centring + `np.cov`, and `np.dot` of the centred table (which the first one made).", ""]

    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write("\n".join(lines))
    print(f"wrote {args.out}")


if __name__ == "__main__":
    main()
