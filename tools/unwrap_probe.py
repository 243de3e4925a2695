"""Times the trajectory unwrap (mdapy_amd/_unwrap.py) on wrapped random walks resident in HBM, at three shapes of about the same
size — many atoms and few frames, the middle, few atoms and many frames:

    N = 1 048 576, F = 32      N = 65 536, F = 512      N = 2 048, F = 16 384

One JSON line per figure, then the table of profiles/unwrap.md:

  copy       torch's device copy of one (F, N, 3) float64 array: the yardstick (tools/ceilings.py measures the same at 4 GiB)
  unwrap     minimum-image mode with the frame axis cut into `chunks` runs: 1, the library's own choice (chunks = 0, resolved by
             the rule of csrc/unwrap.hip's uw_chunks, mirrored here) and the counts of --chunks; with and without row_of
  image      image mode, the library's choice
  npt cell   minimum-image mode with a cell that differs in every frame (the shim then inverts F cells on the host)
  numpy      the restatement of tests/_unwrap_ref.py on the host, once per shape

bytes = F N 24 (P + 1), P the passes over the positions: 1 with one chunk, 2 - 1/C with C (pass A skips the last chunk); plus
F N 8 of row_of per pass when used, F N 12 of flags in image mode.  GB/s = bytes / the median time.  Medians of --calls calls
after a warm-up call, best and worst beside them; every timed call ends in a device synchronise (the library's own: it reads its
flag word back).

Usage: python tools/unwrap_probe.py [--calls 7] [--chunks 2 4 8 ...] [--no-numpy] [--small]"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

SHAPES = ((1 << 20, 32), (1 << 16, 512), (1 << 11, 1 << 14))
AB, T, WAVES = 64, 16, 4096  # csrc/unwrap.hip: UW_AB, UW_T, UW_WAVES (and UW_ENOUGH, UW_ENOUGH_GATHERED in library_chunks)


def library_chunks(F, N, gathered=False):
    nab = (N + AB - 1) // AB
    C = 1 if nab >= (1024 if gathered else 2048) else min((WAVES + nab - 1) // nab, (F + T - 1) // T)
    return max(1, min(C, F))


def timed(run, calls):
    import torch

    run()
    torch.cuda.synchronize()
    times = []
    for _ in range(calls):
        t0 = time.perf_counter()
        run()
        torch.cuda.synchronize()
        times.append(time.perf_counter() - t0)
    times.sort()
    return times[len(times) // 2], times[0], times[-1]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=7)
    ap.add_argument("--chunks", type=int, nargs="*", default=[2, 4, 8, 16, 32, 64, 128, 256, 512])
    ap.add_argument("--no-numpy", action="store_true")
    ap.add_argument("--small", action="store_true", help="the shapes divided by 64 (a rehearsal of the script, not a measurement)")
    args = ap.parse_args()
    import torch

    from mdapy_amd import _lib, kernels

    if _lib.device_count() < 1 or not torch.cuda.is_available():
        sys.exit("unwrap_probe needs a HIP device")
    rows = []

    def report(**figure):
        print(json.dumps(figure), flush=True)
        rows.append(figure)

    for N, F in SHAPES:
        if args.small:
            N = max(N // 64, 1)
        gen = torch.Generator(device="cuda").manual_seed(1000 * F + N)
        length = 10.0
        # a walk with steps up to 0.2 of the edge, wrapped: every step of frac keeps 0.3 from a half-integer
        walk = torch.rand((1, N, 3), generator=gen, device="cuda", dtype=torch.float64) * length + torch.cumsum(
            (torch.rand((F, N, 3), generator=gen, device="cuda", dtype=torch.float64) - 0.5) * (0.4 * length), dim=0)
        flags = torch.floor(walk / length)
        wrapped = (walk - flags * length).contiguous()
        flags = flags.to(torch.int32).contiguous()
        del walk
        row_of = torch.argsort(torch.rand((F, N), generator=gen, device="cuda"), dim=1).contiguous()
        cells = np.repeat(np.diag([length] * 3)[None], F, axis=0)
        out = torch.empty_like(wrapped)
        frame_bytes = F * N * 24
        median, best, worst = timed(lambda: out.copy_(wrapped), args.calls)
        report(figure="copy", N=N, F=F, ms=median * 1e3, best_ms=best * 1e3, worst_ms=worst * 1e3, bytes=2 * frame_bytes,
               GBps=2 * frame_bytes / median / 1e9)
        for rows_used in (None, row_of):
            own = library_chunks(F, N, rows_used is not None)
            for asked in [1, 0] + [c for c in args.chunks if 1 < c <= F and c != own]:
                C = own if asked == 0 else asked
                passes = 1.0 if C == 1 else 2.0 - 1.0 / C
                moved = frame_bytes * (passes + 1.0) + (0 if rows_used is None else F * N * 8 * passes)
                median, best, worst = timed(lambda: kernels.unwrap.unwrap(wrapped, cells, (1, 1, 1), out, row_of=rows_used, chunks=asked),
                                            args.calls)
                report(figure="unwrap", N=N, F=F, row_of=rows_used is not None, chunks=C, library_choice=asked == 0, ms=median * 1e3,
                       best_ms=best * 1e3, worst_ms=worst * 1e3, bytes=moved, GBps=moved / median / 1e9)
        own = library_chunks(F, N)
        moved = frame_bytes * 2.0 + F * N * 12
        median, best, worst = timed(lambda: kernels.unwrap.unwrap(wrapped, cells, (1, 1, 1), out, image=flags), args.calls)
        report(figure="image", N=N, F=F, row_of=False, chunks=own, library_choice=True, ms=median * 1e3, best_ms=best * 1e3,
               worst_ms=worst * 1e3, bytes=moved, GBps=moved / median / 1e9)
        breathing = cells * (1.0 + 1e-6 * np.arange(F))[:, None, None]  # a cell that changes in every frame: F inverses on the host
        median, best, worst = timed(lambda: kernels.unwrap.unwrap(wrapped, breathing, (1, 1, 1), out), args.calls)
        own = library_chunks(F, N)
        passes = 1.0 if own == 1 else 2.0 - 1.0 / own
        report(figure="unwrap, npt cell", N=N, F=F, row_of=False, chunks=own, library_choice=True, ms=median * 1e3, best_ms=best * 1e3,
               worst_ms=worst * 1e3, bytes=frame_bytes * (passes + 1.0), GBps=frame_bytes * (passes + 1.0) / median / 1e9)
        if not args.no_numpy:
            import _unwrap_ref

            host = wrapped.cpu().numpy()
            t0 = time.perf_counter()
            want, _ = _unwrap_ref.restate(host, cells, (1, 1, 1))
            seconds = time.perf_counter() - t0
            report(figure="numpy", N=N, F=F, ms=seconds * 1e3, bytes=2 * frame_bytes, GBps=2 * frame_bytes / seconds / 1e9,
                   same_bits=bool(np.array_equal(want, _device_result(kernels, wrapped, cells, out))))
            del host, want
        del wrapped, flags, row_of, out
        torch.cuda.empty_cache()

    print("\n| N | F | what | chunks | ms (best .. worst) | GB/s |\n|---|---|---|---|---|---|")
    for r in rows:
        what = r["figure"] + (" + row_of" if r.get("row_of") else "")
        chunks = "" if "chunks" not in r else f"{r['chunks']}{' (library)' if r['library_choice'] else ''}"
        spread = f" ({r['best_ms']:.3f} .. {r['worst_ms']:.3f})" if "best_ms" in r else ""
        print(f"| {r['N']} | {r['F']} | {what} | {chunks} | {r['ms']:.3f}{spread} | {r['GBps']:.0f} |")


def _device_result(kernels, wrapped, cells, out):
    kernels.unwrap.unwrap(wrapped, cells, (1, 1, 1), out)
    return out.cpu().numpy()


if __name__ == "__main__":
    main()
