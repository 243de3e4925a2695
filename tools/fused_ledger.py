#!/usr/bin/env python
"""Instruction ledger of the fused label in the headline instance of the tile kernel, k_neighbor_lane<0,0,0,1,1,1,1> (FCNA=1, TK8=1,
IND=1, SLOT=1): the gfx950 ISA of mdapy_amd/csrc/neighbor_lane.hip with line tables, the label's instructions attributed to three phases
by the source line they came from — index and LDS reads (lane_fcna_f32 up to the pair tests, the ticket decode of the FCNA block),
pair tests (pair_tests_f32*), signatures (everything else of cna_core.hpp that the label inlines: the certificate, the pair-count or
word-loop signatures) — and weighted by issue class (profiles/r02_ubench_valu_rate3.txt, docs/NOTEBOOK.md "Micro-benchmarks"):
VGPR-only ~2.6 cycles; an SGPR / VCC / EXEC operand, v_cmp*, f64 and packed ~4.4; transcendental ~8.  Static counts, nothing is run.

The 14-hit branch of the label shares the 12-hit branch's source lines, so the file is compiled with that branch removed from a
temporary copy (the ledger is the 12-hit path's, the headline lattice's).  Phases of the 12-hit path that a wave may skip are listed
by name; the sum of a certified wave's hot path leaves out the general signatures behind the certificate.

    python tools/fused_ledger.py [REPO_ROOT]      (default: this repository; any checkout of it, e.g. the parent commit, works)"""
import collections, os, re, shutil, subprocess, sys, tempfile

KERNEL = "_ZN3mdh4lane15k_neighbor_laneILb0ELb0ELb0ELb1ELb1ELb1ELb1EE"
SGPR_RE = re.compile(r"(?<![a-z_])(s\d+|s\[\d+:\d+\]|vcc|vcc_lo|vcc_hi|exec|exec_lo|m0)(?![a-z_0-9])")
TRANS = ("v_rcp", "v_rsq", "v_sqrt", "v_exp", "v_log", "v_sin", "v_cos")


def cost(op, args):
    if op.startswith(TRANS):
        return 8.0
    if op.startswith(("v_cmp", "v_cmpx")) or "_f64" in op or op.startswith("v_pk_") or SGPR_RE.search(args):
        return 4.4
    return 2.6


def compile_tree(root):
    tmp = tempfile.mkdtemp()
    src = os.path.join(tmp, "mdapy_amd", "csrc")
    shutil.copytree(os.path.join(root, "mdapy_amd", "csrc"), src, ignore=shutil.ignore_patterns("*.o", "*.so"))
    shutil.copytree(os.path.join(root, "include"), os.path.join(tmp, "include"))
    p = os.path.join(src, "neighbor_lane.hip")
    text = open(p).read()
    text2 = re.sub(r"\n\s*else if \(hits == 14 && M >= 14\) label = lane_fcna_f32<14>\([^;]*\);", "", text)
    if text2 == text:
        raise SystemExit("the 14-hit branch of the label was not found")
    open(p, "w").write(text2)
    asm = os.path.join(tmp, "lane.s")
    subprocess.run(["/opt/rocm/bin/hipcc", "-O3", "-std=c++17", "--offload-arch=gfx950", "-ffp-contract=off", "-fPIC", "-gline-tables-only",
                    "-S", "--cuda-device-only", "-o", asm, p], check=True, stderr=subprocess.DEVNULL)
    return asm, src


def phase_table(src):
    """(file, first line, last line, phase) ranges"""
    lane = open(os.path.join(src, "neighbor_lane.hip")).read().splitlines()
    core = open(os.path.join(src, "cna_core.hpp")).read().splitlines()

    def find(lines, needle, start=0):
        for k in range(start, len(lines)):
            if needle in lines[k]:
                return k + 1
        return None

    out = []
    f0 = find(lane, "__device__ __forceinline__ int lane_fcna_f32(")
    fp = find(lane, "pair_tests_f32", f0)
    out.append(("neighbor_lane.hip", f0, fp - 1, "index + LDS reads"))
    out.append(("neighbor_lane.hip", fp, fp, "pair tests"))
    end = fp
    while not lane[end].startswith("}"):
        end += 1
    out.append(("neighbor_lane.hip", fp + 1, end + 1, "signatures"))
    b0 = find(lane, "if (FCNA) { // atoms without 12 or 14 neighbours")
    b1 = find(lane, "else if (label < 0) defer(cna_todo, id);", b0)
    out.append(("neighbor_lane.hip", b0, b1, "index + LDS reads"))
    td = find(core, "// to-do list of atoms left to a later kernel")
    pe = find(core, "template <int NN> constexpr int pair_a")  # pair tests: the pair enumeration up to the certificate (or the end)
    pz = find(core, "// fcc certificate") or td
    out.append(("cna_core.hpp", pe, pz - 1, "pair tests"))
    out.append(("cna_core.hpp", find(core, "struct Rows {"), pe - 1, "signatures"))
    out.append(("cna_core.hpp", pz, td - 1, "signatures"))
    fc = find(core, "__device__ __forceinline__ bool fcc_certificate(")
    if fc:
        fce = fc
        while not core[fce].startswith("}"):
            fce += 1
        out.append(("cna_core.hpp", fc, fce + 1, "certificate"))  # (a part of the signatures phase, listed on its own)
    return out


def main():
    root = os.path.abspath(sys.argv[1]) if len(sys.argv) > 1 else os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    asm, src = compile_tree(root)
    table = phase_table(src)
    files, inside, cur = {}, False, ("?", 0)
    n = collections.Counter()
    cyc = collections.Counter()
    total_valu = 0
    for raw in open(asm):
        m = re.match(r'\s*\.file\s+(\d+)\s+"([^"]*)"(?:\s+"([^"]*)")?', raw)
        if m:
            files[int(m.group(1))] = os.path.basename(m.group(3) or m.group(2))
            continue
        if raw.startswith(KERNEL) and ":" in raw:
            inside = True
            continue
        if not inside:
            continue
        m = re.match(r"\s*\.loc\s+(\d+)\s+(\d+)", raw)
        if m:
            cur = (files.get(int(m.group(1)), "?"), int(m.group(2)))
            continue
        s = raw.split(";")[0].strip()
        if not s or s.startswith(".") or s.endswith(":"):
            continue
        op = s.split()[0]
        if op == "s_endpgm":
            break
        if not op.startswith("v_"):
            continue
        total_valu += 1
        ph = None
        for f, lo, hi, name in table:  # the last matching range wins (the certificate inside the signatures)
            if cur[0] == f and lo <= cur[1] <= hi:
                ph = name
        if ph is None:
            continue
        args = s[len(op):]
        n[ph] += 1
        cyc[ph] += cost(op, args)
    print(f"fused label of {KERNEL} ({root}): static VALU instructions of the 12-hit path")
    print(f"{'phase':34s} {'instr':>6s} {'cycles (weighted)':>18s}")
    for ph in ("index + LDS reads", "pair tests", "certificate", "signatures"):
        if n[ph]:
            print(f"{ph:34s} {n[ph]:6d} {cyc[ph]:18.0f}")
    print(f"{'label total':34s} {sum(n.values()):6d} {sum(cyc.values()):18.0f}")
    hot = [ph for ph in ("index + LDS reads", "pair tests", "certificate") if n[ph]] if n["certificate"] else list(n)
    print(f"{'certified wave (hot path)':34s} {sum(n[p] for p in hot):6d} {sum(cyc[p] for p in hot):18.0f}")
    print(f"{'whole kernel, static VALU':34s} {total_valu:6d}")


if __name__ == "__main__":
    main()
