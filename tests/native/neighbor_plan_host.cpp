// neighbor_plan_host.cpp — the planners of mdapy_amd/csrc/neighbor_plan.hpp in a program of their own: the header, a host compiler,
// nothing else.  Runs the recorded table (tests/golden/neighbor_plan.txt, written by tests/_neighbor_plan_cases.py) and compares
// every answer, then degenerate statistics whose answers only have to be sane.  The planner indexes v[1 + len] with len up to 97 and
// walks ~800 shapes: build this with -fsanitize=address,undefined to have that checked,
//     g++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=all -o neighbor_plan_host neighbor_plan_host.cpp
//     ./neighbor_plan_host ../golden/neighbor_plan.txt
// (tests/test_neighbor_plan.py builds it plain and runs it with the suite.)
#include "../../mdapy_amd/csrc/neighbor_plan.hpp"
#include <climits>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <fstream>
#include <iostream>
#include <sstream>
#include <string>
#include <vector>

using namespace mdh;

struct Case {
    std::string name;
    long long i[19];
    double d[16];
    int v[GridStats::NBIN];
    double want[46];
};

// the layout of mdh_debug_lane_plan (include/mdapy_amd.h)
static void answers(const Case &c, double *out)
{
    LanePlanIn in{};
    TiledPlanIn ti{};
    for (int d = 0; d < 3; ++d) { in.nc[d] = ti.nc[d] = (int)c.i[d]; in.pbc[d] = ti.pbc[d] = (int)c.i[5 + d]; in.o[d] = c.d[9 + d]; in.thick[d] = c.d[12 + d]; }
    for (int d = 0; d < 9; ++d) in.h[d] = c.d[d];
    in.ncell = ti.ncell = c.i[3]; in.mode = ti.mode = (int)c.i[4]; in.tri = ti.tri = (int)c.i[8];
    in.N = ti.N = c.i[9]; in.M = ti.M = c.i[10]; in.fcna = c.i[11] != 0; in.count = c.i[12] != 0; in.rc = c.d[15];
    for (int k = 0; k < GridStats::NBIN; ++k) in.v[k] = c.v[k];
    ti.occupied_cells = c.v[0];
    const LanePlan p = plan_lane(in);
    int hook[8];
    lane_plan_hook(in, p, hook);
    for (int k = 0; k < 46; ++k) out[k] = 0.0;
    const double lane[15] = {(double)p.txy, (double)p.tz, (double)p.cap, (double)p.tk8, (double)p.wgs, (double)p.rw, (double)p.mid, (double)p.T, (double)p.full,
                             (double)p.occupied, (double)p.reason, (double)p.lds_bytes, (double)p.pop, (double)p.over96, (double)p.runs};
    for (int k = 0; k < 15; ++k) out[k] = lane[k];
    for (int k = 0; k < 8; ++k) out[15 + k] = hook[k];
    if (p.txy) {
        const LaneLaunch ll = plan_lane_launch(p, in.nc, (int)c.i[13], (int)c.i[14], (int)c.i[15], (int)c.i[16], (int)c.i[17]);
        const double launch[16] = {(double)ll.nt[0], (double)ll.nt[1], (double)ll.nt[2], (double)ll.ntiles, (double)ll.tiles, (double)ll.tile_base, (double)ll.nt0_run,
                                   (double)ll.per, (double)ll.grid, (double)ll.standby, (double)ll.slice_pass, (double)ll.nsub, (double)ll.nt2b, (double)ll.list_cap,
                                   (double)ll.mop_tile_z, (double)ll.mop_nt2};
        for (int k = 0; k < 16; ++k) out[23 + k] = launch[k];
        out[44] = ll.cen_lo; out[45] = ll.cen_hi;
    }
    const TiledPlan tp = plan_tiled(ti);
    out[39] = tp.tile; out[40] = tp.tile_z; out[41] = tp.cellshift; out[42] = tp.full; out[43] = (double)tp.occupied;
    if (tp.tile) {
        const TiledLaunch tl = plan_tiled_launch(tp, ti.nc, ti.M);
        if (tl.per < 1 || tl.per_standby < 1 || tl.per_standby > 96 || (int64_t)tl.per * 8 < (tl.listed ? 1 : tl.ntiles)) { std::printf("%s: tiled launch\n", c.name.c_str()); std::exit(1); }
    }
}

static bool read_case(const std::string &line, Case &c)
{
    std::vector<std::string> f;
    std::stringstream ss(line);
    for (std::string part; std::getline(ss, part, '|');) f.push_back(part);
    if (f.size() != 5) return false;
    std::stringstream(f[0]) >> c.name;
    std::stringstream si(f[1]), sd(f[2]), sv(f[3]), so(f[4]);
    std::string tok;
    for (int k = 0; k < 19; ++k) { if (!(si >> c.i[k])) return false; }
    for (int k = 0; k < 16; ++k) { if (!(sd >> tok)) return false; c.d[k] = std::strtod(tok.c_str(), nullptr); }
    std::memset(c.v, 0, sizeof(c.v));
    while (sv >> tok) {
        if (tok == "-") continue;
        const size_t colon = tok.find(':');
        if (colon == std::string::npos) return false;
        const int val = (int)std::strtol(tok.c_str() + colon + 1, nullptr, 10);
        if (tok[0] == '*') { for (int k = 0; k < GridStats::NBIN; ++k) c.v[k] = val; continue; }
        const long k = std::strtol(tok.c_str(), nullptr, 10);
        if (k < 0 || k >= GridStats::NBIN) return false;
        c.v[k] = val;
    }
    for (int k = 0; k < 46; ++k) { if (!(so >> tok)) return false; c.want[k] = std::strtod(tok.c_str(), nullptr); }
    return true;
}

// what the kernel's comments promise of any plan
static bool sane(const LanePlanIn &in, const LanePlan &p)
{
    if (!p.txy) return p.reason == -1 || (p.reason <= -3 && p.reason >= -7);
    return p.reason == 0 && (p.txy + 2) * (p.txy + 2) * (p.tz + 2) <= 256 && p.cap >= 64 && p.cap <= 2040 && p.wgs >= 1 && p.wgs <= (p.tk8 ? 4 : 3) &&
           p.lds_bytes <= lane_lds_budget(p.wgs) && p.rw % 4 == 0 && p.rw >= 8 && p.rw <= 64 && (double)p.mid < in.rc * in.rc && p.T > 0.0f;
}

int main(int argc, char **argv)
{
    if (argc < 2) { std::printf("usage: %s tests/golden/neighbor_plan.txt\n", argv[0]); return 2; }
    std::ifstream f(argv[1]);
    if (!f) { std::printf("cannot read %s\n", argv[1]); return 2; }
    int cases = 0, bad = 0;
    Case head{};
    for (std::string line; std::getline(f, line);) {
        if (line.empty() || line[0] == '#') continue;
        Case c{};
        if (!read_case(line, c)) { std::printf("malformed line: %.40s\n", line.c_str()); return 2; }
        double got[46];
        answers(c, got);
        ++cases;
        for (int k = 0; k < 46; ++k)
            if (std::memcmp(&got[k], &c.want[k], sizeof(double)) != 0) { std::printf("%s: out[%d] = %a, recorded %a\n", c.name.c_str(), k, got[k], c.want[k]); ++bad; }
        if (c.name == "headline") head = c;
    }
    if (head.name.empty()) { std::printf("no case named headline\n"); return 2; }
    // degenerate statistics on the headline's box: all zero, all INT_MAX / 128, a negative occupancy, runs in the last bins only, and
    // each of them for every row width and both flags — the answers only have to be plans that keep the kernel's promises, or refusals
    int degenerate = 0;
    for (int kind = 0; kind < 5; ++kind)
        for (int M = 0; M <= 130; ++M)
            for (int flags = 0; flags < 4; ++flags) {
                Case c = head;
                c.i[10] = M; c.i[11] = flags & 1; c.i[12] = flags >> 1;
                for (int k = 0; k < GridStats::NBIN; ++k) c.v[k] = kind == 1 ? INT_MAX / 128 : 0;
                if (kind == 2) { c.v[0] = -7; c.v[9] = 1000; }
                if (kind == 3) { c.v[0] = INT_MIN; c.v[97] = c.v[98] = INT_MAX / 128; c.v[1] = INT_MAX / 4; }
                if (kind == 4) { c.v[0] = 1; c.v[29] = 1; c.i[9] = 19; } // one occupied cell, 19 atoms in it
                LanePlanIn in{};
                for (int d = 0; d < 3; ++d) { in.nc[d] = (int)c.i[d]; in.pbc[d] = (int)c.i[5 + d]; in.o[d] = c.d[9 + d]; in.thick[d] = c.d[12 + d]; }
                for (int d = 0; d < 9; ++d) in.h[d] = c.d[d];
                in.ncell = c.i[3]; in.N = c.i[9]; in.M = M; in.fcna = flags & 1; in.count = flags >> 1; in.rc = c.d[15];
                for (int k = 0; k < GridStats::NBIN; ++k) in.v[k] = c.v[k];
                const LanePlan p = plan_lane(in);
                int hook[8];
                lane_plan_hook(in, p, hook);
                if (!sane(in, p) || (hook[7] != 0) != (p.txy != 0)) { std::printf("degenerate statistics %d, M = %d, flags %d: not sane\n", kind, M, flags); ++bad; }
                if (p.txy)
                    for (int ll = -1; ll <= 1; ++ll) {
                        const LaneLaunch L = plan_lane_launch(p, in.nc, 0, kind == 2 ? 7 : 0, 0, 0, ll);
                        if (L.per < 1 || L.grid != (unsigned)L.per * 8u || L.ntiles < 1 || L.list_cap < 1) { std::printf("degenerate statistics %d, M = %d: launch\n", kind, M); ++bad; }
                    }
                double out[46];
                answers(c, out); // (the tiled plan and its launch too)
                ++degenerate;
            }
    std::printf("%d cases, %d degenerate inputs, %d differences\n", cases, degenerate, bad);
    return bad ? 1 : 0;
}
