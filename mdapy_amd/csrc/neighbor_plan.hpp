// neighbor_plan.hpp — what a pass over a built cell grid decides before it enqueues anything (neighbor_pass, neighbor.hip, and the
// launchers of neighbor_lane.hip and neighbor_tiled.hip).
//
// The decisions, written once for the launchers and for the host tests (mdh_debug_lane_plan, tests/test_neighbor_plan.py,
// tests/native/neighbor_plan_host.cpp): plain values in, plain structs out, no HIP call, no HIP type and no global — the header
// compiles with a host C++17 compiler alone.  The launchers do the I/O — the signature's statistics (grid_stats_hint), the plan
// memo, the test hook's words, allocations, launches — and every number a launch uses comes out of a struct from here.
//   plan_lane, lane_plan_hook, plan_lane_launch   the LDS-tile kernel (neighbor_lane.hip)
//   plan_tiled, plan_tiled_launch                 the round-1 tiled kernel (neighbor_tiled.hip)
//   choose_rows_front                             which of them runs in front of the thread-per-atom mop-up (neighbor_pass)
// Every rule only picks a path or a tile: the rows are the same whichever way a pass goes.
#pragma once
#include <stdint.h>
#include <stddef.h>
#include <algorithm>
#include <cmath>

#ifdef __HIPCC__
#define MDH_HD __host__ __device__
#else
#define MDH_HD
#endif

namespace mdh {

namespace img {
constexpr int MAX_M = 14; // whole box lengths an atom's raw coordinate may lie outside the box and still carry an image code (grid.hpp img::)
}

// the signature's statistics as a pass reads them (grid_stats_hint, neighbor_lane.hip)
struct GridStats {
    static constexpr int NBIN = 99; // v[0] = cells of the occupied region; v[1 + len] = 3-cell z-runs of that length (98: longer than 96)
    int v[NBIN];
    int last_listed = -1;   // tiles the first pass of the previous build with this (N, grid) listed for the second (-1: not known)
    int *listed_sink = nullptr; // pinned host word THIS build writes that count to (device-visible): its second pass, or, when none is launched, its mop-up (TileFilter::listed_sink)
};

// ---- the LDS-tile kernel (neighbor_lane.hip) ----
namespace lane {

// A workgroup is NW waves: 256 threads, four workgroups per CU.  A tile has at most one halo cell per thread.
constexpr int NW = 4;
constexpr int CEN_CAP = 80 * NW; // centre atoms a tile may hold
// tickets of a row + the spare slot, rounded up (rows are read back four tickets at a time).  (cna_rows: 28 bytes, room for a centre's
// bond rows — built, and dropped: the 2 KB cost the headline tile 49 atoms of room, 169 of its 51 200 tiles went to the slice pass
// (33 us), and since cna_counts_words fetches no row by a computed index nothing needs them)
MDH_HD constexpr int ticket_row(int M, bool cna_rows) { return (cna_rows && ((M + 4) & ~3) < 28) ? 28 : ((M + 4) & ~3); }
constexpr unsigned STANDBY_GRID = 512; // workgroups of the walked launch that stands by behind a first pass over a list of tiles
constexpr unsigned SLICE_GRID = 1024;  // workgroups of the slice pass

// tk8: one-byte tickets, else two-byte ones; rows of (M + 1) tickets rounded up to a multiple of four; rw rows per wave
// (the fused label takes no LDS of its own: ticket_row)
inline size_t lds_bytes(int cap, int64_t M, bool tk8, int rw, bool /* fcna */ = false)
{
    const size_t wave = std::max<size_t>((size_t)rw * (size_t)ticket_row((int)M, false) * (tk8 ? 1 : 2), 256); // (the kernel's wstride)
    const size_t tk = (size_t)NW * wave;
    return (size_t)cap * 16 + (size_t)cap * 16 + (size_t)cap * 8 + (size_t)CEN_CAP * 4 + (size_t)(cap + (cap & 1)) * 2 + ((tk + 15) & ~(size_t)15);
}

} // namespace lane

// Everything plan_lane reads.  Value-initialised and free of padding: it is compared as bytes (the launcher's memo keeps the last one
// as its key — an input added here is part of the key by construction).
struct LanePlanIn {
    int nc[3], mode;     // the grid (Grid, grid.hpp)
    int pbc[3], tri;     // the box (DBox, common.hpp) ...
    int64_t ncell;
    int64_t N, M;        // atoms; slots of a row (1 when counting)
    double h[9], o[3], thick[3];
    double rc;
    int fcna, count;     // the fused CNA label is wanted; counts only
    int v[GridStats::NBIN]; // GridStats::v
    int zero_;           // (keeps the struct free of padding)
};
static_assert(sizeof(LanePlanIn) == sizeof(int) * (11 + GridStats::NBIN) + sizeof(int64_t) * 3 + sizeof(double) * 16, "LanePlanIn must have no padding");

struct LanePlan {
    int txy, tz;      // tile shape in cells; txy == 0: not applicable
    int cap;          // atoms a tile's halo may hold in LDS
    bool tk8;         // rows of at most 16 slots: one-byte tickets, lean LDS layout, rows written by the centre's lane
    int wgs;          // workgroups per CU the LDS budget was cut for
    int rw;           // rows (centres) a wave works on at a time: 64, fewer for long rows in dense cells
    float mid, T;     // single-precision scan: the constant c subtracted from d2 (a little below rc^2) and the width W of the band above it
    bool full;        // every 4x4x4 block of cells holds atoms (last known statistics): all tiles are live
    int64_t occupied; // cells of the occupied region (last known)
    // why there is no plan (txy == 0), else 0:  -1 no atoms, a grid of equal cells, or rows of no or more than 128 slots;  -3 fewer than 7
    // cells on a periodic axis or 4 on an open one;  -4 a cutoff out of range;  -5 more than 5 % of the runs hold 89 atoms or more
    // (over96 of runs);  -6 no tile shape fits LDS;  -7 rows of more than 64 slots in cells of more than 19.5 atoms
    int reason;
    int lds_bytes;    // dynamic LDS of a workgroup
    int pop;          // atoms per cell of the occupied region, in thousandths (a plan, and refusal -7)
    int over96, runs; // refusal -5
};

// LDS budget of a workgroup where `wgs` of them share a CU: static tables (1.1 KB: the run table, scan scratch, flags) and a margin.
// LDS is handed out in 512-byte granules: 40 960 B in all give four workgroups per CU (measured: 40 544 do, 41 216 do not; 52.9 KB
// three, 54.3 KB not)
inline long lane_lds_budget(int wgs) { return 160 * 1024 / wgs - 1088 - (wgs == 4 ? 64 : 1600); }

// reason (negative) the tile kernel cannot take a call with this box, grid and row width; 0: it can
inline int lane_refusal(const LanePlanIn &in)
{
    if (in.mode != 0 || in.M <= 0 || in.M > 128) return -1;
    for (int d = 0; d < 3; ++d)
        if (in.nc[d] < (in.pbc[d] ? 7 : 4)) return -3; // image numbers from the cell pair need >= 7 cells; skipping the far side of an open axis >= 4
    return 0;
}

// The plan is a function of the box, the grid, N, M, rc and the run-length / occupancy statistics — in a trajectory the same from
// call to call; the search walks ~800 tile shapes (the launcher keeps the last plan of the thread, plan_lane_memo).
inline LanePlan plan_lane(const LanePlanIn &in)
{
    using namespace lane;
    const int64_t N = in.N, M = in.M;
    const double rc = in.rc;
    const bool fcna = in.fcna != 0, count = in.count != 0;
    LanePlan p{};
    if (N <= 0) { p.reason = -1; return p; }
    if (const int why = lane_refusal(in)) { p.reason = why; return p; }
    if (!(rc > 1e-12 && rc < 1e12)) { p.reason = -4; return p; }
    int64_t runs = 0, over32 = 0, over96 = 0;
    for (int k = 1; k < GridStats::NBIN; ++k) runs += in.v[k];
    for (int len = 29; len <= 97; ++len) over32 += in.v[1 + len]; // (a little below the limits: the statistics are the previous call's)
    for (int len = 89; len <= 97; ++len) over96 += in.v[1 + len];
    const bool long_runs = runs > 0 && (double)over32 > 0.002 * (double)runs; // many runs would not fit one 32-bit hit mask: the wide instance (three)
    // cells so full that more than a few per cent of the runs would not fit three masks (fewer — the wider last cell of a small box — go to the mop-up kernel)
    if (runs > 0 && (double)over96 > 0.05 * (double)runs) { p.reason = -5; p.over96 = (int)over96; p.runs = (int)runs; return p; }
    const int64_t occ = in.v[0] > 0 ? in.v[0] : in.ncell;
    const double pop = (double)N / (double)occ; // mean atoms per cell of the occupied region
    // rows of 65 ... 128 slots: measured against the round-1 tiled kernel on 4 M atoms of rattled fcc Cu (tools/rc_sweep.py,
    // profiles/r04_rc_sweep.txt) — ahead while a cell holds fewer than ~20 atoms (rc 5.6 / 5.8 / 6.0 A: 7.6 -> 5.5, ~8.3 -> 5.9,
    // 8.8 -> 5.7 ms), behind beyond (rc 6.5 A, 24 atoms per cell: a third of the tiles hold a run of more than 96 candidates and
    // go to the mop-up code, 10.9 -> 12.7 ms)
    if (M > 64 && pop > 19.5) { p.reason = -7; p.pop = (int)(1000.0 * pop); return p; }
    // rows of at most 16 slots in cells of a few atoms: one-byte tickets, the lean LDS layout, rows written by the centre's lane;
    // four workgroups per CU where the instance keeps to 128 VGPRs
    const bool tk8 = (count || M <= 16) && !long_runs;
    const int max_wgs = tk8 ? 4 : 3;
    // LDS budget: four workgroups per CU (the 128-VGPR instance only), else three, two, one, if the tile that allows is not
    // much worse than what fewer would get.  Rows of many slots in cells of many atoms (rc = 5 A, 50 slots: the reference's
    // own benchmark call) leave few centres per tile: the ticket rows are sized for them (rw rows per wave), not for 64.
    int best_txy = 0, best_tz = 0;
    int best_cap = 0, best_wgs = 0, best_rw = 64;
    double best_score = -1.0;
    const int nthr = NW * 64;
    for (int wgs = max_wgs; wgs >= 1; --wgs) {
        const long budget = lane_lds_budget(wgs);
        for (int txy = 1; txy <= 8; ++txy)
            for (int tz = 1; tz <= 24; ++tz) {
                const int nh = (txy + 2) * (txy + 2) * (tz + 2);
                if (nh > nthr)
                    continue;
                const int ncc = txy * txy * tz;
                const double c = ncc * pop;                                 // centre atoms per tile
                if (c * 1.15 > CEN_CAP)
                    continue;
                int rw = 64;
                if (!tk8) rw = std::min(64, std::max(8, ((int)std::ceil(c * 1.15 / NW) + 3) & ~3)); // (a row is a multiple of eight bytes: any count keeps the waves' blocks aligned)
                const long fixed = (long)lds_bytes(0, M, tk8, rw, fcna);
                const int cap = std::min((int)((budget - fixed - 2) / 42), 2040); // (a centre's LDS index takes 11 bits of its table entry)
                if (cap < 64 || nh * pop > 0.875 * cap) // head-room for density fluctuations; what overflows goes to the slice pass
                    continue;
                const double passes = std::ceil(c * 1.15 / (NW * rw)); // (head-room: a second pass for a handful of centres is a waste)
                const double util = c / (passes * nthr);                   // lane utilisation of the scan
                const double reuse = (double)ncc / (double)nh;             // centre cells per staged cell
                const int wpc = wgs * NW;                                  // waves per CU
                const double score = util * (0.35 + reuse) * (wpc == 16 ? 1.1 : (wpc == 12 ? 1.0 : (wpc == 8 ? 0.85 : (M > 64 ? 0.45 : 0.6))));
                if (score > best_score) { best_score = score; best_txy = txy; best_tz = tz; best_cap = cap; best_wgs = wgs; best_rw = rw; }
            }
    }
    if (!best_txy) { p.reason = -6; return p; }
    // Decision band of the single-precision scan (neighbor_lane.hip, file header).  E bounds the staged coordinates (far-atom check of
    // the kernel), du the error of one staged coordinate: rounding to f32 plus what the double-precision shift can lose;
    // |d2_f32 - d2| <= (2 du)(2 sqrt(3) |d| + 6 du) + 5 * 2^-24 max(d2, rc^2) for the three subtractions and the FMA chain.
    const int hmax = std::max(best_txy, best_tz) + 2;
    double E = ((double)hmax + 1.5) * rc;
    double big = E;
    if (in.tri) { // the halo is a parallelepiped: its edges along the cell vectors, coordinates bounded by their sum
        double ext = 0, span = 0;
        for (int d = 0; d < 3; ++d) {
            const double len = std::sqrt(in.h[3 * d] * in.h[3 * d] + in.h[3 * d + 1] * in.h[3 * d + 1] + in.h[3 * d + 2] * in.h[3 * d + 2]);
            ext += ((double)((d == 2 ? best_tz : best_txy) + 2) + 1.5) * len * rc / in.thick[d]; // a cell is rc / thickness of the vector
            span += len;
        }
        E = ext;
        big = E + 3.0 * span;
        for (int d = 0; d < 3; ++d) big += std::fabs(in.o[d]);
        big *= 4.0; // the wrap and the frame shift go through the fractional coordinates: a few more roundings
    } else {
        // (a raw coordinate may be img::MAX_M + 1 box lengths away from the box: the shift L * n loses at most an ulp of THAT)
        for (int d = 0; d < 3; ++d) big = std::max(big, std::fabs(in.o[d]) + (double)(img::MAX_M + 2) * std::fabs(in.h[d * 4]) + E);
    }
    const double du = std::ldexp(E, -24) * 1.01 + std::ldexp(big, -49);
    const double rcsq = rc * rc;
    const double tol = 2.0 * (11.0 * du * rc + 12.0 * std::ldexp(rcsq, -24)); // twice the bound: a wider band costs nothing
    // e = d2 - c in single precision is within tol of the exact value.  c: the largest float <= rc^2 - tol, so that e < 0 is
    // a hit for sure; W: the smallest float >= (rc^2 - c) + tol, so that e > W is a miss for sure
    float c = (float)(rcsq - tol);
    while ((double)c > rcsq - tol) c = std::nextafterf(c, -INFINITY);
    const double want = (rcsq - (double)c) + tol;
    float W = (float)want;
    while ((double)W < want) W = std::nextafterf(W, INFINITY);
    p.mid = c;
    p.T = W;
    p.txy = best_txy;
    p.tz = best_tz;
    p.cap = best_cap;
    p.tk8 = tk8;
    p.wgs = best_wgs;
    p.rw = best_rw;
    p.occupied = occ;
    // "full": (nearly) every 4x4x4 block of cells holds atoms — all tiles are launched, no list of live ones is made.  A couple of
    // per cent of empty blocks (the corner cell of a 100^3-cell fcc box holds no lattice site) cost a workgroup each that finds no
    // centre and leaves; the list costs three launches
    p.full = (double)occ >= 0.98 * (double)in.ncell;
    p.lds_bytes = (int)lds_bytes(p.cap, M, tk8, p.rw, fcna);
    p.pop = (int)(1000.0 * pop);
    return p;
}

// the eight words mdh_debug_neighbor_plan reports for a plan just made ([7] = 1: made since the last query) or refused
inline void lane_plan_hook(const LanePlanIn &, const LanePlan &p, int out8[8])
{
    for (int k = 0; k < 8; ++k) out8[k] = 0;
    if (!p.txy) {
        out8[6] = p.reason;
        if (p.reason == -5) { out8[5] = p.over96; out8[4] = p.runs; }
        if (p.reason == -7) out8[5] = p.pop;
        return;
    }
    out8[0] = p.txy; out8[1] = p.tz; out8[2] = p.cap; out8[3] = p.lds_bytes;
    out8[4] = p.full | (p.tk8 ? 2 : 0) | (p.wgs << 2); out8[5] = p.pop; out8[6] = (int)std::min<int64_t>(p.occupied, 2147483647); out8[7] = 1;
}

// Workgroups per XCD chunk (the launch grid is eight of them) of a first pass over a list of live tiles whose length only the device
// knows: live tiles expected from the last known occupancy — occupied cells / cells per tile, twice that since tiles are cut partly
// empty at the surface of the occupied region — plus 25 %, at most per_max; a workgroup takes further tiles of its chunk if that was too few
inline int expected_live_tiles_per_xcd(int64_t occupied, int cells_per_tile, int per_max)
{
    const int64_t est_live = std::max<int64_t>(1, occupied / std::max(1, cells_per_tile) * 2);
    return std::max(1, std::min(per_max, (int)((est_live + est_live / 4 + 7) / 8)));
}

// What launch_neighbor_lane allocates and enqueues.
// First pass, one tile per workgroup (`grid` of them) over
//   ALL     every tile of the grid: the statistics say that no 4x4x4 block of cells is empty, workgroup b owns tile b
//   WINDOW  the caller promised a window of planes along axis 0 (a slab of a decomposed system, mdh_hint_cell_window) and the cell
//           grid was built over it: the tiles that can hold atoms are ONE range of tile numbers (axis 0 is the slowest index) — no
//           list, no pass over the tiles of the global grid to make one; nt0_run tile planes from tile number tile_base
//   LIST    the list of live tiles, whose length only the device knows: the grid is cut for the expected number and a walked launch
//           stands by (`standby`) for what a longer list leaves over — it leaves at once otherwise
// Second pass (`slice_pass`): workgroups walk one-cell slices along z (nsub per tile) of the tiles the first pass listed.  Nothing
// was listed by the previous build with this (N, grid) (last_listed == 0: a lattice, nearly always): no slice pass at all — the
// mop-up takes the first pass's own list, whatever turns up on it this time, slowly but correctly, and reports its length so that the
// next build launches the slice pass again (a stand-by launch that finds an empty list is 5 us and a kernel boundary of every build).
struct LaneLaunch {
    enum Tiles { ALL, WINDOW, LIST };
    int nt[3];        // tiles per axis
    int64_t ntiles;
    Tiles tiles;
    int tile_base, nt0_run;
    int per;          // workgroups per XCD chunk of the first pass
    unsigned grid;    // ... and its launch grid
    bool standby;
    int cen_lo, cen_hi; // planes of axis 0 whose atoms want rows, as the kernel compares them
    bool slice_pass;
    int nsub, nt2b;   // slices per tile; tiles along z of the slice pass's tiling
    // what the mop-up walks (TileFilter): the slices of the second pass, or, without one, the tiles of the first in its own tiling
    int list_cap, mop_tile_z, mop_nt2;
};
inline LaneLaunch plan_lane_launch(const LanePlan &plan, const int nc[3], int win_lo, int win_hi, int cen_lo, int cen_hi, int last_listed)
{
    LaneLaunch L{};
    for (int d = 0; d < 3; ++d) {
        const int T = d == 2 ? plan.tz : plan.txy;
        L.nt[d] = (nc[d] + T - 1) / T;
    }
    const int *nt = L.nt;
    L.ntiles = (int64_t)nt[0] * nt[1] * nt[2];
    L.nsub = plan.tz; // second pass: one-cell slices along z
    L.per = (int)((L.ntiles + 7) / 8);
    L.tile_base = 0;
    L.nt0_run = nt[0];
    if (plan.full) {
        L.tiles = LaneLaunch::ALL;
    } else if (win_hi > win_lo) {
        L.tiles = LaneLaunch::WINDOW;
        // (tiles of the planes that hold atoms wanting rows: the window, or the centre window inside it)
        const int w_lo = cen_hi > cen_lo ? std::max(win_lo, cen_lo) : win_lo, w_hi = cen_hi > cen_lo ? std::min(win_hi, cen_hi) : win_hi;
        const int t_lo = w_lo / plan.txy, t_hi = (std::max(w_hi, w_lo + 1) - 1) / plan.txy;
        L.tile_base = t_lo * nt[1] * nt[2];
        L.nt0_run = t_hi - t_lo + 1;
        L.per = (int)(((int64_t)L.nt0_run * nt[1] * nt[2] + 7) / 8);
    } else {
        L.tiles = LaneLaunch::LIST;
        L.per = expected_live_tiles_per_xcd(plan.occupied, plan.txy * plan.txy * plan.tz, L.per);
    }
    L.grid = (unsigned)(L.per * 8);
    L.standby = L.tiles == LaneLaunch::LIST && (int64_t)L.per * 8 < L.ntiles;
    L.cen_lo = cen_hi > cen_lo ? cen_lo : 0;
    L.cen_hi = cen_hi > cen_lo ? cen_hi : 0x7fffffff;
    L.nt2b = nt[2] * L.nsub;
    L.slice_pass = last_listed != 0;
    L.list_cap = (int)std::min<int64_t>(L.slice_pass ? L.ntiles * L.nsub : L.ntiles, 2147483647);
    L.mop_tile_z = L.slice_pass ? 1 : plan.tz;
    L.mop_nt2 = L.slice_pass ? L.nt2b : nt[2];
    return L;
}

// ---- the round-1 LDS-tiled kernel (neighbor_tiled.hip): double-precision scan, any run length; serves the cells too full for the
// tile kernel above ----
// Tile shape (cells): TXY x TXY x TZ
struct TileShape { int txy, tz; };
namespace tiled {
#ifndef MDH_HALO_CAP
#define MDH_HALO_CAP 1024
#endif
constexpr int HALO_CAP = MDH_HALO_CAP; // atoms a tile's halo may hold in LDS (30 B each)
constexpr int NT = 256;        // threads per workgroup
#ifndef MDH_MAX_NH
#define MDH_MAX_NH 512
#endif
constexpr int MAX_NH = MDH_MAX_NH;    // halo cells a tile may have
constexpr int MAX_COLS = 64;   // (x,y) columns of centre cells a tile may have
constexpr int TICK_STRIDE = NT + 2; // ticket slot stride (u16 units): 516 B -> consecutive slots shift by one bank

inline size_t tiled_lds_bytes(int64_t M)
{
    return (size_t)HALO_CAP * (24 + 4 + 2) + (size_t)NT * (24 + 4 + 4) + (size_t)TICK_STRIDE * (size_t)M * 2;
}

// pick the tile shape for a mean cell population `pop`
inline TileShape choose_shape(double pop)
{
    TileShape best{0, 0};
    double best_score = -1.0;
    for (int txy = 2; txy <= 8; ++txy)
        for (int tz = 2; tz <= 16; ++tz) {
            const int nh = (txy + 2) * (txy + 2) * (tz + 2);
            if (nh > MAX_NH || txy * txy > MAX_COLS)
                continue;
            if (nh * pop > 0.86 * HALO_CAP) // head-room for density fluctuations; overflowing tiles fall back
                continue;
            const double c = txy * txy * tz * pop;                       // centre atoms per tile
            const double util = c / (std::ceil(c / NT) * NT);           // lane utilisation of the scan
            const double reuse = (double)(txy * txy * tz) / (double)nh; // centre cells per staged cell
            const double score = util * (0.35 + reuse);
            if (score > best_score) { best_score = score; best = TileShape{txy, tz}; }
        }
    return best;
}
} // namespace tiled

struct TiledPlanIn {
    int nc[3], mode;
    int pbc[3], tri;
    int64_t ncell, N, M;
    int64_t occupied_cells; // cells of the occupied region (GridStats::v[0]); 0 = assume all of them
};
struct TiledPlan {
    int tile;        // cells per tile edge in x and y; 0 = not applicable
    int tile_z;      // cells per tile edge in z
    bool cellshift;  // every periodic axis has >= 7 cells: per-cell image shifts may replace the minimum-image search
    bool full;       // every 4x4x4 block of cells holds atoms (last known occupancy): all tiles are live
    int64_t occupied; // cells of the occupied region (last known)
};
// How many cells hold atoms?  The tile shape is sized for the population of the OCCUPIED region: a box that is mostly empty
// (vacuum around a slab or a particle, the other ranks' slabs of a decomposed system) would otherwise get tiles whose halo
// overflows LDS wherever the atoms are.  occupied_cells is GridStats::v[0] of the signature (grid_stats_hint, neighbor_lane.hip:
// counted on the device in blocks of 4 x 4 x 4 cells, read by the next call).  A stale value costs speed, never correctness
// (overflowing tiles fall back to the thread-per-atom kernel).
inline TiledPlan plan_tiled(const TiledPlanIn &in)
{
    using namespace tiled;
    TiledPlan p{0, 0, false, false, 0};
    if (in.tri || in.mode != 0 || in.N <= 0 || in.M <= 0)
        return p;
    const double pop = (double)in.N / (double)(in.occupied_cells > 0 ? in.occupied_cells : in.ncell); // mean atoms per occupied cell
    const TileShape sh = choose_shape(pop);
    if (!sh.txy)
        return p;
    if (tiled_lds_bytes(in.M) > 62 * 1024) // ticket rows must fit next to the halo (<= 64 KiB: two workgroups per CU)
        return p;
    int mp = 1;
    while (mp < in.M) mp <<= 1;
    if (mp > NT)
        return p;
    p.tile = sh.txy;
    p.tile_z = sh.tz;
    p.full = in.occupied_cells >= in.ncell;
    p.occupied = in.occupied_cells > 0 ? in.occupied_cells : in.ncell;
    p.cellshift = true;
    for (int d = 0; d < 3; ++d)
        if (in.pbc[d] && in.nc[d] < 7)
            p.cellshift = false;
    return p;
}

// What launch_neighbor_tiled allocates and enqueues: a box that is full of atoms takes one tile per workgroup (workgroup b owns tile
// b); else the XCD chunks are cut from the list of tiles that hold centre atoms and the grid follows the expected number of them —
// more than that and workgroups loop (k_neighbor_tiled)
struct TiledLaunch {
    int nt[3];
    int64_t ntiles;
    bool listed;        // the list of live tiles is made
    int per;            // workgroups per XCD chunk of the launch that is expected to run
    int per_standby;    // ... of the variant that the device flag will most likely send home: three workgroups per CU, looping if it does run
    int mp_shift;       // log2 of the row width rounded up to a power of two
    size_t lds;
};
inline TiledLaunch plan_tiled_launch(const TiledPlan &plan, const int nc[3], int64_t M)
{
    TiledLaunch L{};
    for (int d = 0; d < 3; ++d) {
        const int T = d == 2 ? plan.tile_z : plan.tile;
        L.nt[d] = (nc[d] + T - 1) / T;
    }
    L.ntiles = (int64_t)L.nt[0] * L.nt[1] * L.nt[2];
    L.listed = !plan.full;
    L.per = (int)((L.ntiles + 7) / 8);
    if (L.listed) L.per = expected_live_tiles_per_xcd(plan.occupied, plan.tile * plan.tile * plan.tile_z, L.per);
    L.per_standby = std::min(L.per, 96);
    while ((1 << L.mp_shift) < M) ++L.mp_shift;
    L.lds = tiled::tiled_lds_bytes(M);
    return L;
}

// ---- neighbor_pass: the kernel in front of the thread-per-atom mop-up ----
// LANE: the LDS-tile kernel (orthogonal and triclinic boxes); the thread-per-atom code then only mops up what it listed
// TILED: cells too full for it (or forced): the round-1 tiled kernel — orthogonal boxes, rows, and no slot grid, which it does not read
// ATOMS_ONLY: the thread-per-atom code does everything
// variant: mdh_debug_set_neighbor_variant (0: as shipped; 1: thread-per-atom only; 2: no tile kernel)
enum class RowsFront { LANE, TILED, ATOMS_ONLY };
inline RowsFront choose_rows_front(int variant, bool count, bool tri, bool slot_grid, bool lane_plan, bool tiled_plan)
{
    if (variant == 0 && lane_plan) return RowsFront::LANE;
    if (!count && variant != 1 && !tri && !slot_grid && tiled_plan) return RowsFront::TILED;
    return RowsFront::ATOMS_ONLY;
}

} // namespace mdh
