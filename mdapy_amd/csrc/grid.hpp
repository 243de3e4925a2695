// grid.hpp — the rc-wide cell grid shared by the neighbor build, kNN and RDF kernels.
#pragma once
#include "common.hpp"
#include "grid_plan.hpp"
#include "neighbor_plan.hpp"
#include <atomic>
#include <cmath>

namespace mdh {

// mode 0: cells of width rc anchored at the origin, last cell absorbs the remainder (neighbor.cpp:29-62)
// mode 1: nc equal cells across the box, floor((x-o)/L*nc)  (radial_distribution_function.cpp:109-141; also kNN)
struct Grid {
    int nc[3];
    int64_t ncell;
    double rc_inv;
    int mode;
};

// Image codes (orthogonal boxes).  An atom handed in outside the box on a periodic axis has raw = wrapped + m L, m a whole number
// of box lengths (an unwrapped trajectory: atoms that have diffused through the faces); the cell grid sees the wrapped atom, the
// reference's distances are computed from the raw one (neighbor.cpp:164-166) and then folded by L * floor(d / L + 0.5)
// (box.h:120-124).  The tile kernels take that image number from codes instead of a division per pair:
//   atom code      (m + 15) per axis, 5 bits each, m in [-14, 14] (more: the build's flags[0], the thread-per-atom kernel)
//   cell code      (n + 1) per axis, 2 bits each: the candidate's cell seen from the tile, n in {-1, 0, 1}
//   combined code  (n + m + 16) per axis, 5 bits each — fits the 16-bit LDS entry of a staged atom
namespace img { // (MAX_M = 14: neighbor_plan.hpp)
constexpr int ATOM_NEUTRAL = 15 | (15 << 5) | (15 << 10);
constexpr int CELL_NEUTRAL = 1 | (1 << 2) | (1 << 4);
constexpr int NEUTRAL = 16 | (16 << 5) | (16 << 10); // combined code "no shift"
__host__ __device__ __forceinline__ int combine(int cc, int ca)
{
    return ((cc & 3) + (ca & 31)) | ((((cc >> 2) & 3) + ((ca >> 5) & 31)) << 5) | ((((cc >> 4) & 3) + ((ca >> 10) & 31)) << 10);
}
__host__ __device__ __forceinline__ int axis(int code, int d) { return ((code >> (5 * d)) & 31) - 16; } // image number of a combined code
} // namespace img

struct GridFeedback;
// device buffers produced by build_cell_grid, cell_grid.hip (owned by the Scope that built them)
struct CellGrid {
    Grid g{};
    GridFeedback *fb = nullptr; // a build for neighbor rows (GridRequest::slots_ok): what the builds of its signature leave for the next one
    int win_lo = 0, win_hi = 0; // planes [win_lo, win_hi) of axis 0 the grid was built over (a promised window, cell_grid.hip); 0, 0: all
    int cen_lo = 0, cen_hi = 0; // planes [cen_lo, cen_hi) of axis 0 whose atoms want rows (mdh_hint_centre_window: a slab's own atoms; the rest of the window is halo); 0, 0: all
    mutable bool flags_fresh = false; // flags[] were zeroed by build_cell_grid and nobody has used them yet (the first neighbor pass skips its own memset: every hipMemsetAsync is a 5 us launch)
    int *cell_start = nullptr; // [ncell+1] exclusive prefix of the per-cell populations
    int *order = nullptr;      // [N] atom ids, cell-major, DESCENDING id inside a cell
    double *xs = nullptr, *ys = nullptr, *zs = nullptr; // [N] raw positions in `order`
    // device flags written while binning:
    //   flags[0] != 0 : some atom's raw coordinate differs from its wrapped one by more than `slack` on a
    //                   periodic axis (unwrapped input) -> per-cell image shifts are not valid
    //   flags[1]      : largest cell population
    int *flags = nullptr;
    unsigned short *mvs = nullptr; // [N] per-atom image code (raw vs wrapped coordinate; img::), in `order`
    // [N] the same five values as one 32-byte record per atom (neighbor builds): the tile kernel stages an atom with two
    // 16-byte requests instead of five small ones
    struct Packed { double x, y, z; int id, code; };
    Packed *pk = nullptr; // when set, xs / ys / zs / mvs are NOT filled (ensure_unpacked() does that for the kernels that want them)
    // INDIRECT (neighbor builds of input that comes in some spatial order): no sorted copy of the atoms at all — atom q of the cell
    // order is atom order[q] of the CALLER's arrays (ix, iy, iz; image code imv[order[q]] when flags[4] says that any atom has
    // one).  pk, xs, ys, zs, mvs are all null; the kernels read through `order` (the tile kernel stages a cell's atoms with four
    // small gathers per atom where the record took two 16-byte reads — and the grid build is one pass over 56 B per atom shorter)
    const double *ix = nullptr, *iy = nullptr, *iz = nullptr;
    const unsigned short *imv = nullptr;
    // SLOT GRID (slot_cap != 0; an indirect grid of a neighbor build whose cells were small last time, cell_grid.hip): the ids of
    // cell c sit in fixed slots of `order`, DESCENDING, where the cell's atomic counter placed them — no prefix sum, no second
    // scatter.  Two planes of four slots per cell (slot_pos): the first four ids at order[4 c ...], the next four at
    // order[slot_hi + 4 c ...] — a lattice's cells hold one, two or four atoms and touch the first plane only, half the bytes of
    // eight slots side by side (profiles/slot_grid.md).  cell_start then holds the ncell per-cell COUNTS (no [ncell] entry); a count
    // keeps running past slot_cap, and the atoms it could not place are (cell, id) entries of the spill list, in no order.
    int slot_cap = 0;
    int64_t slot_hi = 0;              // first entry of the second plane (4 ncell)
    const int2 *spill = nullptr;      // [N]
    const unsigned *n_spill = nullptr; // device counter: entries of spill
    int64_t n_binned = 0;             // slot grid: atoms handed to the build (absent ones, x = NaN, included: they take no cell)
    // a build that keeps the slot grid's history (GridFeedback::BIG): its in-cell sort stamps *big_stamp with big_gen when it sees
    // a cell of more than SLOT_CAP atoms; the LAST kernel of the pass over the grid turns that into the signature's pinned word
    // (TileFilter::big_sink: 1 or 0 — a definite answer per finished build, so a host that runs many builds ahead reads the last one)
    const unsigned *big_stamp = nullptr;
    unsigned big_gen = 0;
    int *big_sink = nullptr;
};
// position in CellGrid::order of slot k (< SLOT_CAP) of cell c; hi: CellGrid::slot_hi
__host__ __device__ __forceinline__ int64_t slot_pos(int64_t c, int k, int64_t hi) { return c * 4 + k + (k >= 4 ? hi - 4 : 0); }
// the second plane and the spill list of a slot grid, as the thread-per-atom kernels see them (CellView below)
struct SlotSpill { const int2 *list = nullptr; const unsigned *n = nullptr; int64_t hi = 0; };
// a cell-sorted atom, from either representation
struct SortedView {
    const double *xs, *ys, *zs;
    const int *order;
    const CellGrid::Packed *pk;
    bool indirect; // xs, ys, zs are the caller's arrays, read at order[q] (CellGrid::ix)
    __device__ __forceinline__ void get(int64_t q, double &x, double &y, double &z, int &id) const
    {
        if (pk) { const CellGrid::Packed r = pk[q]; x = r.x; y = r.y; z = r.z; id = r.id; }
        else if (indirect) { id = order[q]; x = xs[id]; y = ys[id]; z = zs[id]; }
        else { x = xs[q]; y = ys[q]; z = zs[q]; id = order[q]; }
    }
    // four of them, every load of the four issued before the first is used: the form is looked at once, not per atom
    __device__ __forceinline__ void get4(const int64_t (&q)[4], double (&x)[4], double (&y)[4], double (&z)[4], int (&id)[4]) const
    {
        if (pk) {
#pragma unroll
            for (int u = 0; u < 4; ++u) { const CellGrid::Packed r = pk[q[u]]; x[u] = r.x; y[u] = r.y; z[u] = r.z; id[u] = r.id; }
            return;
        }
#pragma unroll
        for (int u = 0; u < 4; ++u) id[u] = order[q[u]];
        if (indirect) {
#pragma unroll
            for (int u = 0; u < 4; ++u) { x[u] = xs[id[u]]; y[u] = ys[id[u]]; z[u] = zs[id[u]]; }
        } else {
#pragma unroll
            for (int u = 0; u < 4; ++u) { x[u] = xs[q[u]]; y[u] = ys[q[u]]; z[u] = zs[q[u]]; }
        }
    }
    __device__ __forceinline__ int id_of(int64_t q) const { return pk ? pk[q].id : order[q]; }
};
inline SortedView view_of(const CellGrid &cg)
{
    if (!cg.pk && !cg.xs && cg.ix) return SortedView{cg.ix, cg.iy, cg.iz, cg.order, nullptr, true};
    return SortedView{cg.xs, cg.ys, cg.zs, cg.order, cg.pk, false};
}
int ensure_unpacked(Scope &sc, CellGrid &cg, int64_t N); // xs, ys, zs, mvs from pk (no-op when they exist)

// neighbor_tiled.hip: the round-1 LDS-tiled kernel (double-precision scan, any run length); serves the cells too full for neighbor_lane.hip
// (TiledPlan, plan_tiled: neighbor_plan.hpp)
// what the LDS-tiled kernel leaves to the thread-per-atom kernel: tiles whose halo did not fit in LDS
// (flag[t] != 0; *any counts them).  flag == nullptr: no filtering (the thread-per-atom kernel does everything).
struct TileFilter {
    const unsigned char *flag = nullptr;
    const int *any = nullptr;
    const int *moved = nullptr; // != nullptr and *moved != 0: the tiled kernel stood down (unwrapped input), take every atom
    const int *list = nullptr;  // != nullptr: ids of the flagged tiles, *any of them (k_neighbor_tiles walks the list; the flag scan over all atoms is skipped)
    int list_cap = 0;
    int *cna_todo = nullptr;    // != nullptr (fused neighbor + fixed CNA): the mop-up kernels list the atoms they take here, count first
    int tile = 1, tile_z = 1;
    int nt[3] = {1, 1, 1};
    int *listed_sink = nullptr; // != nullptr: the list is the tile kernel's FIRST pass's (no slice pass ran); the mop-up writes its length here (GridStats::listed_sink)
    const unsigned *big_stamp = nullptr; unsigned big_gen = 0; int *big_sink = nullptr; // CellGrid::big_sink: published by the pass's last kernel
};

// What one pass over a built cell grid is to leave behind (neighbor.hip neighbor_pass and the kernels' launchers)
struct RowsRequest {
    // COUNT_ONLY: nn and *max_count only (first pass of the exact-width variant): no rows, M is 1
    // KEEP_PADS:  reference semantics: valid slots written, the slots behind them keep what the caller put there
    // WRITE_PADS: ... and the slots behind them written too (-1, rc + 1)
    enum Pads { COUNT_ONLY, KEEP_PADS, WRITE_PADS };
    int *verlet = nullptr;  // [N][M] rows in original atom order
    double *dist = nullptr; // [N][M]
    int *nn = nullptr;      // [N] counts (they keep running past M)
    int64_t M = 1;
    Pads pads = WRITE_PADS;
    // nobody reads the distances (knn.hip: rows as candidates of a k-nearest search; 8 M bytes per atom written and ~300 instructions
    // per four slots saved): the tile kernel's wide instance writes ids and counts only, every other kernel distances as always
    bool ids_only = false;
    int *max_count = nullptr; // COUNT_ONLY: the largest count (device word, zeroed by the caller)
    // pattern != nullptr (not COUNT_ONLY): the fixed-cutoff CNA label (cna.cpp:429-506, same rc) of every centre the tile kernel
    // takes is written too; the atoms its mop-up kernels take are listed in todo (count first) for a pass over the finished rows
    int *pattern = nullptr, *todo = nullptr;
};
int launch_neighbor_tiled(Scope &sc, const CellGrid &cg, const TiledPlan &plan, int64_t N, const DBox &b, double rc,
                          const RowsRequest &rows, TileFilter &tf);

// neighbor_lane.hip: LDS tiles, one thread per centre atom, single-precision pruning (see the file header)
// (GridStats, LanePlanIn, LanePlan, plan_lane: neighbor_plan.hpp)
// What the builds of one (N, grid, device) signature leave for the next one: a neighbor build steers itself by what the previous
// build of the same system reported.  One heap object per signature, never freed (cell_grid.hip grid_feedback), reached through
// CellGrid::fb.  Every word arrives when the device gets there: a build that reads an old answer is a slower one, never a wrong one.
struct GridFeedback {
    static constexpr int LISTED = GridStats::NBIN, BIG = LISTED + 1, WORDS = BIG + 2;
    int64_t N, ncell; int device; // the signature
    // one block of pinned host memory that the device writes:
    //   [0, NBIN)  GridStats::v, copied behind k_grid_stats (grid_stats_hint)
    //   [LISTED]   tiles the first pass of the last finished build listed for the second (-1: not known; GridStats::listed_sink)
    //   [BIG]      did the last FINISHED build see a cell of more than SLOT_CAP atoms (1 / 0; -1: none has finished yet — the first
    //              builds of a signature are compact ones; CellGrid::big_sink), [BIG + 1] such a cell's count
    int *host;
    // host only (atomic: two threads may build the same signature)
    std::atomic<int> width;      // the last exact row width (mdh_build_neighbor_exact); 0: none
    std::atomic<unsigned> calls; // builds that have read the statistics; 0: not counted yet
};
// the statistics of cg's signature (cg.fb), counted on the device when they are stale
int grid_stats_hint(Scope &sc, const CellGrid &cg, GridStats *out);
// what plan_lane reads, from the box, the grid and the statistics
LanePlanIn lane_plan_in(const DBox &b, const Grid &g, int64_t N, int64_t M, const GridStats &gs, double rc, bool fcna, bool count);
// plan_lane behind the thread's memo of its last plan; fills the thread's report (mdh_debug_neighbor_plan, lane_last_listed)
LanePlan plan_lane_memo(const LanePlanIn &in, const GridStats &gs);
int lane_last_listed(); // tiles listed for the slice pass as last seen when a plan was made (mdh_debug_counters)
int launch_neighbor_lane(Scope &sc, const CellGrid &cg, const LanePlan &plan, const GridStats &gs, int64_t N, const DBox &b, double rc,
                         const RowsRequest &rows, TileFilter &tf);
// neighbor.hip, for other units of the library (knn.hip): the rows of a cutoff build on device arrays — its own cell grid, pads
// written (-1 / rc + 1), counts that keep running past M — enqueued on the Scope's stream.  ids_only: RowsRequest::ids_only
int neighbor_rows_device(Scope &sc, const double *dx, const double *dy, const double *dz, int64_t N, const DBox &b, double rc, int *dv,
                         double *dd, int *dn, int64_t M, const int64_t *dkey, bool ids_only);
// cna.hip: fixed-cutoff CNA from finished lists on the caller's stream — of all atoms, or of the atoms listed in todo
// (todo[0] = count, device side) with the reference expression
// done != nullptr: todo sits in a kept block (Scope::KEEP_TODO) — the kernel that walks the list clears its counters when it leaves
void launch_fcna_all(hipStream_t st, const DBox &b, const double *x, const double *y, const double *z, int64_t N, const int *verlet,
                     int64_t M, const int *nn, int *pattern, double rc, int *todo, int *done = nullptr, const Pos4 *pos = nullptr, const int *use_pos = nullptr);
void launch_fcna_listed(hipStream_t st, const DBox &b, const double *x, const double *y, const double *z, int64_t N, const int *verlet,
                        int64_t M, const int *nn, int *pattern, double rc, int *todo, int *done = nullptr);

__host__ __device__ __forceinline__ int pmod(int a, int n) // neighbor.cpp:18-22
{
    int r = a % n;
    return r < 0 ? r + n : r;
}

// cell coordinates of an already wrapped position (neighbor.cpp:29-62)
template <bool TRI>
__device__ __forceinline__ void cell_coords(const DBox &b, const Grid &g, double x, double y, double z, int &c0,
                                            int &c1, int &c2)
{
    double f0, f1, f2;
    if (TRI) {
        double dx = x - b.o[0], dy = y - b.o[1], dz = z - b.o[2];
        double nx = dx * b.hi[0] + dy * b.hi[3] + dz * b.hi[6];
        double ny = dx * b.hi[1] + dy * b.hi[4] + dz * b.hi[7];
        double nz = dx * b.hi[2] + dy * b.hi[5] + dz * b.hi[8];
        if (g.mode == 0) {
            f0 = floor(nx * b.thick[0] * g.rc_inv);
            f1 = floor(ny * b.thick[1] * g.rc_inv);
            f2 = floor(nz * b.thick[2] * g.rc_inv);
        } else {
            f0 = floor(nx * g.nc[0]);
            f1 = floor(ny * g.nc[1]);
            f2 = floor(nz * g.nc[2]);
        }
    } else if (g.mode == 0) {
        f0 = floor((x - b.o[0]) * g.rc_inv);
        f1 = floor((y - b.o[1]) * g.rc_inv);
        f2 = floor((z - b.o[2]) * g.rc_inv);
    } else {
        f0 = floor((x - b.o[0]) / b.h[0] * g.nc[0]);
        f1 = floor((y - b.o[1]) / b.h[4] * g.nc[1]);
        f2 = floor((z - b.o[2]) / b.h[8] * g.nc[2]);
    }
    // static_cast<int> then clamp to [0, nc-1] (neighbor.cpp:58-61); done in
    // floating point first so that huge values saturate instead of wrapping.
    f0 = fmin(fmax(f0, 0.0), (double)(g.nc[0] - 1));
    f1 = fmin(fmax(f1, 0.0), (double)(g.nc[1] - 1));
    f2 = fmin(fmax(f2, 0.0), (double)(g.nc[2] - 1));
    c0 = (int)f0; // NaN -> fmax(NaN,0)=0
    c1 = (int)f1;
    c2 = (int)f2;
}

// The cell grid as the thread-per-atom and wave-per-atom kernels of neighbor.hip walk it, in either of its two forms.
//   Compact (SLOT = false): position p of the cell order names an atom, a cell is the range [cell_start[c], cell_start[c + 1]) of it,
//     and the three cells of a z-run that does not cross the box's face are ONE range.
//   Slot grid (SLOT = true, CellGrid::slot_cap): cell_start[c] is the cell's COUNT, its first SLOT_CAP ids sit in descending order in
//     the cell's slots of `order` (slot_pos), the cells are walked one by one, a centre is named by its id (p = id: the atoms are the
//     caller's arrays), and a cell whose count ran past SLOT_CAP has the rest of its atoms on the spill list.
// The candidates of a centre — the atoms of the 27 cells around it in the reference's order (neighbor.cpp:147-151), each cell's by
// descending id — come as a sequence of pieces (for_each_piece), a piece being one of
//   a run:              n consecutive positions of the cell order from `at` (compact);
//   a cell's slots:     the n <= SLOT_CAP slot positions of cell `at` (slot grid);
//   an overflowed cell: cell `at` with n > SLOT_CAP atoms, handed out one by one in descending id by next_id_below (slot grid).
// Candidate k of a piece of the first two kinds is read at pos(piece, k).
struct CellPiece { int64_t at; int n; };
template <bool SLOT>
struct CellView {
    SortedView sv;
    const int *__restrict__ cell_start;
    SlotSpill sp; // (a compact grid has none: never read)

    // centres are numbered 0 ... centres() - 1: the atoms the grid holds (cell_start[ncell]: N, or fewer after a windowed build that
    // dropped atoms outside its window — the records behind them were never written); a slot grid takes them by id from the caller's
    // arrays — its atoms are in a spatial order already
    __device__ __forceinline__ int64_t centres(int64_t N, const Grid &g) const { return SLOT ? N : min(N, (int64_t)cell_start[g.ncell]); }
    // centre p: its raw position and its id; -1: an absent atom (slot grid, x = NaN), which has no cell and gets no row
    __device__ __forceinline__ int centre(int64_t p, double &x, double &y, double &z) const
    {
        int id;
        if (SLOT) { id = (int)p; x = sv.xs[p]; y = sv.ys[p]; z = sv.zs[p]; return x == x ? id : -1; }
        sv.get(p, x, y, z, id);
        return id;
    }
    // the pieces of the centre in cell (c0, c1, c2), in candidate order: f(piece) for each
    template <class F>
    __device__ __forceinline__ void for_each_piece(const Grid &g, int c0, int c1, int c2, F &&f) const
    {
        const bool zrun = !SLOT && c2 >= 1 && c2 + 1 < g.nc[2]; // the three z-cells are one contiguous run
        for (int a = c0 - 1; a <= c0 + 1; ++a) {                // neighbor.cpp:147-151
            const int ca = pmod(a, g.nc[0]);
            for (int bb = c1 - 1; bb <= c1 + 1; ++bb) {
                const int64_t base = ((int64_t)ca * g.nc[1] + pmod(bb, g.nc[1])) * g.nc[2];
                for (int seg = 0; seg < (zrun ? 1 : 3); ++seg) {
                    const int64_t cell = base + (zrun ? c2 - 1 : pmod(c2 - 1 + seg, g.nc[2]));
                    if (SLOT) {
                        f(CellPiece{cell, cell_start[cell]});
                    } else {
                        const int s = cell_start[cell];
                        f(CellPiece{s, cell_start[cell + (zrun ? 3 : 1)] - s});
                    }
                }
            }
        }
    }
    __device__ __forceinline__ bool overflowed(const CellPiece &pc) const { return SLOT && pc.n > SLOT_CAP; }
    __device__ __forceinline__ int64_t pos(const CellPiece &pc, int k) const { return SLOT ? slot_pos(pc.at, k, sp.hi) : pc.at + k; }
    // the largest id below `prev` among the atoms of an overflowed cell — its slots and its entries of the spill list — or -1: a
    // selection walk, one pass over the (short) list per candidate; the rare path, and the next build of the signature is a compact one
    __device__ __forceinline__ int next_id_below(int64_t cell, int prev) const
    {
        int best = -1;
        for (int u = 0; u < SLOT_CAP; ++u) {
            const int v = sv.order[slot_pos(cell, u, sp.hi)];
            if (v < prev && v > best) best = v;
        }
        const unsigned ns = *sp.n;
        for (unsigned w = 0; w < ns; ++w) {
            const int2 e = sp.list[w];
            if ((int64_t)e.x == cell && e.y < prev && e.y > best) best = e.y;
        }
        return best;
    }
    // The centres of the cells [z0, z1) of the column that starts at cell `col`, numbered 0, 1, ... as they come: f(p) for number
    // `first` and every `step`-th behind it.  Compact: the z-run of a column is contiguous in the cell order; slot grid: cell by
    // cell, the slots and then the cell's entries of the spill list.
    template <class F>
    __device__ __forceinline__ void for_each_column_centre(int64_t col, int z0, int z1, int first, int step, F &&f) const
    {
        if (SLOT) {
            int seen = 0;
            for (int cz = z0; cz < z1; ++cz) {
                const int n = cell_start[col + cz];
                for (int k = 0; k < n; ++k, ++seen) {
                    if (seen % step != first)
                        continue;
                    const int id = cell_atom(col + cz, k);
                    if (id >= 0) f((int64_t)id);
                }
            }
        } else {
            const int e = cell_start[col + z1];
            for (int p = cell_start[col + z0] + first; p < e; p += step) f((int64_t)p);
        }
    }
    // the k-th atom of a cell of a slot grid, in any fixed order (every atom of the cell once); -1: none
    __device__ __forceinline__ int cell_atom(int64_t cell, int k) const
    {
        if (k < SLOT_CAP)
            return sv.order[slot_pos(cell, k, sp.hi)];
        k -= SLOT_CAP;
        const unsigned ns = *sp.n;
        for (unsigned w = 0; w < ns; ++w) {
            const int2 e = sp.list[w];
            if ((int64_t)e.x == cell && k-- == 0) return e.y;
        }
        return -1;
    }
};

// fills cg.g for the cutoff neighbor search: nc = max(floor(thickness/rc), 3) (neighbor.cpp:203-206)
int neighbor_grid_dims(const DBox &b, double rc, Grid &g);

// What build_cell_grid is asked for
struct GridRequest {
    // SORTED_ARRAYS:      xs, ys, zs, mvs: the atoms as coordinate arrays in cell order (kNN, RDF, Voronoi, the overlap filter)
    // FOR_ROWS:           for neighbor rows: the 32-byte records (CellGrid::pk), or no sorted copy at all (CellGrid::ix)
    // FOR_ROWS_UNORDERED: ... of input the caller knows to come in no spatial order (mdh_spatial_sort): records, moved whole
    enum Atoms { SORTED_ARRAYS, FOR_ROWS, FOR_ROWS_UNORDERED };
    bool wrap_first = false; // wrap a position into the primary cell before binning when any axis is periodic
    bool sort_desc = false;  // every cell's atoms by descending id (reference row order); else as the atomic counters placed them
    const int64_t *sort_key = nullptr; // [N] descending key[id] instead of descending id
    Atoms atoms = SORTED_ARRAYS;
    // FOR_ROWS: width of the rows about to be built (0: not known, or counting; < 0: the signature's last exact width, GridFeedback::width).  Rows of more than 16 slots go to the tile kernel's
    // wide instance, which hides the indirect staging's gathers badly (two or three workgroups per CU): such a build keeps the
    // records (the 12-nearest search's cutoff build, 4.7 atoms per cell, rows of 24: 2.15 ms with records, 2.22 without)
    int row_width = 0;
    // FOR_ROWS: the atoms may also be wanted as a SLOT GRID (CellGrid::slot_cap) where slot_grid_rule() (grid_plan.hpp) allows: every kernel behind
    // neighbor_pass reads both forms
    bool slots_ok = false;
};
// Bins the atoms into cg.g (dims/mode set by the caller: all the build keeps of cg) and produces cell_start/order and the atoms in
// the form plan_grid (grid_plan.hpp) picks for rq; takes the thread's pending window hints (mdh_hint_cell_window,
// mdh_hint_centre_window), whatever the build is for
int build_cell_grid(Scope &sc, const double *x, const double *y, const double *z, int64_t N, const DBox &b, const GridRequest &rq,
                    CellGrid &cg);

// cell_grid.hip: out[0..n] = exclusive prefix sums of in[0..n), out[n] = total
int exclusive_scan_u32(Scope &sc, const unsigned *in, int *out, int64_t n);

} // namespace mdh
