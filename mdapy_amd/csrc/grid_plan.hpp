// grid_plan.hpp — what a cell grid build decides before it enqueues anything (build_cell_grid, cell_grid.hip).
//
// The decisions, written once for the build and for the host test (mdh_debug_grid_plan, tests/test_grid_plan.py): plain values in,
// a plain struct out, no HIP call and no HIP type.  build_cell_grid does the I/O — the thread's window hints, the signature's
// feedback record, the pinned words — and hands the values in; what it allocates and enqueues follows from the plan alone.
// Every rule only picks a path: the grid's contents are the same whichever form, sort or window the plan names.
#pragma once
#include <stdint.h>
#include <algorithm>
#include <cmath>

namespace mdh {

// atoms a cell of a slot grid holds in place (two planes of four ids, slot_pos in grid.hpp)
constexpr int SLOT_CAP = 8;

// may this build bin straight into cell slots?  (exported as mdh_debug_slot_grid_rule for the table test)
// ordered: the ix form would be taken; keyed: a sort_key; windowed: a pending cell or centre window; seen: a build of this (N, grid)
// has reported; big: that build saw a cell of more than SLOT_CAP atoms; listed: tiles it listed (-1: not known)
inline bool slot_grid_rule(bool ordered, bool keyed, bool windowed, int row_width, int64_t ncell, int64_t N, bool seen, bool big, int listed)
{
    if (!ordered || keyed || windowed || row_width > 16) return false;
    if (ncell > 2 * N || ncell * SLOT_CAP >= (int64_t(1) << 31)) return false; // (the slots are indexed with 32 bits; 32 bytes a cell)
    return seen && !big && listed == 0;
}

// a window of fractional coordinates along one axis, as hinted (mdh_hint_cell_window, mdh_hint_centre_window)
struct CellWindow { int axis = 0; double lo = 0.0, hi = 0.0; bool set = false; };

struct GridPlanIn {
    // the request (GridRequest, grid.hpp)
    enum Atoms { SORTED_ARRAYS, FOR_ROWS, FOR_ROWS_UNORDERED }; // (GridRequest::Atoms, same values)
    int atoms = SORTED_ARRAYS;
    bool sort_desc = false, keyed = false, slots_ok = false;
    int row_width = 0; // < 0: the record's last exact width
    // the system and its grid
    int64_t N = 0, ncell = 0;
    int nc[3] = {0, 0, 0};
    int mode = 0;
    double rc_inv = 0.0;
    bool tri = false;
    double h0 = 0.0; // box length along axis 0 (DBox::h[0])
    // the thread's pending hints
    CellWindow cells, centre;
    // the pinned words, read by the caller
    int order_word = 0;         // the order hint's word (0 where none was asked for or had)
    bool order_sample = false;  // ... and the hint says that this build is to sample the question again
    int big = -1, listed = -1;  // the record's GridFeedback::BIG and LISTED
    int record_width = 0;       // the record's last exact row width
    // the switches
    bool indirect_on = true, slot_on = true, slot_force = false;

    bool for_rows() const { return atoms != SORTED_ARRAYS; }
    // the I/O the caller does for these values: the signature's record is looked up for ...
    bool has_record() const { return for_rows() && slots_ok; }
    // ... and the order hint is consulted for (a caller that knows its atoms unordered is not asked; small systems never)
    bool asks_order() const { return atoms == FOR_ROWS && N >= (int64_t(1) << 18); }
};

struct GridPlan {
    // ARRAYS:           xs, ys, zs, mvs gathered into cell order
    // RECORDS_GATHERED: the 32-byte records (CellGrid::pk), gathered from the caller's arrays
    // RECORDS_MOVED:    ... written in input order while binning and moved whole (input in no spatial order)
    // INDIRECT:         no sorted copy, the kernels read through `order` (CellGrid::ix)
    // SLOT:             ... and the ids in fixed cell slots: no scan, no scatter (CellGrid::slot_cap)
    enum Form { ARRAYS, RECORDS_GATHERED, RECORDS_MOVED, INDIRECT, SLOT };
    // DENSE: eight lanes per cell (k_sort_cells_dense); CELLS: a thread per cell over the whole grid; PIECES: ... over the window's pieces
    // (a slot grid sorts its slots in place, whatever this says)
    enum Sort { SORT_NONE, SORT_DENSE, SORT_CELLS, SORT_PIECES };
    Form form = ARRAYS;
    bool keeps_history = false; // this build's in-cell sort reports a cell of more than SLOT_CAP atoms to the record (GridFeedback::BIG)
    bool samples_order = false; // k_order_far_flag runs in front of the binning
    bool assign4 = false;       // four atoms per lane in k_assign
    int p0 = 0, p1 = 0, p2 = 0, p3 = 0; // planes [p0, p1) and [p2, p3) of axis 0 hold every atom
    bool windowed = false;      // ... as promised by a cell window: the passes over the grid run over them only
    int win_lo = 0, win_hi = 0; // CellGrid::win_lo, win_hi (a one-piece window; 0, 0: all)
    int cen_lo = 0, cen_hi = 0; // CellGrid::cen_lo, cen_hi (0, 0: all)
    Sort sort = SORT_NONE;
    int row_width = 0;          // the request's, or the record's where the request says so
};

inline GridPlan plan_grid(const GridPlanIn &in)
{
    GridPlan pl;
    const bool packed = in.for_rows();
    const int64_t N = in.N;
    pl.row_width = in.row_width < 0 ? (in.has_record() ? in.record_width : 0) : in.row_width;

    // records moved whole: always for a caller that knows (FOR_ROWS_UNORDERED); for a large system otherwise when the last sample
    // of this (N, grid) said so
    bool scattered = in.atoms == GridPlanIn::FOR_ROWS_UNORDERED;
    if (in.asks_order()) {
        scattered = in.order_word != 0;
        pl.samples_order = in.order_sample;
    }
    // input in some spatial order: no sorted copy (not for dense cells — six atoms and more — nor for rows of more than 16
    // slots: the tile kernel's wide instance hides the staging's dependent gathers badly, profiles/r06_cell_grid_ab.txt)
    const bool indirect = packed && in.indirect_on && !scattered && in.sort_desc && (double)N <= 6.0 * (double)in.ncell && pl.row_width <= 16;
    // The slot grid where the rule allows.  A build that could be one but for its signature's history keeps that history; what
    // the history says arrives when the device gets there: a build that reads an old answer is a slower one, never a wrong one.
    const bool windows = in.cells.set || in.centre.set;
    bool slot = false;
    if (in.has_record() && slot_grid_rule(indirect, in.keyed, windows, pl.row_width, in.ncell, N, true, false, 0)) {
        pl.keeps_history = true;
        slot = in.slot_on && (in.slot_force || slot_grid_rule(indirect, in.keyed, windows, pl.row_width, in.ncell, N, in.big >= 0, in.big > 0, in.listed));
    }
    pl.form = !packed ? GridPlan::ARRAYS : slot ? GridPlan::SLOT : indirect ? GridPlan::INDIRECT : scattered ? GridPlan::RECORDS_MOVED : GridPlan::RECORDS_GATHERED;
    // atoms per lane: four; small systems keep one atom per lane (they need the workgroups to fill the chip), and so does a
    // shuffled frame (10 M runs of one atom, the atomics' own throughput: 413 -> 440 us with four; profiles/r05_assign_k.txt)
    pl.assign4 = N >= (int64_t(1) << 20) && !scattered;

    // window of planes along axis 0 (orthogonal boxes, rc-wide cells): [p0, p1) and, when it wraps around the ring, [p2, p3)
    // (only the neighbor builds know what a window leaves undone; a hint that meets any other grid build is dropped)
    const int n0 = in.nc[0];
    const bool planes_ok = packed && !in.tri && in.mode == 0;
    pl.p1 = n0;
    const CellWindow &w = in.cells;
    if (w.set && planes_ok && w.axis == 0 && n0 >= 16 && w.hi > w.lo && w.hi - w.lo < 0.75) {
        const int lo = (int)std::floor(w.lo * in.h0 * in.rc_inv) - 1, hi = (int)std::ceil(w.hi * in.h0 * in.rc_inv) + 1; // one plane of margin
        if (hi - lo < n0 - 2) {
            pl.windowed = true;
            if (lo < 0) { pl.p0 = 0; pl.p1 = std::min(hi, n0); pl.p2 = n0 + lo; pl.p3 = n0; }   // wraps below
            else if (hi > n0) { pl.p0 = 0; pl.p1 = hi - n0; pl.p2 = lo; pl.p3 = n0; }           // wraps above
            else { pl.p0 = lo; pl.p1 = hi; pl.p2 = pl.p3 = 0; }
            // the pieces meet: everything.  (Looks unreachable: hi - lo < n0 - 2 keeps the two pieces more than two planes apart;
            // kept as it stood)
            if (pl.p2 < pl.p1 && pl.p3 > pl.p2) { pl.windowed = false; pl.p0 = 0; pl.p1 = n0; pl.p2 = pl.p3 = 0; }
        }
    }
    if (pl.windowed && pl.p3 <= pl.p2) { pl.win_lo = pl.p0; pl.win_hi = pl.p1; } // one piece: the tile kernel runs over its range of tiles
    const CellWindow &c = in.centre;
    if (c.set && planes_ok && c.axis == 0 && c.hi > c.lo && c.lo >= 0.0 && c.hi <= 1.0) {
        // the planes an atom of fraction [lo, hi) can be binned into (cell_coords: floor((x - o) rc_inv), clamped); the ends moved
        // out by 1e-9 of their value — far more than the roundings that separate the caller's fraction of an atom from the grid's
        // (x - o) rc_inv, far less than a plane: an atom ON the slab's face is inside whichever way it was rounded
        pl.cen_lo = std::max(0, std::min(n0 - 1, (int)std::floor(c.lo * in.h0 * in.rc_inv * (1.0 - 1e-9) - 1e-9)));
        pl.cen_hi = std::min(n0, (int)std::floor(c.hi * in.h0 * in.rc_inv * (1.0 + 1e-9) + 1e-9) + 1);
    }

    if (!in.sort_desc) pl.sort = GridPlan::SORT_NONE;
    else if (pl.windowed) pl.sort = GridPlan::SORT_PIECES;
    else if (!in.keyed && (double)N > 6.0 * (double)in.ncell) pl.sort = GridPlan::SORT_DENSE; // (11 atoms per cell at rc = 5 A in a metal)
    else pl.sort = GridPlan::SORT_CELLS;
    return pl;
}

} // namespace mdh
