// assign_groups.hpp — which lanes of a 64-atom slice share ONE returning atomic on their cell's counter (k_assign, cell_grid.hip).
//
// The rule, written once for the kernel and for the host (mdh_debug_assign_groups, tests/test_assign_groups.py).  It looks three
// lanes back: the four basis atoms of an fcc lattice cell alternate between two or three grid cells (A B A B, not A A B B), so
// runs of ADJACENT equal lanes are one or two atoms long where the same cell comes again two or three lanes later.
//   1. eq: bit d - 1 set when this lane's cell equals the cell of lane - d (d = 1, 2, 3; same slice, cell >= 0)
//   2. a lane without such a bit is a PRIMARY head
//   3. a lane is a MEMBER of lane - d when bit d - 1 is set and lane - d is a primary head.  There is at most one such d: two
//      primary heads of one cell are more than three lanes apart, or the later one would not be primary
//   4. every other lane is a head of its own with count 1: cell < 0 (it issues no atomic), and lanes whose equal neighbours are
//      all members of a head further away
//   5. a head counts its members among the three lanes behind it; a member's rank is one more than the members of its head
//      in front of it
// A window of three lanes cannot hold a group of more than four: the fifth and later lanes of a long run of ONE cell (input sorted
// by cell, dense cells) would each be a head.  Such runs are what the rule of ADJACENT lanes serves with one atomic (a run of equal
// neighbouring lanes is a group, its first lane the head), so a slice is grouped by both rules and takes, as a whole, the one
// that issues fewer atomics (use_runs).
// Nothing here depends on the input's order for correctness: any sequence of cells gets distinct slots under either rule; an
// ordered one gets them with fewer atomics.
#pragma once
#include <stdint.h>

#ifdef __HIPCC__
#define MDH_AG_HD __host__ __device__ __forceinline__
#else
#define MDH_AG_HD inline
#endif

namespace mdh {
namespace assign_groups {

constexpr int WINDOW = 3;

// step 1: c1, c2, c3 = the cells of lanes - 1, - 2, - 3 (ignored where the lane does not exist)
MDH_AG_HD unsigned equal_bits(int cell, int c1, int c2, int c3, int lane)
{
    if (cell < 0)
        return 0u;
    return (lane >= 1 && c1 == cell ? 1u : 0u) | (lane >= 2 && c2 == cell ? 2u : 0u) | (lane >= 3 && c3 == cell ? 4u : 0u);
}

// step 3: distance to the head this lane is a member of (0: a head itself); primary = the lanes whose equal_bits are 0
MDH_AG_HD int member_distance(unsigned eq, uint64_t primary, int lane)
{
    for (int d = 1; d <= WINDOW; ++d)
        if (((eq >> (d - 1)) & 1u) && ((primary >> (lane - d)) & 1ull)) // (bit d - 1 set implies lane >= d)
            return d;
    return 0;
}

// step 5: m1, m2, m3 = the lanes whose member_distance is 1, 2, 3.  A head (d == 0): *count = atoms of its group, *rank = 0;
// a member: *count = 0, *rank = its place in the group (1 ... count - 1)
MDH_AG_HD void count_and_rank(int d, uint64_t m1, uint64_t m2, uint64_t m3, int lane, int *count, int *rank)
{
    if (d == 0) {
        // (shifted by the lane first, then by the distance: no shift reaches 64; past lane 63 there is nobody)
        *count = 1 + (int)(((m1 >> lane) >> 1) & 1ull) + (int)(((m2 >> lane) >> 2) & 1ull) + (int)(((m3 >> lane) >> 3) & 1ull);
        *rank = 0;
        return;
    }
    const int head = lane - d;
    int r = 1;
    if (d >= 2) r += (int)((m1 >> (head + 1)) & 1ull);
    if (d >= 3) r += (int)((m2 >> (head + 2)) & 1ull);
    *count = 0;
    *rank = r;
}

// the rule of adjacent lanes.  heads = the lanes that start a run (lane 0, a cell other than the lane before's, cell < 0);
// the same three results as above: distance to the head, the head's count, the member's rank
MDH_AG_HD bool starts_run(int cell, int c1, int lane) { return lane == 0 || c1 != cell || cell < 0; }
MDH_AG_HD int run_distance(uint64_t heads, int lane, int *count, int *rank)
{
    const uint64_t upto = heads & ((2ull << lane) - 1ull); // (lane 63: 2 << 63 wraps to 0, minus one: all bits)
    const int first = 63 - __builtin_clzll(upto | 1ull); // head of this lane's run (bit 0 is always set: lane 0 starts a run)
    const uint64_t later = lane == 63 ? 0ull : (heads >> (lane + 1));
    const int last = later ? lane + __builtin_ctzll(later) : 63; // last lane of the run, as seen from its head
    *count = first == lane ? last - lane + 1 : 0;
    *rank = lane - first;
    return lane - first;
}
// which rule the slice takes: atomics (heads with a cell) under the rule of runs and under the window rule
MDH_AG_HD bool use_runs(int run_atomics, int window_atomics) { return run_atomics < window_atomics; }

// the whole rule on one slice, lane by lane: head[l] = lane whose atomic serves lane l, count[l] = what that atomic adds
// (0 for a member), rank[l] = offset of lane l from the value the atomic returns
inline void slice(const int *cells, int *head, int *count, int *rank)
{
    unsigned eq[64];
    int dist[64];
    uint64_t primary = 0, m[WINDOW + 1] = {0, 0, 0, 0};
    for (int l = 0; l < 64; ++l) {
        eq[l] = equal_bits(cells[l], l >= 1 ? cells[l - 1] : 0, l >= 2 ? cells[l - 2] : 0, l >= 3 ? cells[l - 3] : 0, l);
        if (eq[l] == 0) primary |= 1ull << l;
    }
    for (int l = 0; l < 64; ++l) {
        dist[l] = member_distance(eq[l], primary, l);
        m[dist[l]] |= 1ull << l;
    }
    uint64_t starts = 0;
    int run_atomics = 0, window_atomics = 0;
    for (int l = 0; l < 64; ++l) {
        if (starts_run(cells[l], l >= 1 ? cells[l - 1] : 0, l)) { starts |= 1ull << l; run_atomics += cells[l] >= 0; }
        window_atomics += dist[l] == 0 && cells[l] >= 0;
    }
    const bool runs = use_runs(run_atomics, window_atomics);
    for (int l = 0; l < 64; ++l) {
        int d = dist[l];
        if (runs) d = run_distance(starts, l, &count[l], &rank[l]);
        else count_and_rank(d, m[1], m[2], m[3], l, &count[l], &rank[l]);
        head[l] = l - d;
    }
}

} // namespace assign_groups
} // namespace mdh
