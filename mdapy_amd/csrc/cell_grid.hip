// cell_grid.hip — the cell grid of the cutoff neighbor search, kNN, RDF, Voronoi, the spatial sort and the overlap filter.
//
// Replaces build_cell of the reference (src/neighbor.cpp :64-100) and the cell arithmetic around it.
//
// Scratch in HBM:
//   cell_count u32[ncell] -> cell_start i32[ncell+1] (exclusive scan),
//   ent int2[N] ((cell, slot handed out by the cell's atomic counter) of every atom: k_assign -> k_scatter; afterwards
//                  N ints of scratch for the in-cell sorts),
//   order i32[N]  (atom ids sorted by cell; inside a cell DESCENDING id, the order in which the reference's head-inserted
//                  linked list is walked),
//   xs,ys,zs f64[N] (raw positions gathered into cell order, so a cell's atoms — and the 3 cells of a z-run — are
//                  contiguous and loads are coalesced).
// The slot grid (CellGrid::slot_cap, grid.hpp; neighbor builds of spatially ordered input whose cells were small last time):
//   count u32[ncell] (two arrays in one kept block, alternating from one slot build to the next), slots i32[2][ncell][4] (the ids
//   of a cell where its counter placed them, then sorted in place: k_assign<SLOT> -> k_sort_slots, no scan, no scatter),
//   spill int2[N] + a counter (the atoms of cells that hold more than SLOT_CAP).
// A build (build_cell_grid, at the end of the namespace): the thread's window hints are taken, the signature's feedback record is
// looked up and its pinned words read, plan_grid (grid_plan.hpp: pure, tested on the host) decides the form, the window's planes and
// the in-cell sort from those values, the buffers of that form are allocated, and file-static steps that only enqueue carry the plan
// out: bin_atoms, then finish_slot_grid, or scan_cells, k_scatter, sort_cells, gather_atoms.
#include "common.hpp"
#include "grid.hpp"
#include "assign_groups.hpp"
#include "grid_plan.hpp"
#include <algorithm>
#include <atomic>
#include <mutex>
#include <vector>

namespace mdh {
// 1: neighbor builds of input in spatial order keep no sorted copy of the atoms (CellGrid::ix); 0: the 32-byte records always
static std::atomic<int> g_indirect{[] { const char *e = std::getenv("MDH_INDIRECT"); return e ? std::atoi(e) : 1; }()};

// ----------------------------------------------------------------------------
// cell assignment: wrap, bin, take a slot from the cell's atomic counter
// ----------------------------------------------------------------------------
struct CellPlanes { int p0, p1, p2, p3; int *bad; }; // planes [p0, p1) and [p2, p3) of axis 0 hold every atom (bad == nullptr: not promised; else a pinned host word)
// K atoms per lane: a wave takes 64 * K consecutive atoms as K slices of 64 (slice k: atom base + 64 k + lane, so adjacent lanes
// still hold adjacent atoms and the groups below are found per slice).  The kernel is a chain of dependent memory trips — position
// loads, the returning atomic, the store — at full occupancy (26-38 VGPRs; 87 % of the wave-cycles waiting,
// profiles/r05_step_counters.json): with K > 1 the loads of a lane's K atoms are in flight together, and so are its K atomics.
// One atomic per group of lanes of a cell up to three lanes apart (assign_groups.hpp) and ONE 8-byte store of (cell, slot) per atom:
// 133.8 -> 90-104 us at 10 M lattice atoms (8.23 M -> 6.73 M atomics, the distinct cells per slice; with runs of adjacent lanes and
// two 4-byte stores before), profiles/assign_window.md.
// SLOT (a slot grid, CellGrid::slot_cap): the slot the counter hands out IS the atom's final place — its id goes to
// slots[cell * SLOT_CAP + slot], a scattered 4-byte store in place of the coalesced 8-byte entry, and the scan and the scatter that
// turned the entries into a cell order are not run at all (slots in two planes of four per cell, slot_pos; slot_hi: the second);
// an atom whose cell is full goes to the spill list as (cell, id), the count keeps running so that every reader sees the overflow
template <bool TRI, int K, bool SLOT = false>
__global__ __launch_bounds__(256) void k_assign(const double *__restrict__ x, const double *__restrict__ y,
                                                const double *__restrict__ z, int64_t N, DBox b, Grid g,
                                                int wrap_first, int2 *__restrict__ ent,
                                                unsigned *__restrict__ cell_count, unsigned *__restrict__ ctl, unsigned gen,
                                                double slack, unsigned short *__restrict__ mv, CellPlanes win,
                                                CellGrid::Packed *__restrict__ rec, int drop_absent, int *__restrict__ slots = nullptr,
                                                int2 *__restrict__ spill = nullptr, unsigned *__restrict__ spill_n = nullptr, int64_t slot_hi = 0)
{
    const int lane = threadIdx.x & 63;
    const int64_t i0 = ((int64_t)blockIdx.x * (blockDim.x >> 6) + (threadIdx.x >> 6)) * (64 * K) + lane;
    bool moved = false, outside = false, coded = false;
    double xr[K], yr[K], zr[K];
#pragma unroll
    for (int k = 0; k < K; ++k) { // (all loads of the lane first)
        const int64_t i = i0 + 64 * k;
        xr[k] = yr[k] = zr[k] = 0.0;
        if (i < N) { xr[k] = x[i]; yr[k] = y[i]; zr[k] = z[i]; }
    }
    int cells[K];
#pragma unroll
    for (int k = 0; k < K; ++k) {
        const int64_t i = i0 + 64 * k;
        int cell = -1 - lane; // lanes past the end, absent atoms: negative, no group, no atomic
        // an atom whose x is NaN is ABSENT: it takes no cell, appears in nobody's row and gets no row of its own (the unused slots of a
        // decomposed system's fixed-size ghost block, slab.hip k_slab_append_static; the reference has no meaning for such input)
        // (only the neighbor builds — drop_absent — know what to do without such an atom: their kernels walk cells, and their per-atom
        // passes end at the number of atoms binned; every other user of the grid bins a NaN as it always did, into cell 0)
        const bool absent = drop_absent && i < N && xr[k] != xr[k];
        if (absent && mv) mv[i] = (unsigned short)img::ATOM_NEUTRAL;
        if (i < N && !absent) {
            double xi = xr[k], yi = yr[k], zi = zr[k];
            int code = img::ATOM_NEUTRAL; // (m + 15) per axis: raw = wrapped + m*L
            if (wrap_first && b.anypbc) { // neighbor.cpp:88-91
                wrap<TRI>(b, xi, yi, zi);
                if (!TRI) {
                    // whole box lengths between the raw and the wrapped coordinate (an unwrapped trajectory: a few); more than
                    // img::MAX_M of them, or a coordinate that is not wrapped + m L to within `slack`, invalidates the image codes
                    // for this call (flags[0])
                    const double raw[3] = {xr[k], yr[k], zr[k]}, wrp[3] = {xi, yi, zi};
                    code = 0;
#pragma unroll
                    for (int d = 0; d < 3; ++d) {
                        double m = 0.0;
                        if (b.pbc[d] && raw[d] != wrp[d]) { // already wrapped (the common case): m = 0, no division
                            m = rint((raw[d] - wrp[d]) / b.h[d * 4]);
                            if (!(fabs(m) <= (double)img::MAX_M) || !(fabs(raw[d] - m * b.h[d * 4] - wrp[d]) <= slack)) { moved = true; m = 0.0; }
                        }
                        code |= ((int)m + 15) << (5 * d);
                    }
                }
            }
            if (mv) mv[i] = (unsigned short)code;
            // scattered input (mdh_spatial_sort): the atom as ONE 32-byte record in input order — the gather then reads one random
            // sector per atom instead of three (x, y, z) or four (the image code)
            if (rec) rec[i] = CellGrid::Packed{xr[k], yr[k], zr[k], (int)i, code};
            coded = coded || code != img::ATOM_NEUTRAL;
            int c0, c1, c2;
            cell_coords<TRI>(b, g, xi, yi, zi, c0, c1, c2);
            cell = (c0 * g.nc[1] + c1) * g.nc[2] + c2; // neighbor.cpp:24-27 (ncell < 2^31 checked on the host)
            if (win.bad && !((c0 >= win.p0 && c0 < win.p1) || (c0 >= win.p2 && c0 < win.p3))) {
                // an atom outside the window of planes the caller promised (mdh_hint_cell_window): the counters out there were
                // never zeroed — it takes no slot and is not scattered (cell -1); the build is reported broken (win.bad), its
                // rows are not to be used, and nothing is written out of bounds
                outside = true;
                cell = -1 - lane;
            }
        }
        cells[k] = cell;
    }
    // One returning atomic per GROUP of lanes in the same cell instead of one per atom: atoms usually arrive in some spatial
    // order (a lattice builder, a file written cell by cell, a previous sort), so nearby lanes share cells; the slot inside a
    // cell is arbitrary anyway (k_sort_cells restores the reference's order).  A group is a head and the lanes of its cell up
    // to three behind it (assign_groups.hpp: the basis atoms of an fcc cell alternate between grid cells, A B A B), or, where
    // that makes fewer atomics of the slice, a run of adjacent lanes.  Unordered input pays four shuffles (three up, one from the
    // head) and seven ballots (primary heads, run starts, the two counts of atomics, the members at distance 1, 2, 3).
    unsigned base[K];
    int head[K], slot[K];
#pragma unroll
    for (int k = 0; k < K; ++k) { // (the K atomics of the lane in flight together)
        const int cell = cells[k];
        const int c1 = __shfl_up(cell, 1, 64);
        const unsigned eq = assign_groups::equal_bits(cell, c1, __shfl_up(cell, 2, 64), __shfl_up(cell, 3, 64), lane);
        const unsigned long long primary = __ballot(eq == 0);
        int d = assign_groups::member_distance(eq, primary, lane);
        const bool start = assign_groups::starts_run(cell, c1, lane);
        const unsigned long long starts = __ballot(start);
        int count;
        if (assign_groups::use_runs(__popcll(__ballot(start && cell >= 0)), __popcll(__ballot(d == 0 && cell >= 0)))) // (wave-uniform)
            d = assign_groups::run_distance(starts, lane, &count, &slot[k]);
        else
            assign_groups::count_and_rank(d, __ballot(d == 1), __ballot(d == 2), __ballot(d == 3), lane, &count, &slot[k]);
        head[k] = lane - d;
        base[k] = 0;
        if (d == 0 && cell >= 0)
            base[k] = atomicAdd(&cell_count[cell], (unsigned)count);
    }
#pragma unroll
    for (int k = 0; k < K; ++k) {
        const unsigned bs = __shfl(base[k], head[k], 64);
        const int64_t i = i0 + 64 * k;
        if (SLOT) {
            if (i < N && cells[k] >= 0) {
                const unsigned s = bs + (unsigned)slot[k];
                if (s < (unsigned)SLOT_CAP) slots[slot_pos(cells[k], (int)s, slot_hi)] = (int)i;
                else spill[atomicAdd(spill_n, 1u)] = make_int2(cells[k], (int)i); // (at most one entry per atom: the list holds N)
            }
            continue;
        }
        if (i < N) // (cell < 0: absent, or outside a promised window — k_scatter leaves the atom out)
            ent[i] = make_int2(cells[k], (int)(bs + (unsigned)slot[k]));
    }
    // what this kernel finds out about the input goes into generation-stamped control words (no memset per build): the scan
    // that follows turns them into the build's flags[0] (unwrapped input) and flags[4] (image codes present)
    if (__any(moved) && lane == 0)
        ctl[1] = gen;
    if (__any(coded) && lane == 0)
        ctl[2] = gen; // some atom was handed in outside the box: the gather has to read the image codes (else they are all neutral)
    if (__any(outside) && lane == 0)
        *win.bad = 1; // (pinned host memory: read by the next build of the thread / mdh_cell_window_check)
}

// ----------------------------------------------------------------------------
// exclusive prefix sum of the bin counters (three small kernels)
// ----------------------------------------------------------------------------
static constexpr int SCAN_BLOCK = 256;
static constexpr int SCAN_ITEMS = 4; // per thread -> 1024 per block (small inputs); SCAN_ITEMS_BIG for large ones
static constexpr int SCAN_ITEMS_BIG = 32; // 8192 per block: every block takes a ticket from ONE word, ~90 of them per microsecond —
                                          // with 1024 per block the 3 925 tickets of a 4 M-cell grid were 43 of the scan's 62 us
static constexpr int64_t SCAN_BIG_FROM = 1 << 19; // items from which the big blocks are used

__device__ __forceinline__ unsigned wave_incl_scan(unsigned v, int lane)
{
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
        unsigned t = __shfl_up(v, d, 64);
        if (lane >= d) v += t;
    }
    return v;
}

// block-wide exclusive scan of one value per thread (256 threads = 4 waves); returns exclusive prefix, total via *tot
__device__ __forceinline__ unsigned block_excl_scan(unsigned v, unsigned *tot)
{
    __shared__ unsigned wsum[4];
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    unsigned inc = wave_incl_scan(v, lane);
    if (lane == 63) wsum[w] = inc;
    __syncthreads();
    unsigned off = 0, t = 0;
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        if (k < w) off += wsum[k];
        t += wsum[k];
    }
    __syncthreads();
    *tot = t;
    return off + inc - v;
}

// ----------------------------------------------------------------------------
// Single-pass exclusive scan (decoupled look-back: Merrill & Garland, "Single-pass parallel prefix scan with decoupled
// look-back", NVIDIA NVR-2016-002) — ONE launch instead of three: at a few thousand atoms a build is a chain of dependent
// launches of ~4 us each, whatever they do.  A block takes a ticket (so that every predecessor it waits for is already
// running), scans its 1024 items, publishes its total, and wave 0 collects the totals / inclusive prefixes of the blocks
// before it, 64 at a time.  Control words live in a kept block (Scope::KEEP_SCAN): ctl[0] the ticket counter (reset by
// the block that takes the last ticket), ctl[1], ctl[2] the stamps of k_assign, status words from byte 256 on:
// generation (30 bits) | state (2: 1 = block total, 2 = inclusive prefix) | value (32) — a word of an earlier launch
// carries an older generation and reads as "not there yet", so nothing is cleared between launches.
// REZERO: the input is a build's bin counters in a KEEP_ZERO block: every counter is cleared as it is read.
// flags != nullptr: the first block also writes the build's eight device flags (grid.hpp) from the stamps.
// ----------------------------------------------------------------------------
static std::atomic<unsigned> g_scan_gen{0};
static unsigned next_scan_gen()
{
    unsigned g = (++g_scan_gen) & 0x3fffffffu;
    if (g == 0) { // 2^30 launches: old status words could repeat a generation — start over from clean control blocks
        reset_kept_blocks(Scope::KEEP_SCAN);
        g = (++g_scan_gen) & 0x3fffffffu;
    }
    return g;
}

template <bool REZERO, int ITEMS = SCAN_ITEMS>
__global__ __launch_bounds__(SCAN_BLOCK) void k_scan_onepass(unsigned *__restrict__ in, int *__restrict__ out, int64_t n,
                                                             unsigned *__restrict__ ctl, unsigned gen, int *__restrict__ flags)
{
    constexpr int SCAN_ITEMS = ITEMS; // (shadows the namespace constant: the body below is written for any multiple of four)
    __shared__ unsigned s_blk, s_excl;
    unsigned long long *status = reinterpret_cast<unsigned long long *>(ctl + 64);
    const int tid = threadIdx.x, lane = tid & 63;
    if (tid == 0) s_blk = atomicAdd(&ctl[0], 1u);
    __syncthreads();
    const unsigned blk = s_blk, nblk = gridDim.x;
    if (tid == 0) {
        if (blk == nblk - 1) ctl[0] = 0; // every ticket has been taken: ready for the next launch
        if (blk == 0 && flags) {
            flags[0] = ctl[1] == gen ? 1 : 0; flags[1] = 0; flags[2] = 0; flags[3] = 0;
            flags[4] = ctl[2] == gen ? 1 : 0; flags[5] = 0; flags[6] = 0; flags[7] = 0;
        }
    }
    const int64_t base = ((int64_t)blk * SCAN_BLOCK + tid) * SCAN_ITEMS;
    unsigned v[SCAN_ITEMS], s = 0;
    const bool vec = base + SCAN_ITEMS <= n && ((reinterpret_cast<uintptr_t>(in + base) | reinterpret_cast<uintptr_t>(out + base)) & 15u) == 0;
    if (vec) {
#pragma unroll
        for (int c = 0; c < SCAN_ITEMS / 4; ++c) {
            const uint4 q = reinterpret_cast<const uint4 *>(in + base)[c];
            v[4 * c] = q.x; v[4 * c + 1] = q.y; v[4 * c + 2] = q.z; v[4 * c + 3] = q.w;
        }
        if (REZERO) {
#pragma unroll
            for (int c = 0; c < SCAN_ITEMS / 4; ++c) reinterpret_cast<uint4 *>(in + base)[c] = make_uint4(0u, 0u, 0u, 0u);
        }
    } else {
#pragma unroll
        for (int k = 0; k < SCAN_ITEMS; ++k) {
            v[k] = (base + k < n) ? in[base + k] : 0u;
            if (REZERO && base + k < n) in[base + k] = 0u;
        }
    }
#pragma unroll
    for (int k = 0; k < SCAN_ITEMS; ++k) s += v[k];
    unsigned tot;
    unsigned ex = block_excl_scan(s, &tot);
    const unsigned long long stamp = (unsigned long long)gen << 34;
    if (tid == 0) // this block's total (block 0: its inclusive prefix) for the blocks behind it
        __hip_atomic_store(&status[blk], stamp | ((unsigned long long)(blk == 0 ? 2u : 1u) << 32) | tot, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    if (tid < 64) {
        unsigned excl = 0;
        if (blk > 0) {
            int64_t j = (int64_t)blk - 1; // nearest predecessor
            for (;;) {
                const int64_t idx = j - lane;
                unsigned long long st;
                for (;;) {
                    st = idx >= 0 ? __hip_atomic_load(&status[idx], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) : (stamp | (2ull << 32));
                    const bool there = (st >> 34) == gen && ((st >> 32) & 3u) != 0;
                    if (__all(there))
                        break;
                    __builtin_amdgcn_s_sleep(2);
                }
                const unsigned long long pm = __ballot(((st >> 32) & 3u) == 2u);
                const int first = pm ? __builtin_ctzll(pm) : 64; // nearest block that already knows its inclusive prefix
                unsigned val = lane <= first ? (unsigned)(st & 0xffffffffull) : 0u;
#pragma unroll
                for (int d = 32; d >= 1; d >>= 1) val += __shfl_xor(val, d, 64);
                excl += val;
                if (pm)
                    break;
                j -= 64;
            }
            if (lane == 0)
                __hip_atomic_store(&status[blk], stamp | (2ull << 32) | (unsigned long long)(excl + tot), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        }
        if (lane == 0) s_excl = excl;
    }
    __syncthreads();
    ex += s_excl;
    if (vec) {
#pragma unroll
        for (int c = 0; c < SCAN_ITEMS / 4; ++c) {
            int4 o;
            o.x = (int)ex; o.y = (int)(ex + v[4 * c]); o.z = (int)(ex + v[4 * c] + v[4 * c + 1]); o.w = (int)(ex + v[4 * c] + v[4 * c + 1] + v[4 * c + 2]);
            reinterpret_cast<int4 *>(out + base)[c] = o;
            ex += v[4 * c] + v[4 * c + 1] + v[4 * c + 2] + v[4 * c + 3];
        }
    } else {
#pragma unroll
        for (int k = 0; k < SCAN_ITEMS; ++k) {
            if (base + k < n) out[base + k] = (int)ex;
            ex += v[k];
        }
    }
    if (blk == nblk - 1 && tid == 0) out[n] = (int)(s_excl + tot); // grand total
}

static size_t scan_ctl_bytes(int64_t n)
{
    const int64_t per = (int64_t)SCAN_BLOCK * SCAN_ITEMS;
    return 256 + (size_t)((n + per - 1) / per) * 8;
}
// out[0..n] = exclusive prefix of in[0..n), out[n] = total; rezero: clear in[] on the way (bin counters of a kept block)
static void launch_scan_gen(hipStream_t st, unsigned *in, int *out, int64_t n, unsigned *ctl, unsigned gen, bool rezero, int *flags)
{
    const bool big = n >= SCAN_BIG_FROM;
    const int64_t per = (int64_t)SCAN_BLOCK * (big ? SCAN_ITEMS_BIG : SCAN_ITEMS);
    const dim3 grid((unsigned)std::max<int64_t>(1, (n + per - 1) / per)), block(SCAN_BLOCK);
    if (big) {
        if (rezero) hipLaunchKernelGGL((k_scan_onepass<true, SCAN_ITEMS_BIG>), grid, block, 0, st, in, out, n, ctl, gen, flags);
        else hipLaunchKernelGGL((k_scan_onepass<false, SCAN_ITEMS_BIG>), grid, block, 0, st, in, out, n, ctl, gen, flags);
    } else {
        if (rezero) hipLaunchKernelGGL((k_scan_onepass<true, SCAN_ITEMS>), grid, block, 0, st, in, out, n, ctl, gen, flags);
        else hipLaunchKernelGGL((k_scan_onepass<false, SCAN_ITEMS>), grid, block, 0, st, in, out, n, ctl, gen, flags);
    }
}
static void launch_scan(hipStream_t st, unsigned *in, int *out, int64_t n, unsigned *ctl, bool rezero, int *flags)
{
    launch_scan_gen(st, in, out, n, ctl, next_scan_gen(), rezero, flags);
}

// out[0..n] = exclusive prefix sums of in[0..n) (out[n] = total); for other translation units (grid.hpp)
int exclusive_scan_u32(Scope &sc, const unsigned *in, int *out, int64_t n)
{
    unsigned *ctl = static_cast<unsigned *>(sc.alloc_kept(scan_ctl_bytes(n), Scope::KEEP_SCAN));
    if (sc.failed())
        return sc.error();
    launch_scan(sc.stream(), const_cast<unsigned *>(in), out, n, ctl, false, nullptr);
    MDH_HIP(hipGetLastError());
    return MDH_OK;
}

// ent: (cell, slot inside the cell) of every atom, one 8-byte entry from k_assign.  Two atoms per thread: their entries are ONE
// 16-byte load: 31.9 us at 10 M atoms (8-byte loads run at 0.54-0.70 of the 16-byte rate: one atom per thread took 40.7 us, the two
// separate arrays of ints before that 37.0; profiles/assign_window.md)
__global__ __launch_bounds__(256) void k_scatter(const int2 *__restrict__ ent, const int *__restrict__ cell_start,
                                                 int *__restrict__ order, int64_t N)
{
    const int64_t i = 2 * ((int64_t)blockIdx.x * blockDim.x + threadIdx.x);
    if (i >= N)
        return;
    int4 e; // (ent is 256-byte aligned and i is even: the pair is 16-byte aligned)
    if (i + 1 < N) e = *reinterpret_cast<const int4 *>(ent + i);
    else { const int2 last = ent[i]; e = make_int4(last.x, last.y, -1, 0); }
    if (e.x >= 0) // (< 0: an absent atom, or one outside a promised cell window, k_assign)
        order[cell_start[e.x] + e.y] = (int)i;
    if (e.z >= 0)
        order[cell_start[e.z] + e.w] = (int)(i + 1);
}

// The atomic counters hand out slots in arbitrary order; put every cell's
// atoms into DESCENDING id order (what a walk of the reference's linked list
// sees, neighbor.cpp:97-98) so that rows come out in reference order and the
// result is deterministic.  One thread per cell; cells hold a handful of atoms.
// key != nullptr: descending key[id] instead of descending id (a decomposed system: key = global atom id, so that the rows of
// a slab come out in the order the whole system's rows have)
// Cells of up to eight atoms (nearly all of them at cell width rc) are sorted in registers: the ids, then the keys, loaded as
// one batch, a sorting network with fixed indices, the ids stored back.  The insertion sort below — every comparison a
// dependent read of order[] and, with a key, of key[order[]] — was a chain of 6-10 memory latencies per cell: 32 us of the
// headline build, 77 us of a slab's (random 8-byte key reads).
template <int W, typename K>
__device__ __forceinline__ void sort_cell_net(int *__restrict__ order, int s, int n, const int64_t *__restrict__ key)
{
    int id[W];
    K k[W];
#pragma unroll
    for (int u = 0; u < W; ++u) id[u] = order[s + min(u, n - 1)];
#pragma unroll
    for (int u = 0; u < W; ++u) {
        const K v = key ? (K)key[id[u]] : (K)id[u];
        k[u] = u < n ? v : (sizeof(K) == 8 ? (K)INT64_MIN : (K)INT32_MIN); // pads sink to the end (descending order)
    }
    auto ce = [&](int a, int b) { // k[a] >= k[b] afterwards
        const bool sw = k[a] < k[b];
        const K ka = sw ? k[b] : k[a], kb = sw ? k[a] : k[b];
        const int ia = sw ? id[b] : id[a], ib = sw ? id[a] : id[b];
        k[a] = ka; k[b] = kb; id[a] = ia; id[b] = ib;
    };
    if (W == 4) {
        ce(0, 1); ce(2, 3); ce(0, 2); ce(1, 3); ce(1, 2);
    } else { // Batcher's odd-even merge sort of eight
        ce(0, 1); ce(2, 3); ce(4, 5); ce(6, 7);
        ce(0, 2); ce(1, 3); ce(4, 6); ce(5, 7);
        ce(1, 2); ce(5, 6);
        ce(0, 4); ce(1, 5); ce(2, 6); ce(3, 7);
        ce(2, 4); ce(3, 5);
        ce(1, 2); ce(3, 4); ce(5, 6);
    }
#pragma unroll
    for (int u = 0; u < W; ++u)
        if (u < n) order[s + u] = id[u];
}

// tmp: N ints of scratch indexed like `order` (the entries of k_assign, free once the atoms are scattered), for cells of
// more than eight atoms without a key: the ids are copied there and every atom is PLACED at the number of larger ids of its
// cell — n^2 independent, cached reads instead of the insertion sort's chain of dependent ones (dense cells, rc = 5 A: 11 atoms
// per cell, up to 50 in the fat last cells: 239 -> 204 us at 10 M atoms, 131 -> 94 us at 3.4 M)
// A cell of more than SLOT_CAP atoms, seen by the in-cell sort of a build whose signature may take the slot grid next time: the
// build's generation is stamped into ctl[3] (once per build or nearly: the others find the stamp in L2 and leave) and the cell's
// count goes to the signature's record (GridFeedback::BIG + 1).  The last kernel of the pass over the grid publishes the
// stamp as its word BIG = 1 or 0 (CellGrid::big_sink).
__device__ __forceinline__ void report_big_cell(unsigned *__restrict__ ctl, unsigned gen, int *__restrict__ sink, int n)
{
    if (__hip_atomic_load(&ctl[3], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) == gen)
        return;
    __hip_atomic_store(&ctl[3], gen, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    sink[1] = n;
}

__global__ __launch_bounds__(256) void k_sort_cells(const int *__restrict__ cell_start, int *__restrict__ order,
                                                    int64_t ncell, const int64_t *__restrict__ key, int *__restrict__ tmp,
                                                    unsigned *__restrict__ ctl = nullptr, unsigned gen = 0, int *__restrict__ big_sink = nullptr)
{
    int64_t c = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (c >= ncell)
        return;
    const int s = cell_start[c], e = cell_start[c + 1];
    const int n = e - s;
    if (big_sink && n > SLOT_CAP) report_big_cell(ctl, gen, big_sink, n);
    if (n <= 1)
        return;
    if (n <= 4) {
        if (key) sort_cell_net<4, int64_t>(order, s, n, key);
        else sort_cell_net<4, int>(order, s, n, nullptr);
        return;
    }
    if (n <= 8) {
        if (key) sort_cell_net<8, int64_t>(order, s, n, key);
        else sort_cell_net<8, int>(order, s, n, nullptr);
        return;
    }
    if (!key && tmp) {
        for (int a = s; a < e; ++a) tmp[a] = order[a];
        for (int a = s; a < e; ++a) {
            const int mine = tmp[a];
            int larger = 0;
            for (int q = s; q < e; ++q) larger += tmp[q] > mine ? 1 : 0;
            order[s + larger] = mine; // (ids are distinct: every slot of the cell is written once)
        }
        return;
    }
    for (int a = s + 1; a < e; ++a) {
        int v = order[a], q = a - 1;
        const int64_t kv = key ? key[v] : (int64_t)v;
        while (q >= s && (key ? key[order[q]] : (int64_t)order[q]) < kv) {
            order[q + 1] = order[q];
            --q;
        }
        order[q + 1] = v;
    }
}

// The same order for grids of many atoms per cell (N / ncell > 6: rc = 5 A in a metal, 11 atoms per cell): EIGHT lanes per cell.
// The cell's ids are staged in LDS (64 per cell; a fuller cell is sorted by its first lane as above), then lane l
// ranks the atoms l, l + 8, ... by counting the larger ids of its cell — n / 8 trips of n LDS reads instead of n * n dependent
// global ones in a single lane (rc = 6 A, 18 atoms per cell, 4 M atoms: 240 us, as long as k_assign, k_scatter and k_gather together).
constexpr int SORT_DENSE_CAP = 64;
__global__ __launch_bounds__(256) void k_sort_cells_dense(const int *__restrict__ cell_start, int *__restrict__ order, int64_t ncell,
                                                          int *__restrict__ tmp)
{
    __shared__ int ids[32 * SORT_DENSE_CAP];
    const int sub = threadIdx.x & 7, lc = threadIdx.x >> 3;
    const int64_t c = (int64_t)blockIdx.x * 32 + lc;
    int s = 0, n = 0;
    if (c < ncell) {
        s = cell_start[c];
        n = cell_start[c + 1] - s;
    }
    const bool staged = n > 1 && n <= SORT_DENSE_CAP, big = n > SORT_DENSE_CAP;
    if (staged)
        for (int a = sub; a < n; a += 8) ids[lc * SORT_DENSE_CAP + a] = order[s + a];
    // a fuller cell — the LAST cell of an axis takes the remainder of the box (neighbor.cpp:58-61) and is up to twice as wide: the
    // corner cell of a 256 k-atom box at rc = 5 A holds 84 atoms where the mean is 12 — goes through the free entries of k_assign instead,
    // still eight lanes to the cell (one lane, n * n loads: 330 us for that one cell, as long as the rest of the call)
    if (big)
        for (int a = sub; a < n; a += 8) tmp[s + a] = order[s + a];
    __syncthreads(); // (workgroup scope: the copies in LDS and in HBM are visible to the cell's other lanes)
    if (staged) {
        for (int a = sub; a < n; a += 8) {
            const int mine = ids[lc * SORT_DENSE_CAP + a];
            int larger = 0;
            for (int q = 0; q < n; ++q) larger += ids[lc * SORT_DENSE_CAP + q] > mine ? 1 : 0;
            order[s + larger] = mine; // (ids are distinct: every slot of the cell is written once)
        }
    } else if (big) {
        for (int a = sub; a < n; a += 8) {
            const int mine = tmp[s + a];
            int larger = 0;
            for (int q = 0; q < n; ++q) larger += tmp[s + q] > mine ? 1 : 0;
            order[s + larger] = mine;
        }
    }
}

// The in-cell sort of a slot grid, one thread per cell: the cell's ids as one or two 16-byte loads (one per plane), the networks above in
// registers (descending; the slots behind the count sink to the end and are stored back as they fall, nobody reads them), one or
// two 16-byte stores.  A cell whose count ran past SLOT_CAP sorts its first SLOT_CAP ids; the walkers merge the spill list in
// (neighbor.hip), and the build is reported (report_big_cell) so that the next one of this signature is a compact one.
// On the way: the words [0, idle_n) of the OTHER counter array — the previous slot build's counts, which nobody reads any more —
// are cleared for the next build (Scope::KEEP_SLOT), and the first thread writes the build's eight device flags from the stamps
// of k_assign, as the scan of a compact build does.
__global__ __launch_bounds__(256) void k_sort_slots(const unsigned *__restrict__ count, int *__restrict__ slots, int64_t ncell,
                                                    unsigned *__restrict__ idle, int64_t idle_n, unsigned *__restrict__ ctl, unsigned gen,
                                                    int *__restrict__ big_sink, int *__restrict__ flags, int64_t slot_hi)
{
    const int64_t c = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (c == 0) {
        flags[0] = ctl[1] == gen ? 1 : 0; flags[1] = 0; flags[2] = 0; flags[3] = 0;
        flags[4] = ctl[2] == gen ? 1 : 0; flags[5] = 0; flags[6] = 0; flags[7] = 0;
    }
    if (c < idle_n) idle[c] = 0u;
    if (c >= ncell)
        return;
    const int full = (int)count[c];
    if (full > SLOT_CAP) report_big_cell(ctl, gen, big_sink, full);
    const int n = min(full, SLOT_CAP);
    if (n <= 1)
        return;
    int4 *cell = reinterpret_cast<int4 *>(slots + 4 * c), *cell_hi = reinterpret_cast<int4 *>(slots + slot_hi + 4 * c); // (slots is 256-byte aligned, slot_hi a multiple of four)
    auto ce = [](int &a, int &b) { const int hi = max(a, b), lo = min(a, b); a = hi; b = lo; }; // a >= b afterwards
    int4 q0 = cell[0];
    int id[8] = {q0.x, n > 1 ? q0.y : INT32_MIN, n > 2 ? q0.z : INT32_MIN, n > 3 ? q0.w : INT32_MIN, INT32_MIN, INT32_MIN, INT32_MIN, INT32_MIN};
    if (SLOT_CAP == 4 || n <= 4) {
        ce(id[0], id[1]); ce(id[2], id[3]); ce(id[0], id[2]); ce(id[1], id[3]); ce(id[1], id[2]);
        cell[0] = make_int4(id[0], id[1], id[2], id[3]);
        return;
    }
    const int4 q1 = cell_hi[0];
    id[4] = q1.x; id[5] = n > 5 ? q1.y : INT32_MIN; id[6] = n > 6 ? q1.z : INT32_MIN; id[7] = n > 7 ? q1.w : INT32_MIN;
    ce(id[0], id[1]); ce(id[2], id[3]); ce(id[4], id[5]); ce(id[6], id[7]); // Batcher's odd-even merge sort of eight (sort_cell_net)
    ce(id[0], id[2]); ce(id[1], id[3]); ce(id[4], id[6]); ce(id[5], id[7]);
    ce(id[1], id[2]); ce(id[5], id[6]);
    ce(id[0], id[4]); ce(id[1], id[5]); ce(id[2], id[6]); ce(id[3], id[7]);
    ce(id[2], id[4]); ce(id[3], id[5]);
    ce(id[1], id[2]); ce(id[3], id[4]); ce(id[5], id[6]);
    cell[0] = make_int4(id[0], id[1], id[2], id[3]);
    cell_hi[0] = make_int4(id[4], id[5], id[6], id[7]);
}

__global__ __launch_bounds__(256) void k_gather(const double *__restrict__ x, const double *__restrict__ y,
                                                const double *__restrict__ z, const int *__restrict__ order,
                                                double *__restrict__ xs, double *__restrict__ ys,
                                                double *__restrict__ zs, int64_t N,
                                                const unsigned short *__restrict__ mv, unsigned short *__restrict__ mvs,
                                                CellGrid::Packed *__restrict__ pk, const int *__restrict__ any_code,
                                                const int *__restrict__ n_binned)
{
    int64_t p = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (p >= N)
        return;
    if (n_binned && p >= *n_binned) // a windowed build that dropped atoms outside its window: order[] ends at the atoms binned
        return;
    const int i = order[p];

    const double a = x[i], b = y[i], c = z[i];
    // the image codes are a fourth scattered read per atom (one byte each); k_assign says whether any of them is not neutral
    const unsigned short m = *any_code ? mv[i] : (unsigned short)img::ATOM_NEUTRAL;
    if (pk) {
        pk[p] = CellGrid::Packed{a, b, c, i, (int)m};
        return;
    }
    xs[p] = a;
    ys[p] = b;
    zs[p] = c;
    mvs[p] = m;
}

// the gather of scattered input: whole records (written in input order by k_assign), one random 32-byte read per atom
__global__ __launch_bounds__(256) void k_gather_records(const CellGrid::Packed *__restrict__ rec, const int *__restrict__ order,
                                                        CellGrid::Packed *__restrict__ pk, int64_t N, const int *__restrict__ n_binned)
{
    const int64_t p = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (p >= N || p >= *n_binned)
        return;
    pk[p] = rec[order[p]];
}

__global__ __launch_bounds__(256) void k_unpack(const CellGrid::Packed *__restrict__ pk, int64_t N, double *__restrict__ xs,
                                                double *__restrict__ ys, double *__restrict__ zs, unsigned short *__restrict__ mvs)
{
    const int64_t p = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (p >= N)
        return;
    const CellGrid::Packed r = pk[p];
    xs[p] = r.x; ys[p] = r.y; zs[p] = r.z; mvs[p] = (unsigned short)r.code;
}

int ensure_unpacked(Scope &sc, CellGrid &cg, int64_t N)
{
    if ((!cg.pk && !cg.ix) || cg.xs)
        return MDH_OK;
    cg.xs = sc.alloc_n<double>((size_t)N);
    cg.ys = sc.alloc_n<double>((size_t)N);
    cg.zs = sc.alloc_n<double>((size_t)N);
    cg.mvs = sc.alloc_n<unsigned short>((size_t)N);
    if (sc.failed())
        return sc.error();
    if (cg.pk) // from the records
        hipLaunchKernelGGL(k_unpack, dim3(grid_for(N, 256)), dim3(256), 0, sc.stream(), cg.pk, N, cg.xs, cg.ys, cg.zs, cg.mvs);
    else // an indirect grid: the gather its build left out
        hipLaunchKernelGGL(k_gather, dim3(grid_for(N, 256)), dim3(256), 0, sc.stream(), cg.ix, cg.iy, cg.iz, cg.order, cg.xs, cg.ys, cg.zs, N, cg.imv,
                           cg.mvs, (CellGrid::Packed *)nullptr, cg.flags + 4, cg.cell_start + cg.g.ncell);
    MDH_HIP(hipGetLastError());
    return MDH_OK;
}

// ----------------------------------------------------------------------------
// Cell window (decomposed systems).  A rank's atoms — its slab and the halo — occupy a few planes of the GLOBAL cell grid the
// neighbor build works on (global box, global cells: the rows equal the undivided system's), and the passes over ALL cells
// (bin counters zeroed, three scan kernels, the in-cell sort) then cost more than the passes over the atoms.  The caller, who
// knows where its atoms are, promises a window of fractional coordinates along one axis (mdh_hint_cell_window, consumed by
// the next build on this thread); those passes run over the window's planes (one more on each side) only, and the prefix
// array outside them is filled with the constants a full scan would have left there, so that every reader of cell_start is
// served as before.  An atom binned outside the promised window breaks the promise: counted on the device, reported by
// the next call of this thread that builds a grid.
// ----------------------------------------------------------------------------
// The hints for the NEXT grid build of this thread: the window, and inside it the stretch that holds the atoms whose rows are wanted
// (mdh_hint_centre_window: a rank's OWN slab; what lies between it and the window's ends are ghosts — candidates of the tile
// kernel, never its centres: their rows are not made)
struct PendingWindows { CellWindow cells, centre; };
static thread_local PendingWindows g_pending;
static thread_local int *g_window_violations = nullptr; // pinned host word of the previous windowed build

// The top of every grid build: the thread's hints are taken (and with that spent, whatever the build is for), and a promise the
// previous windowed build found broken is reported
static int take_pending_windows(PendingWindows &w)
{
    w = g_pending;
    g_pending = PendingWindows{};
    if (g_window_violations && *(volatile int *)g_window_violations != 0) {
        *g_window_violations = 0;
        set_error("an earlier neighbor build on this thread found atoms outside the cell window it had been promised (mdh_hint_cell_window)");
        return MDH_ERR_ARG;
    }
    return MDH_OK;
}

// out[a..b) = *v (a value that is on the device only)
// (16-byte stores over the aligned middle — the region behind a slab's window is most of the global grid, 100 MB on eight ranks —
// launched by fill_from() below)
__global__ __launch_bounds__(256) void k_fill_from(int *__restrict__ out, int64_t a, int64_t b, const int *__restrict__ v)
{
    const int val = *v;
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (b - a < 8) {
        if (a + i < b) out[a + i] = val;
        return;
    }
    const int64_t a4 = (a + 3) & ~(int64_t)3, b4 = b & ~(int64_t)3; // a4 <= b4: out is 16-byte aligned at multiples of four
    const int64_t q = a4 + 4 * i;
    if (q + 4 <= b4) *reinterpret_cast<int4 *>(out + q) = make_int4(val, val, val, val);
    if (i < 4) {
        if (a + i < a4) out[a + i] = val;
        if (b4 + i < b) out[b4 + i] = val;
    }
}
// a one-piece window [a0, a1] of the grid: zeros in front of it, *v (the atoms binned, cell_start[a1]) behind it — ONE launch behind
// the window's scan instead of a memset in front of it and a fill behind (a memset is two 5 us nodes on the stream)
__global__ __launch_bounds__(256) void k_fill_outside(int *__restrict__ out, int64_t a0, int64_t a1, int64_t n1, const int *__restrict__ v)
{
    const int val = *v;
    const int64_t q = 4 * ((int64_t)blockIdx.x * blockDim.x + threadIdx.x);
    const int64_t head4 = (a0 + 3) >> 2 << 2;               // the head [0, a0) rounded up to whole quads (the overshoot is fixed below)
    const int64_t t0 = (a1 + 1 + 3) & ~(int64_t)3;          // first aligned index behind the window
    if (q < head4) {
        if (q + 4 <= a0) *reinterpret_cast<int4 *>(out + q) = make_int4(0, 0, 0, 0);
        else for (int64_t i = q; i < a0; ++i) out[i] = 0;
        return;
    }
    const int64_t r = q - head4 + t0;                       // quads behind the window
    if (r == t0) for (int64_t i = a1 + 1; i < t0 && i < n1; ++i) out[i] = val;
    if (r + 4 <= n1) *reinterpret_cast<int4 *>(out + r) = make_int4(val, val, val, val);
    else for (int64_t i = r; i < n1; ++i) out[i] = val;
}
static void fill_from(hipStream_t st, int *out, int64_t a, int64_t b, const int *v)
{
    if (b > a)
        hipLaunchKernelGGL(k_fill_from, dim3(grid_for((b - a) / 4 + 8, 256)), dim3(256), 0, st, out, a, b, v);
}

// out[a..b) += *v  (v outside [a, b)); the entry `skip`, if in range, is left alone
__global__ __launch_bounds__(256) void k_add_from(int *__restrict__ out, int64_t a, int64_t b, const int *__restrict__ v, int64_t skip)
{
    const int64_t i = a + (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i < b && i != skip) out[i] += *v;
}

// atoms binned outside planes [p0, p1) u [p2, p3) of axis 0 (cells are a0-major)
int neighbor_grid_dims(const DBox &b, double rc, Grid &g)
{
    double nc_total = 1.0;
    for (int d = 0; d < 3; ++d) { // neighbor.cpp:203-206
        double f = std::floor(b.thick[d] / rc);
        if (!(f < 2147483647.0)) { set_error("cell grid too large (box thickness / rc overflows int)"); return MDH_ERR_ARG; }
        int n = (int)f;
        g.nc[d] = n > 3 ? n : 3;
        nc_total *= (double)g.nc[d];
    }
    if (nc_total > 2147483000.0) {
        set_error("cell grid too large: " + std::to_string(nc_total) + " cells (the reference indexes cells with int32)");
        return MDH_ERR_ARG;
    }
    g.ncell = (int64_t)g.nc[0] * g.nc[1] * g.nc[2];
    g.rc_inv = 1.0 / rc; // neighbor.cpp:78
    g.mode = 0;
    return MDH_OK;
}

// Do the atoms come in a spatial order?  One workgroup samples 1 024 pairs of consecutive atoms (i, i+1): far = more than two
// bins of ~64 atoms apart along some axis (fractional coordinates, periodic axes wrapped); more than a quarter far -> *flag = 1 (a word
// of pinned host memory, order_hint()): the NEXT builds of this (N, grid) move whole 32-byte records (k_assign writes them in input
// order, the gather reads one random sector per atom instead of three or four: 598 -> ~250 us at 10 M shuffled atoms).  A lattice
// builder's order, a file written cell by cell, a sorted copy: 0.  Launched on the first and every eighth build of a signature.
__global__ __launch_bounds__(1024) void k_order_far_flag(const double *__restrict__ x, const double *__restrict__ y, const double *__restrict__ z,
                                                         int64_t N, DBox b, double nb0, double nb1, double nb2, int *__restrict__ flag)
{
    __shared__ int s_far;
    if (threadIdx.x == 0) s_far = 0;
    __syncthreads();
    const int64_t step = (N - 1) / 1024 > 0 ? (N - 1) / 1024 : 1;
    const int64_t i = (int64_t)threadIdx.x * step;
    bool far = false;
    if (i + 1 < N) {
        const double dx = x[i + 1] - x[i], dy = y[i + 1] - y[i], dz = z[i + 1] - z[i];
        double f[3] = {dx * b.hi[0] + dy * b.hi[3] + dz * b.hi[6], dx * b.hi[1] + dy * b.hi[4] + dz * b.hi[7], dx * b.hi[2] + dy * b.hi[5] + dz * b.hi[8]};
        const double nb[3] = {nb0, nb1, nb2};
#pragma unroll
        for (int d = 0; d < 3; ++d) {
            if (b.pbc[d]) f[d] -= rint(f[d]);
            far = far || !(fabs(f[d]) * nb[d] <= 2.0); // (NaN counts as far)
        }
    }
    const unsigned long long m = __ballot(far);
    if ((threadIdx.x & 63) == 0 && m) atomicAdd(&s_far, __popcll(m));
    __syncthreads();
    if (threadIdx.x == 0) *flag = 4 * s_far > 1024 ? 1 : 0;
}

// ----------------------------------------------------------------------------
// The slot grid's host state
// ----------------------------------------------------------------------------
// 1: neighbor builds may bin straight into cell slots (CellGrid::slot_cap); 0: the compact grid always (mdh_debug_set_slot_grid)
static std::atomic<int> g_slot_grid{[] { const char *e = std::getenv("MDH_SLOT_GRID"); return e ? std::atoi(e) : 1; }()};
// MDH_SLOT_GRID_FORCE=1 (a measuring switch, profiles/slot_grid.md): the slot grid wherever its layout allows, whatever the history
// says — what a build that meets full cells costs (spill list, listed tiles, the thread-per-atom mop-up); results are the same
static const bool g_slot_force = [] { const char *e = std::getenv("MDH_SLOT_GRID_FORCE"); return e && std::atoi(e) != 0; }();
static std::atomic<int> g_last_form{GridPlan::ARRAYS}; // the form the last grid build of the process was planned in (mdh_debug_neighbor_plan)
int last_grid_was_slot() { return g_last_form.load(std::memory_order_relaxed) == GridPlan::SLOT; }
static std::mutex g_slot_mu; // the two tables below: their lookups and hand-overs only, never across a launch, a copy or a wait
// per KEEP_SLOT block: the half the next slot build counts into (all zero) and the words of each half that are not zero
struct SlotBlock { void *p; int next; int64_t dirty[2]; };
static std::vector<GridFeedback *> g_feedback; // per (N, grid, device), grid.hpp: at most 64, the oldest first
static std::atomic<GridFeedback *> g_last_hist{nullptr}; // the signature of the last build that kept a history (mdh_debug_slot_grid_counters)
static std::vector<SlotBlock *> g_slot_blocks;

// the signature's record, made on first sight with nothing known.  (Two threads that meet the same fresh signature get the same
// record and may both count its statistics into it, grid_stats_hint: the same numbers twice.)
static int grid_feedback(int64_t N, int64_t ncell, GridFeedback **out)
{
    int device = 0;
    (void)hipGetDevice(&device);
    std::lock_guard<std::mutex> lk(g_slot_mu);
    for (GridFeedback *f : g_feedback)
        if (f->N == N && f->ncell == ncell && f->device == device) { *out = f; return MDH_OK; }
    GridFeedback *f = nullptr;
    if (g_feedback.size() >= 64) {
        // the oldest signature hands its record and its pinned block on.  A build of that old signature may still be in flight and
        // write its answers into them (a copy enqueued on some other stream may still land, too): the new signature then reads a
        // wrong hint or a wrong history once, which picks a path, never a result
        f = g_feedback.front();
        g_feedback.erase(g_feedback.begin());
    } else {
        int *host = nullptr;
        MDH_HIP(hipHostMalloc(reinterpret_cast<void **>(&host), GridFeedback::WORDS * sizeof(int), hipHostMallocDefault));
        f = new GridFeedback{};
        f->host = host;
    }
    f->N = N; f->ncell = ncell; f->device = device;
    std::fill(f->host, f->host + GridFeedback::WORDS, 0);
    f->host[GridFeedback::LISTED] = f->host[GridFeedback::BIG] = -1;
    f->width = 0; f->calls = 0;
    g_feedback.push_back(f);
    *out = f;
    return MDH_OK;
}
static SlotBlock *slot_block_state(void *p)
{
    std::lock_guard<std::mutex> lk(g_slot_mu);
    for (SlotBlock *b : g_slot_blocks)
        if (b->p == p) return b;
    // (a kept block starts zero-filled.  Entries are never removed, not even when mdh_release_workspace frees the block: one per
    // distinct block address, and an address that comes back names a new, zero-filled block, for which any entry is right — its
    // "dirty" extent only makes the next sort clear more than it has to, within the block: build_cell_grid clamps it)
    g_slot_blocks.push_back(new SlotBlock{p, 0, {0, 0}});
    return g_slot_blocks.back();
}

// ----------------------------------------------------------------------------
// The build: take the hints, look up the record, read the words, plan (grid_plan.hpp), allocate for the plan's form, enqueue.
// The steps below only enqueue; what they share is one GridBuild.
// ----------------------------------------------------------------------------
static_assert((int)GridRequest::SORTED_ARRAYS == GridPlanIn::SORTED_ARRAYS && (int)GridRequest::FOR_ROWS == GridPlanIn::FOR_ROWS &&
              (int)GridRequest::FOR_ROWS_UNORDERED == GridPlanIn::FOR_ROWS_UNORDERED, "GridPlanIn::Atoms mirrors GridRequest::Atoms");

struct GridBuild {
    hipStream_t st;
    const double *x, *y, *z;
    int64_t N;
    const DBox &b;
    const GridRequest &rq;
    GridPlan pl;
    unsigned gen = 0; // stamps of this build's k_assign; the (first) scan is launched with the same value
    // bin counters in a kept block (all zero whenever idle: the scan clears what it reads), the scan's control words in
    // another; the eight device flags are plain scratch, written by the scan — a build enqueues no hipMemsetAsync
    unsigned *cell_count = nullptr, *ctl = nullptr;
    int2 *ent = nullptr;          // (cell, slot) of every atom: k_assign -> k_scatter; afterwards the N ints of scratch of the in-cell sorts; a slot build: its spill list
    unsigned short *mv = nullptr; // image codes in input order
    CellGrid::Packed *rec = nullptr; // records in input order (GridPlan::RECORDS_MOVED)
    int *hist = nullptr;          // != nullptr: this build keeps the history (the record's two words from BIG on)
    int *bad = nullptr;           // != nullptr: a windowed build's pinned word for atoms outside the promise
    // a slot build: the half of a KEEP_SLOT block that the previous slot build's sort cleared, 64 words of header — [0] the length
    // of the spill list — and the counters behind them (cell_count); the other half, which this build's sort clears
    unsigned *slot_block = nullptr, *slot_idle = nullptr;
    int64_t slot_idle_n = 0;
    SlotBlock *sb = nullptr;
    bool slot() const { return pl.form == GridPlan::SLOT; }
};

// the values plan_grid decides by: the request, the grid, the hints, and the words read from the signature's record (cg.fb, looked
// up here: the passes over the grid reach it through cg.fb) and from the order hint (*order_word: where a sample would go)
static int read_plan_inputs(const GridRequest &rq, int64_t N, const DBox &b, const double *x, const PendingWindows &hints, CellGrid &cg,
                            GridPlanIn &in, int **order_word)
{
    const Grid &g = cg.g;
    in.atoms = (int)rq.atoms; in.sort_desc = rq.sort_desc; in.keyed = rq.sort_key != nullptr; in.slots_ok = rq.slots_ok; in.row_width = rq.row_width;
    in.N = N; in.ncell = g.ncell; in.mode = g.mode; in.rc_inv = g.rc_inv; in.tri = b.tri; in.h0 = b.h[0];
    for (int d = 0; d < 3; ++d) in.nc[d] = g.nc[d];
    in.cells = hints.cells; in.centre = hints.centre;
    in.indirect_on = g_indirect.load(std::memory_order_relaxed) != 0;
    in.slot_on = g_slot_grid.load(std::memory_order_relaxed) != 0;
    in.slot_force = g_slot_force;
    if (in.has_record()) {
        MDH_TRY(grid_feedback(N, g.ncell, &cg.fb));
        const volatile int *host = cg.fb->host;
        in.big = host[GridFeedback::BIG]; in.listed = host[GridFeedback::LISTED];
        in.record_width = cg.fb->width.load(std::memory_order_relaxed);
    }
    if (in.asks_order()) {
        const OrderHint h = order_hint(1, N, g.ncell, x);
        if (h.word) { in.order_word = *(volatile int *)h.word; in.order_sample = h.sample; *order_word = h.word; }
    }
    return MDH_OK;
}

static int allocate_grid(Scope &sc, GridBuild &bd, CellGrid &cg)
{
    const Grid &g = cg.g;
    const size_t N = (size_t)bd.N;
    if (bd.slot()) {
        // (+ 64 words behind the counts: the tile kernel reads a cell's count with the word behind it)
        bd.slot_block = static_cast<unsigned *>(sc.alloc_kept(2 * sizeof(unsigned) * (size_t)(g.ncell + 128), Scope::KEEP_SLOT));
        if (bd.slot_block) {
            const size_t half = sc.held_bytes(bd.slot_block) / 8; // words of a half (a block is a multiple of 256 bytes)
            bd.sb = slot_block_state(bd.slot_block);
            bd.cell_count = bd.slot_block + (size_t)bd.sb->next * half + 64;
            bd.slot_idle = bd.slot_block + (size_t)(1 - bd.sb->next) * half;
            bd.slot_idle_n = std::min<int64_t>(bd.sb->dirty[1 - bd.sb->next], (int64_t)half); // (a freed block's address may come back as a smaller, zero-filled one)
        }
        cg.slot_hi = 4 * g.ncell; // where the second plane of four slots per cell starts
    } else {
        bd.cell_count = static_cast<unsigned *>(sc.alloc_kept(sizeof(unsigned) * (size_t)g.ncell, Scope::KEEP_ZERO));
    }
    bd.ctl = static_cast<unsigned *>(sc.alloc_kept(scan_ctl_bytes(g.ncell), Scope::KEEP_SCAN));
    cg.flags = sc.alloc_n<int>(8);
    // a slot grid has no entries, no prefix array and counters of its own
    cg.cell_start = bd.slot() ? reinterpret_cast<int *>(bd.cell_count) : sc.alloc_n<int>((size_t)g.ncell + 1);
    bd.ent = sc.alloc_n<int2>(N);
    // (four spare entries: the tile kernel reads a cell's first four ids as one 16-byte request)
    cg.order = sc.alloc_n<int>(bd.slot() ? (size_t)g.ncell * SLOT_CAP + 4 : N + 4);
    bd.mv = sc.alloc_n<unsigned short>(N);
    switch (bd.pl.form) {
    case GridPlan::ARRAYS:
        cg.xs = sc.alloc_n<double>(N);
        cg.ys = sc.alloc_n<double>(N);
        cg.zs = sc.alloc_n<double>(N);
        cg.mvs = sc.alloc_n<unsigned short>(N);
        break;
    case GridPlan::RECORDS_GATHERED: cg.pk = sc.alloc_n<CellGrid::Packed>(N); break;
    case GridPlan::RECORDS_MOVED: cg.pk = sc.alloc_n<CellGrid::Packed>(N); bd.rec = sc.alloc_n<CellGrid::Packed>(N); break;
    case GridPlan::INDIRECT: case GridPlan::SLOT: break; // no sorted copy
    }
    return sc.failed() ? sc.error() : MDH_OK;
}

// the order question (k_order_far_flag), asked again: the answer lands in the hint's pinned word for the NEXT builds
static void sample_order(const GridBuild &bd, int *word)
{
    const double *h = bd.b.h;
    const double vol = std::fabs(h[0] * (h[4] * h[8] - h[5] * h[7]) - h[1] * (h[3] * h[8] - h[5] * h[6]) + h[2] * (h[3] * h[7] - h[4] * h[6]));
    const double edge = std::cbrt(64.0 * vol / (double)bd.N);
    double nb[3];
    for (int d = 0; d < 3; ++d) nb[d] = std::max(1.0, std::floor(bd.b.thick[d] / edge));
    hipLaunchKernelGGL(k_order_far_flag, dim3(1), dim3(1024), 0, bd.st, bd.x, bd.y, bd.z, bd.N, bd.b, nb[0], nb[1], nb[2], word);
}

// binning: every atom takes a slot from its cell's counter — an entry (cell, slot) for the scan and the scatter, or, a slot grid,
// its id straight into the cell's slots (cg.order) and the spill list (ent; its length in the header word in front of the counts)
template <bool TRI, int K, bool SLOT>
static void launch_assign(const GridBuild &bd, const CellGrid &cg)
{
    const Grid &g = cg.g;
    // slack for the raw-vs-wrapped consistency flag: far above rounding, far below a cell width
    const double slack = 0.01 / (g.rc_inv > 0 ? g.rc_inv : 1.0);
    // the promise is checked where the atoms are binned (a word of pinned host memory the kernel writes) and read by the next
    // build of this thread or by mdh_cell_window_check
    const CellPlanes win{bd.pl.p0, bd.pl.p1, bd.pl.p2, bd.pl.p3, bd.bad};
    int2 *const ent = SLOT ? nullptr : bd.ent, *const spill = SLOT ? bd.ent : nullptr;
    int *const slots = SLOT ? cg.order : nullptr;
    unsigned *const spill_n = SLOT ? bd.cell_count - 64 : nullptr;
    hipLaunchKernelGGL((k_assign<TRI, K, SLOT>), dim3(grid_for(bd.N, 256 * K)), dim3(256), 0, bd.st, bd.x, bd.y, bd.z, bd.N, bd.b, g, (int)bd.rq.wrap_first,
                       ent, bd.cell_count, bd.ctl, bd.gen, slack, bd.mv, win, bd.rec, bd.pl.form != GridPlan::ARRAYS ? 1 : 0, slots, spill, spill_n,
                       SLOT ? cg.slot_hi : (int64_t)0);
}
static void bin_atoms(const GridBuild &bd, const CellGrid &cg)
{
    switch ((bd.b.tri ? 4 : 0) | (bd.pl.assign4 ? 2 : 0) | (bd.slot() ? 1 : 0)) {
    case 0: launch_assign<false, 1, false>(bd, cg); break;
    case 1: launch_assign<false, 1, true>(bd, cg); break;
    case 2: launch_assign<false, 4, false>(bd, cg); break;
    case 3: launch_assign<false, 4, true>(bd, cg); break;
    case 4: launch_assign<true, 1, false>(bd, cg); break;
    case 5: launch_assign<true, 1, true>(bd, cg); break;
    case 6: launch_assign<true, 4, false>(bd, cg); break;
    case 7: launch_assign<true, 4, true>(bd, cg); break;
    }
}

// a slot grid: sort in place, done — no scan, no scatter, no gather (the atoms stay where the caller has them, CellGrid::ix)
static int finish_slot_grid(Scope &sc, const GridBuild &bd, CellGrid &cg)
{
    const Grid &g = cg.g;
    hipLaunchKernelGGL(k_sort_slots, dim3(grid_for(std::max<int64_t>(g.ncell, bd.slot_idle_n), 256)), dim3(256), 0, bd.st, bd.cell_count, cg.order, g.ncell,
                       bd.slot_idle, bd.slot_idle_n, bd.ctl, bd.gen, bd.hist, cg.flags, cg.slot_hi);
    MDH_HIP(hipGetLastError());
    {
        std::lock_guard<std::mutex> lk(g_slot_mu);
        SlotBlock *sb = bd.sb;
        sb->dirty[1 - sb->next] = 0;          // cleared by the sort above
        sb->dirty[sb->next] = g.ncell + 64;   // this build's header and counts: read until the next slot build's sort clears them
        sb->next = 1 - sb->next;
    }
    sc.keep_confirm(bd.slot_block);
    cg.big_stamp = bd.ctl + 3; cg.big_gen = bd.gen; cg.big_sink = bd.hist;
    cg.slot_cap = SLOT_CAP;
    cg.spill = bd.ent;
    cg.n_spill = bd.cell_count - 64;
    cg.ix = bd.x; cg.iy = bd.y; cg.iz = bd.z; cg.imv = bd.mv;
    return MDH_OK;
}

// the scan of the bin counters into cg.cell_start: the whole grid, or a window's pieces with cell_start elsewhere filled with what
// a full scan leaves there
static int scan_cells(const GridBuild &bd, CellGrid &cg)
{
    const Grid &g = cg.g;
    const GridPlan &pl = bd.pl;
    hipStream_t st = bd.st;
    auto scan_piece = [&](int64_t from, int64_t to, unsigned use_gen, int *flags) {
        launch_scan_gen(st, bd.cell_count + from, cg.cell_start + from, to - from, bd.ctl, use_gen, true, flags); // [to] = the piece's total
    };
    if (!pl.windowed) {
        scan_piece(0, g.ncell, bd.gen, cg.flags);
        return MDH_OK;
    }
    // the pieces in index order: [p0, p1) then [p2, p3); a piece is scanned on its own, the atoms before it added by the
    // fill / by a second add pass; cell_start elsewhere = what a full scan leaves: the atoms binned so far.  The counters
    // outside the window are zero (kept block; atoms out there take no slot) and stay untouched.
    const int64_t plane = (int64_t)g.nc[1] * g.nc[2];
    const int64_t a0 = pl.p0 * plane, a1 = pl.p1 * plane, b0 = pl.p2 * plane, b1 = pl.p3 * plane;
    // (a constant fill through the runtime's fill kernel.  Looks unreachable: a window of two pieces starts at plane 0; kept as it stood)
    if (b1 > b0 && a0 > 0) MDH_HIP(hipMemsetD32Async(reinterpret_cast<hipDeviceptr_t>(cg.cell_start), 0, (size_t)a0, st));
    // (from a multiple of four cells on: the scan moves 16 bytes per access only from an aligned start — 66 against 26 us for the
    // 3.6 M cells of a 10 M-atom slab; the up to three counters in front of the window are zero, and zero is what the cells in
    // front of the window hold)
    scan_piece(a0 & ~(int64_t)3, a1, bd.gen, cg.flags);
    if (b1 <= b0) { // one piece: everything outside it in one launch
        const int64_t n1 = g.ncell + 1, quads = ((a0 + 3) >> 2) + ((n1 - std::min(n1, (a1 + 1 + 3) & ~(int64_t)3) + 3) >> 2) + 1;
        hipLaunchKernelGGL(k_fill_outside, dim3(grid_for(quads, 256)), dim3(256), 0, st, cg.cell_start, a0, a1, n1, cg.cell_start + a1);
    } else {
        // second piece: offsets start at the first piece's total, which sits on the device in cell_start[a1]
        fill_from(st, cg.cell_start, a1 + 1, b0, cg.cell_start + a1);
        scan_piece(b0, b1, next_scan_gen(), nullptr);
        hipLaunchKernelGGL(k_add_from, dim3(grid_for(b1 - b0 + 1, 256)), dim3(256), 0, st, cg.cell_start, b0, b1 + 1, cg.cell_start + a1, (int64_t)-1);
        // behind the window: the number of atoms BINNED (cell_start[b1], on the device) — N unless the promise was broken; with
        // the constant N a cell behind a broken window spanned the records [n_binned, N), which k_scatter / k_gather never wrote
        if (b1 < g.ncell)
            fill_from(st, cg.cell_start, b1 + 1, g.ncell + 1, cg.cell_start + b1);
    }
    return MDH_OK;
}

// every cell's atoms into descending id (or key) order
static void sort_cells(const GridBuild &bd, CellGrid &cg)
{
    const Grid &g = cg.g;
    const GridPlan &pl = bd.pl;
    int *rank = reinterpret_cast<int *>(bd.ent); // (free once the atoms are scattered)
    const int64_t plane = (int64_t)g.nc[1] * g.nc[2];
    auto piece = [&](int64_t from, int64_t to) {
        hipLaunchKernelGGL(k_sort_cells, dim3(grid_for((to - from) * plane, 256)), dim3(256), 0, bd.st, cg.cell_start + from * plane, cg.order, (to - from) * plane, bd.rq.sort_key, rank);
    };
    switch (pl.sort) {
    case GridPlan::SORT_NONE: break;
    case GridPlan::SORT_DENSE:
        hipLaunchKernelGGL(k_sort_cells_dense, dim3(grid_for(g.ncell, 32)), dim3(256), 0, bd.st, cg.cell_start, cg.order, g.ncell, rank);
        break;
    case GridPlan::SORT_CELLS:
        // (hist: this build could have been a slot build — it reports a cell of more than SLOT_CAP atoms as one would)
        hipLaunchKernelGGL(k_sort_cells, dim3(grid_for(g.ncell, 256)), dim3(256), 0, bd.st, cg.cell_start, cg.order, g.ncell, bd.rq.sort_key, rank, bd.ctl, bd.gen, bd.hist);
        if (bd.hist) { cg.big_stamp = bd.ctl + 3; cg.big_gen = bd.gen; cg.big_sink = bd.hist; }
        break;
    case GridPlan::SORT_PIECES:
        piece(pl.p0, pl.p1);
        if (pl.p3 > pl.p2) piece(pl.p2, pl.p3);
        break;
    }
}

// the atoms in the plan's form
static void gather_atoms(const GridBuild &bd, CellGrid &cg)
{
    const int64_t N = bd.N;
    // (the atoms binned = the grid's total, on the device: all N unless absent atoms were handed in or a window's promise was broken)
    const int *n_binned = cg.cell_start + cg.g.ncell;
    if (bd.pl.form == GridPlan::INDIRECT) { cg.ix = bd.x; cg.iy = bd.y; cg.iz = bd.z; cg.imv = bd.mv; } // nothing is gathered
    else if (bd.pl.form == GridPlan::RECORDS_MOVED) hipLaunchKernelGGL(k_gather_records, dim3(grid_for(N, 256)), dim3(256), 0, bd.st, bd.rec, cg.order, cg.pk, N, n_binned);
    else hipLaunchKernelGGL(k_gather, dim3(grid_for(N, 256)), dim3(256), 0, bd.st, bd.x, bd.y, bd.z, cg.order, cg.xs, cg.ys, cg.zs, N, bd.mv, cg.mvs, cg.pk, cg.flags + 4, n_binned);
}

int build_cell_grid(Scope &sc, const double *x, const double *y, const double *z, int64_t N, const DBox &b, const GridRequest &rq,
                    CellGrid &cg)
{
    PendingWindows hints; // (from here on values: only a build for neighbor rows uses them, plan_grid)
    MDH_TRY(take_pending_windows(hints));
    const Grid g = cg.g;
    cg = CellGrid{};
    cg.g = g;
    cg.n_binned = N;

    GridPlanIn in;
    int *order_word = nullptr;
    MDH_TRY(read_plan_inputs(rq, N, b, x, hints, cg, in, &order_word));
    GridBuild bd{sc.stream(), x, y, z, N, b, rq, plan_grid(in)};
    const GridPlan &pl = bd.pl;
    g_last_form.store(pl.form, std::memory_order_relaxed);
    if (pl.keeps_history) {
        bd.hist = cg.fb->host + GridFeedback::BIG;
        g_last_hist.store(cg.fb, std::memory_order_relaxed);
    }
    MDH_TRY(allocate_grid(sc, bd, cg));

    cg.win_lo = pl.win_lo; cg.win_hi = pl.win_hi;
    cg.cen_lo = pl.cen_lo; cg.cen_hi = pl.cen_hi;
    cg.flags_fresh = true;
    if (pl.windowed) {
        if (!g_window_violations) MDH_HIP(hipHostMalloc(reinterpret_cast<void **>(&g_window_violations), sizeof(int), hipHostMallocDefault));
        *g_window_violations = 0;
        bd.bad = g_window_violations;
    }
    if (pl.samples_order) sample_order(bd, order_word);
    bd.gen = next_scan_gen();
    bin_atoms(bd, cg);
    if (bd.slot())
        return finish_slot_grid(sc, bd, cg);
    MDH_TRY(scan_cells(bd, cg));
    sc.keep_confirm(bd.cell_count); // every counter a binned atom touched has been read and cleared by a scan enqueued above
    hipLaunchKernelGGL(k_scatter, dim3(grid_for((N + 1) / 2, 256)), dim3(256), 0, bd.st, bd.ent, cg.cell_start, cg.order, N);
    sort_cells(bd, cg);
    gather_atoms(bd, cg);
    MDH_HIP(hipGetLastError());
    return MDH_OK;
}

} // namespace mdh

using namespace mdh;

extern "C" {

int mdh_hint_centre_window(int axis, double frac_lo, double frac_hi)
{
    g_pending.centre = CellWindow{axis, frac_lo, frac_hi, true};
    return MDH_OK;
}

int mdh_hint_cell_window(int axis, double frac_lo, double frac_hi)
{
    g_pending.cells = CellWindow{axis, frac_lo, frac_hi, true};
    return MDH_OK;
}

int mdh_cell_window_check(void *stream)
{
    if (!g_window_violations)
        return MDH_OK;
    MDH_HIP(hipStreamSynchronize(reinterpret_cast<hipStream_t>(stream)));
    if (*(volatile int *)g_window_violations != 0) {
        *g_window_violations = 0;
        set_error("the last neighbor build on this thread found atoms outside the cell window it had been promised (mdh_hint_cell_window): its rows are incomplete");
        return MDH_ERR_ARG;
    }
    return MDH_OK;
}

int mdh_debug_set_indirect(int on) { return g_indirect.exchange(on ? 1 : 0); }
int mdh_debug_set_slot_grid(int on)
{
    if (on == 2) { // ... and every signature's history forgotten: its next build is a first one
        std::lock_guard<std::mutex> lk(g_slot_mu);
        for (GridFeedback *f : g_feedback) f->host[GridFeedback::BIG] = -1; // (the caller has synchronised: no build is in flight)
    }
    return g_slot_grid.exchange(on ? 1 : 0);
}
int mdh_debug_slot_grid_counters(int64_t *out4)
{
    const GridFeedback *f = g_last_hist.load(std::memory_order_relaxed);
    const volatile int *h = f ? f->host + GridFeedback::BIG : nullptr;
    const int last = h ? h[0] : 0, big = h ? h[1] : 0;
    out4[0] = last_grid_was_slot();
    out4[1] = last > 0 ? 1 : 0;
    out4[2] = out4[1] ? big : 0;
    out4[3] = SLOT_CAP;
    return MDH_OK;
}
int mdh_debug_slot_grid_rule(int ordered, int keyed, int windowed, int row_width, int64_t ncell, int64_t N, int seen, int big, int listed)
{
    return slot_grid_rule(ordered != 0, keyed != 0, windowed != 0, row_width, ncell, N, seen != 0, big != 0, listed) ? 1 : 0;
}
int mdh_debug_grid_plan(const int64_t *in24, const double *in6, int *out15)
{
    GridPlanIn in;
    in.atoms = (int)in24[0]; in.sort_desc = in24[1] != 0; in.keyed = in24[2] != 0; in.slots_ok = in24[3] != 0; in.row_width = (int)in24[4];
    in.N = in24[5]; in.ncell = in24[6]; in.nc[0] = (int)in24[7]; in.nc[1] = (int)in24[8]; in.nc[2] = (int)in24[9];
    in.mode = (int)in24[10]; in.tri = in24[11] != 0;
    in.cells = CellWindow{(int)in24[13], in6[2], in6[3], in24[12] != 0};
    in.centre = CellWindow{(int)in24[15], in6[4], in6[5], in24[14] != 0};
    in.order_word = (int)in24[16]; in.order_sample = in24[17] != 0; in.big = (int)in24[18]; in.listed = (int)in24[19]; in.record_width = (int)in24[20];
    in.indirect_on = in24[21] != 0; in.slot_on = in24[22] != 0; in.slot_force = in24[23] != 0;
    in.rc_inv = in6[0]; in.h0 = in6[1];
    const GridPlan pl = plan_grid(in);
    const int out[15] = {pl.form, pl.keeps_history, pl.samples_order, pl.assign4, pl.p0, pl.p1, pl.p2, pl.p3, pl.windowed, pl.win_lo, pl.win_hi,
                         pl.cen_lo, pl.cen_hi, pl.sort, pl.row_width};
    std::copy(out, out + 15, out15);
    return MDH_OK;
}
}

MDH_WARM_UNIT(cell_grid)

// the grouping rule of k_assign on the host (assign_groups.hpp), slice by slice
extern "C" int64_t mdh_debug_assign_groups(const int *cells, int64_t n, int *head, int *count, int *rank)
{
    int64_t atomics = 0;
    for (int64_t s0 = 0; s0 < n; s0 += 64) {
        int c[64], h[64], k[64], r[64];
        for (int l = 0; l < 64; ++l) c[l] = s0 + l < n ? cells[s0 + l] : -1 - l;
        mdh::assign_groups::slice(c, h, k, r);
        for (int l = 0; l < 64 && s0 + l < n; ++l) {
            head[s0 + l] = h[l]; count[s0 + l] = k[l]; rank[s0 + l] = r[l];
            atomics += k[l] > 0 && c[l] >= 0 ? 1 : 0;
        }
    }
    return atomics;
}
