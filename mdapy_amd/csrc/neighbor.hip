// neighbor.hip — cell-list cutoff neighbor search on gfx950: the thread-per-atom kernels, the pass over a built cell grid
// (cell_grid.hip) that chooses among them and the tile kernels (neighbor_lane.hip, neighbor_tiled.hip), the row utilities and
// the C entry points.  Replaces src/neighbor.cpp of the reference (build_verlet_list :102-187, build_neighbor :351-388, the
// exact-width variant :189-349, sort_verlet_by_distance :745-775, wrap_positions :675-702, average_by_neighbor :704-743).
//
// Data layout in HBM: x,y,z f64[N] (SoA, original atom order); verlet int32[N][M], dist f64[N][M], nn int32[N] —
// rows in ORIGINAL atom order; scratch: the cell grid (CellGrid in grid.hpp).
#include "common.hpp"
#include "grid.hpp"
#include "cna_core.hpp"
#include <algorithm>
#include <mutex>
#include <vector>

namespace mdh {

static int *g_moved_probe = nullptr; // pinned: flags[0] of the last tracked neighbor pass (mdh_debug_track_counters)
int g_neighbor_variant = 0; // 0 = automatic, 1 = force the thread-per-atom kernel, any other value = no tile kernel of neighbor_lane.hip: the round-1 LDS-tiled kernel where it applies (tests pass 2)

// ----------------------------------------------------------------------------
// 27-cell scan, one thread per centre atom (centres taken in cell order so the
// lanes of a wave share their candidate cells through L1/L2).
//   MODE 0: count only            (first pass of the exact-width variant)
//   MODE 1: reference semantics   (write valid slots only, caller pre-filled pads)
//   MODE 2: also write the pads   (-1, rc+1)
// ----------------------------------------------------------------------------
// one centre atom (position p of the cell-sorted arrays): the reference's 27-cell walk, neighbor.cpp:139-177
// The cell view has two forms (template SLOT).  Compact: position p of the cell order names an atom, a cell is the range
// [cell_start[c], cell_start[c + 1]) of it, and the three cells of a z-run are one range.  Slot grid (CellGrid::slot_cap): cell_start[c]
// is the cell's COUNT, its first SLOT_CAP ids sit in descending order in the cell's slots of `order` (two planes of four, slot_pos:
// order[4 c + k] and order[4 ncell + 4 c + k - 4]), the three cells of a run are walked one by one, centres are named by their id (p = id: the atoms are the caller's arrays), and a cell whose count ran past
// SLOT_CAP has the rest of its atoms on the spill list.
//
// the largest id below `prev` among the atoms of an overflowed cell — its slots and its entries of the spill list — or -1: a
// selection walk, one pass over the (short) list per candidate; the rare path, and the next build of the signature is a compact one
__device__ __forceinline__ int next_id_below(const SortedView &sv, const SlotSpill &sp, int64_t cell, int prev)
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
// the k-th atom of a cell of a slot grid, in any fixed order (centres: every atom of the cell once); -1: none
__device__ __forceinline__ int slot_cell_atom(const SortedView &sv, const SlotSpill &sp, int64_t cell, int k)
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

template <bool TRI, int MODE, bool SLOT = false>
__device__ __forceinline__ int neighbor_one(const SortedView &sv, const int *__restrict__ cell_start, const DBox &b,
                                            const Grid &g, double rc, int *__restrict__ verlet, double *__restrict__ dist,
                                            int *__restrict__ nn, int64_t M, int64_t p, double xi, double yi, double zi, int c0, int c1,
                                            int c2, const SlotSpill &sp = SlotSpill{})
{
    int cnt = 0;
    const int i = SLOT ? (int)p : sv.id_of(p);
    const double rcsq = rc * rc; // neighbor.cpp:127
    const int64_t row = (int64_t)i * M;
    if constexpr (SLOT) {
        auto candidate = [&](int j, double xq, double yq, double zq) {
            if (j == i)
                return;
            double dx = xq - xi, dy = yq - yi, dz = zq - zi; // raw x[j] - wrapped centre, :164-166
            pbc<TRI>(b, dx, dy, dz);
            const double d2 = dx * dx + dy * dy + dz * dz;
            if (d2 <= rcsq) {
                if (MODE != 0 && cnt < M) {
                    verlet[row + cnt] = j;
                    dist[row + cnt] = sqrt(d2);
                }
                ++cnt;
            }
        };
        for (int a = c0 - 1; a <= c0 + 1; ++a) { // neighbor.cpp:147-151
            const int ca = pmod(a, g.nc[0]);
            for (int bb = c1 - 1; bb <= c1 + 1; ++bb) {
                const int64_t base = ((int64_t)ca * g.nc[1] + pmod(bb, g.nc[1])) * g.nc[2];
                for (int seg = 0; seg < 3; ++seg) {
                    const int64_t cell = base + pmod(c2 - 1 + seg, g.nc[2]);
                    const int n = cell_start[cell];
                    if (n > SLOT_CAP) { // descending id over the slots and the spill list
                        for (int j = next_id_below(sv, sp, cell, 0x7fffffff); j >= 0; j = next_id_below(sv, sp, cell, j))
                            candidate(j, sv.xs[j], sv.ys[j], sv.zs[j]);
                        continue;
                    }
                    for (int k0 = 0; k0 < n; k0 += 4) { // (four candidates per trip, as below: one plane of the cell's slots)
                        double xq[4], yq[4], zq[4];
                        int jq[4];
#pragma unroll
                        for (int u = 0; u < 4; ++u)
                            sv.get(slot_pos(cell, min(k0 + u, n - 1), sp.hi), xq[u], yq[u], zq[u], jq[u]);
#pragma unroll
                        for (int u = 0; u < 4; ++u)
                            if (k0 + u < n) candidate(jq[u], xq[u], yq[u], zq[u]);
                    }
                }
            }
        }
        nn[i] = cnt;
        if (MODE == 2) {
            const double pad = rc + 1.0;
            for (int64_t n = cnt; n < M; ++n) {
                verlet[row + n] = -1;
                dist[row + n] = pad;
            }
        }
        return cnt;
    }
    const bool zrun = (c2 >= 1) && (c2 + 1 < g.nc[2]); // the three z-cells are one contiguous run
    for (int a = c0 - 1; a <= c0 + 1; ++a) {            // neighbor.cpp:147-151
        const int ca = pmod(a, g.nc[0]);
        for (int bb = c1 - 1; bb <= c1 + 1; ++bb) {
            const int64_t base = ((int64_t)ca * g.nc[1] + pmod(bb, g.nc[1])) * g.nc[2];
            for (int seg = 0; seg < (zrun ? 1 : 3); ++seg) {
                int s, e;
                if (zrun) {
                    s = cell_start[base + c2 - 1];
                    e = cell_start[base + c2 + 2];
                } else {
                    const int cc = pmod(c2 - 1 + seg, g.nc[2]);
                    s = cell_start[base + cc];
                    e = cell_start[base + cc + 1];
                }
                // four candidates per trip, their loads issued together: with one candidate per trip every one of them is a
                // dependent L2 round trip (the loop carries the row count through a store), and a thread of the mop-up kernel in
                // a fat cell at the box's far faces walks a thousand of them — 0.54 ms for the 3 % of a 3.4 M-atom box at rc = 5 A
                for (int q0 = s; q0 < e; q0 += 4) {
                    double xq[4], yq[4], zq[4];
                    int jq[4];
#pragma unroll
                    for (int u = 0; u < 4; ++u) // (past the end of the piece: its last candidate again, not looked at)
                        sv.get(min(q0 + u, e - 1), xq[u], yq[u], zq[u], jq[u]);
#pragma unroll
                    for (int u = 0; u < 4; ++u) {
                        if (q0 + u >= e || jq[u] == i)
                            continue;
                        double dx = xq[u] - xi, dy = yq[u] - yi, dz = zq[u] - zi; // raw x[j] - wrapped centre, :164-166
                        pbc<TRI>(b, dx, dy, dz);
                        const double d2 = dx * dx + dy * dy + dz * dz;
                        if (d2 <= rcsq) {
                            if (MODE != 0 && cnt < M) {
                                verlet[row + cnt] = jq[u];
                                dist[row + cnt] = sqrt(d2);
                            }
                            ++cnt;
                        }
                    }
                }
            }
        }
    }
    nn[i] = cnt;
    if (MODE == 2) {
        const double pad = rc + 1.0;
        for (int64_t n = cnt; n < M; ++n) {
            verlet[row + n] = -1;
            dist[row + n] = pad;
        }
    }
    return cnt;
}

// The same walk by a whole wavefront for ONE atom: 64 candidates per trip, the hits' slots from a ballot (candidate order = row
// order, as above).  For the listed tiles of the mop-up kernel: their atoms sit in the fat last cells of the box, a thread walks
// 300 ... 1000 candidates there four at a time (80 ... 380 dependent trips), a wave 9 runs of one to three trips.
template <bool TRI, int MODE, bool SLOT = false>
__device__ __forceinline__ int neighbor_one_wave(const SortedView &sv, const int *__restrict__ cell_start, const DBox &b,
                                                 const Grid &g, double rc, int *__restrict__ verlet, double *__restrict__ dist,
                                                 int *__restrict__ nn, int64_t M, int64_t p, double xi, double yi, double zi, int c0,
                                                 int c1, int c2, const SlotSpill &sp = SlotSpill{})
{
    const int lane = (int)(threadIdx.x & 63);
    int cnt = 0;
    const int i = SLOT ? (int)p : sv.id_of(p);
    const double rcsq = rc * rc; // neighbor.cpp:127
    const int64_t row = (int64_t)i * M;
    if constexpr (SLOT) { // (the cell view's slot form, neighbor_one: a cell is one trip of the wave)
        for (int a = c0 - 1; a <= c0 + 1; ++a) { // neighbor.cpp:147-151
            const int ca = pmod(a, g.nc[0]);
            for (int bb = c1 - 1; bb <= c1 + 1; ++bb) {
                const int64_t base = ((int64_t)ca * g.nc[1] + pmod(bb, g.nc[1])) * g.nc[2];
                for (int seg = 0; seg < 3; ++seg) {
                    const int64_t cell = base + pmod(c2 - 1 + seg, g.nc[2]);
                    const int n = cell_start[cell];
                    if (n > SLOT_CAP) {
                        // an overflowed cell: every lane walks the same candidates in descending id (next_id_below), lane 0 writes
                        for (int j = next_id_below(sv, sp, cell, 0x7fffffff); j >= 0; j = next_id_below(sv, sp, cell, j)) {
                            double dx = sv.xs[j] - xi, dy = sv.ys[j] - yi, dz = sv.zs[j] - zi;
                            pbc<TRI>(b, dx, dy, dz);
                            const double d2 = dx * dx + dy * dy + dz * dz;
                            if (j != i && d2 <= rcsq) {
                                if (MODE != 0 && lane == 0 && cnt < M) {
                                    verlet[row + cnt] = j;
                                    dist[row + cnt] = sqrt(d2);
                                }
                                ++cnt;
                            }
                        }
                        continue;
                    }
                    bool hit = false;
                    int j = -1;
                    double d2 = 0.0;
                    if (lane < n) {
                        double xq, yq, zq;
                        sv.get(slot_pos(cell, lane, sp.hi), xq, yq, zq, j);
                        double dx = xq - xi, dy = yq - yi, dz = zq - zi; // raw x[j] - wrapped centre, :164-166
                        pbc<TRI>(b, dx, dy, dz);
                        d2 = dx * dx + dy * dy + dz * dz;
                        hit = j != i && d2 <= rcsq;
                    }
                    const unsigned long long m = __ballot(hit);
                    if (MODE != 0 && hit) {
                        const int slot = cnt + __popcll(m & ((1ull << lane) - 1ull));
                        if (slot < M) {
                            verlet[row + slot] = j;
                            dist[row + slot] = sqrt(d2);
                        }
                    }
                    cnt += __popcll(m);
                }
            }
        }
        if (lane == 0) nn[i] = cnt;
        if (MODE == 2) {
            const double pad = rc + 1.0;
            for (int64_t n = cnt + lane; n < M; n += 64) {
                verlet[row + n] = -1;
                dist[row + n] = pad;
            }
        }
        return cnt;
    }
    const bool zrun = (c2 >= 1) && (c2 + 1 < g.nc[2]);
    for (int a = c0 - 1; a <= c0 + 1; ++a) { // neighbor.cpp:147-151
        const int ca = pmod(a, g.nc[0]);
        for (int bb = c1 - 1; bb <= c1 + 1; ++bb) {
            const int64_t base = ((int64_t)ca * g.nc[1] + pmod(bb, g.nc[1])) * g.nc[2];
            for (int seg = 0; seg < (zrun ? 1 : 3); ++seg) {
                int s, e;
                if (zrun) {
                    s = cell_start[base + c2 - 1];
                    e = cell_start[base + c2 + 2];
                } else {
                    const int cc = pmod(c2 - 1 + seg, g.nc[2]);
                    s = cell_start[base + cc];
                    e = cell_start[base + cc + 1];
                }
                for (int q0 = s; q0 < e; q0 += 64) {
                    const int q = q0 + lane;
                    bool hit = false;
                    int j = -1;
                    double d2 = 0.0;
                    if (q < e) {
                        double xq, yq, zq;
                        sv.get(q, xq, yq, zq, j);
                        double dx = xq - xi, dy = yq - yi, dz = zq - zi; // raw x[j] - wrapped centre, :164-166
                        pbc<TRI>(b, dx, dy, dz);
                        d2 = dx * dx + dy * dy + dz * dz;
                        hit = j != i && d2 <= rcsq;
                    }
                    const unsigned long long m = __ballot(hit);
                    if (MODE != 0 && hit) {
                        const int slot = cnt + __popcll(m & ((1ull << lane) - 1ull));
                        if (slot < M) {
                            verlet[row + slot] = j;
                            dist[row + slot] = sqrt(d2);
                        }
                    }
                    cnt += __popcll(m);
                }
            }
        }
    }
    if (lane == 0) nn[i] = cnt;
    if (MODE == 2) {
        const double pad = rc + 1.0;
        for (int64_t n = cnt + lane; n < M; n += 64) {
            verlet[row + n] = -1;
            dist[row + n] = pad;
        }
    }
    return cnt;
}

template <bool TRI, int MODE, bool SLOT = false>
__device__ __forceinline__ void neighbor_atoms_body(const SortedView &sv,
                                                  const int *__restrict__ cell_start, int64_t N, const DBox &b, const Grid &g,
                                                  double rc, int *__restrict__ verlet, double *__restrict__ dist,
                                                  int *__restrict__ nn, int64_t M, int *__restrict__ max_count,
                                                  const TileFilter &tf, const SlotSpill &sp = SlotSpill{})
{
    const bool take_all = tf.moved && *tf.moved != 0; // the tiled kernel stood down: this kernel does the whole call
    if (tf.flag && !take_all && (tf.list || *tf.any == 0)) // nothing to mop up here (flagged tiles go to k_neighbor_tiles when listed)
        return;
    int cnt = 0;
    // the grid is capped (a stand-by launch then costs a few thousand workgroups that leave at once, not N / 256 of them):
    // a workgroup strides over the atoms
    // (cell_start[ncell] = the atoms the grid holds: N, or fewer after a windowed build that dropped atoms outside its window —
    // the records behind them were never written)
    // (a slot grid: the centres are taken by id from the caller's arrays — its atoms are in a spatial order already; an absent atom,
    // x = NaN, has no cell and gets no row)
    if (!SLOT) N = min(N, (int64_t)cell_start[g.ncell]);
    for (int64_t base = (int64_t)blockIdx.x * blockDim.x; base < N; base += (int64_t)gridDim.x * blockDim.x) {
        const int64_t p = base + threadIdx.x;
        bool mine = p < N;
        int c0 = 0, c1 = 0, c2 = 0;
        double xi = 0, yi = 0, zi = 0;
        if (SLOT && mine) {
            xi = sv.xs[p]; yi = sv.ys[p]; zi = sv.zs[p];
            mine = xi == xi;
        }
        if (mine) {
            if (!SLOT) { int idp; sv.get(p, xi, yi, zi, idp); }
            if (b.anypbc) // neighbor.cpp:139-142
                wrap<TRI>(b, xi, yi, zi);
            cell_coords<TRI>(b, g, xi, yi, zi, c0, c1, c2);
            if (tf.flag) { // fallback pass: only atoms of tiles the LDS-tiled kernel could not hold (or all of them when it stood down)
                const int t = ((c0 / tf.tile) * tf.nt[1] + (c1 / tf.tile)) * tf.nt[2] + (c2 / tf.tile_z);
                mine = take_all || tf.flag[t] != 0;
            }
        }
        if (mine) {
            cnt = max(cnt, neighbor_one<TRI, MODE, SLOT>(sv, cell_start, b, g, rc, verlet, dist, nn, M, p, xi, yi, zi, c0, c1, c2, sp));
            if (tf.cna_todo) defer(tf.cna_todo, SLOT ? (int)p : sv.id_of(p));
        }
    }
    if (MODE == 0) {
        int m = cnt;
#pragma unroll
        for (int d = 32; d >= 1; d >>= 1) {
            int t = __shfl_xor(m, d, 64);
            m = t > m ? t : m;
        }
        if ((threadIdx.x & 63) == 0 && m > __hip_atomic_load(max_count, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT))
            atomicMax(max_count, m); // (read first: a single word serialises ~90 atomics per microsecond)
    }
}

// mop-up of the tiles the wave kernel listed (halo over the LDS budget, atoms far outside the box): a workgroup per listed
// tile, its threads over the tile's centre atoms — the cost follows the number of listed tiles, not N
template <bool TRI, int MODE, bool SLOT = false>
__global__ __launch_bounds__(256) void k_neighbor(SortedView sv, const int *__restrict__ cell_start, int64_t N, DBox b, Grid g, double rc,
                                                  int *__restrict__ verlet, double *__restrict__ dist, int *__restrict__ nn, int64_t M,
                                                  int *__restrict__ max_count, TileFilter tf, SlotSpill sp)
{
    if (tf.big_sink && blockIdx.x == 0 && threadIdx.x == 0)
        *tf.big_sink = *tf.big_stamp == tf.big_gen ? 1 : 0; // (pinned host memory: the history of the slot grid, CellGrid::big_sink)
    neighbor_atoms_body<TRI, MODE, SLOT>(sv, cell_start, N, b, g, rc, verlet, dist, nn, M, max_count, tf, sp);
}

template <bool TRI, int MODE, bool SLOT = false>
__device__ __forceinline__ void neighbor_tiles_body(const SortedView &sv,
                                                        const int *__restrict__ cell_start, const DBox &b, const Grid &g, double rc,
                                                        int *__restrict__ verlet, double *__restrict__ dist, int *__restrict__ nn,
                                                        int64_t M, int *__restrict__ max_count, const TileFilter &tf,
                                                        const SlotSpill &sp = SlotSpill{})
{
    if (tf.moved && *tf.moved != 0) // k_neighbor takes the whole call
        return;
    const int nlist = min(*tf.any, tf.list_cap);
    int best = 0;
    // a workgroup per (listed tile, column of the tile), a wavefront per atom of the column's z-run (neighbor_one_wave)
    const int ncol = tf.tile * tf.tile;
    const int wave = (int)(threadIdx.x >> 6), nwave = (int)(blockDim.x >> 6);
    // (... and a column's atoms in MOP_CHUNKS interleaved shares, a workgroup each: the corner column of the box holds 84 atoms in
    // one cell where the mean is 12 — 21 atoms per wave was the whole kernel's critical path, 440 us)
    constexpr int MOP_CHUNKS = 8;
    for (int64_t w8 = blockIdx.x; w8 < (int64_t)nlist * ncol * MOP_CHUNKS; w8 += gridDim.x) {
        const int64_t w = w8 / MOP_CHUNKS;
        const int chunk = (int)(w8 - w * MOP_CHUNKS);
        const int t = tf.list[w / ncol], colq = (int)(w % ncol);
        const int t2 = t % tf.nt[2], t1 = (t / tf.nt[2]) % tf.nt[1], t0 = t / (tf.nt[2] * tf.nt[1]);
        const int z0 = t2 * tf.tile_z, z1 = min(z0 + tf.tile_z, g.nc[2]);
        const int a = t0 * tf.tile + colq / tf.tile, c = t1 * tf.tile + colq % tf.tile;
        if (a < g.nc[0] && c < g.nc[1]) {
            const int64_t col = ((int64_t)a * g.nc[1] + c) * g.nc[2];
            if constexpr (SLOT) {
                // the column's atoms cell by cell, numbered as they come (slot_cell_atom); this wave takes every
                // (nwave * MOP_CHUNKS)-th of them, as below
                int seen = 0;
                for (int cz = z0; cz < z1; ++cz) {
                    const int n = cell_start[col + cz];
                    for (int k = 0; k < n; ++k, ++seen) {
                        if (seen % (nwave * MOP_CHUNKS) != chunk * nwave + wave)
                            continue;
                        const int id = slot_cell_atom(sv, sp, col + cz, k);
                        if (id < 0)
                            continue;
                        double xi = sv.xs[id], yi = sv.ys[id], zi = sv.zs[id];
                        if (b.anypbc)
                            wrap<TRI>(b, xi, yi, zi);
                        int c0, c1, c2;
                        cell_coords<TRI>(b, g, xi, yi, zi, c0, c1, c2);
                        best = max(best, neighbor_one_wave<TRI, MODE, true>(sv, cell_start, b, g, rc, verlet, dist, nn, M, id, xi, yi, zi, c0, c1, c2, sp));
                        if (tf.cna_todo && (threadIdx.x & 63) == 0) defer(tf.cna_todo, id);
                    }
                }
                continue;
            }
            const int s = cell_start[col + z0], e = cell_start[col + z1]; // the z-run of a column is contiguous
            for (int p = s + chunk * nwave + wave; p < e; p += nwave * MOP_CHUNKS) {
                double xi, yi, zi;
                { int idp; sv.get(p, xi, yi, zi, idp); }
                if (b.anypbc)
                    wrap<TRI>(b, xi, yi, zi);
                int c0, c1, c2;
                cell_coords<TRI>(b, g, xi, yi, zi, c0, c1, c2);
                best = max(best, neighbor_one_wave<TRI, MODE>(sv, cell_start, b, g, rc, verlet, dist, nn, M, p, xi, yi, zi, c0, c1, c2));
                if (tf.cna_todo && (threadIdx.x & 63) == 0) defer(tf.cna_todo, sv.id_of(p));
            }
        }
    }
    if (MODE == 0) {
#pragma unroll
        for (int d = 32; d >= 1; d >>= 1) best = max(best, __shfl_xor(best, d, 64));
        if ((threadIdx.x & 63) == 0 && best > __hip_atomic_load(max_count, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT))
            atomicMax(max_count, best);
    }
}

template <bool TRI, int MODE, bool SLOT = false>
__global__ __launch_bounds__(256) void k_neighbor_tiles(SortedView sv, const int *__restrict__ cell_start, DBox b, Grid g, double rc,
                                                        int *__restrict__ verlet, double *__restrict__ dist, int *__restrict__ nn, int64_t M,
                                                        int *__restrict__ max_count, TileFilter tf, SlotSpill sp)
{
    neighbor_tiles_body<TRI, MODE, SLOT>(sv, cell_start, b, g, rc, verlet, dist, nn, M, max_count, tf, sp);
}

// the two stand-bys behind a tile kernel that lists its leftovers, as ONE launch (a launch that finds nothing to do costs
// ~4 us): the whole call atom by atom if the tile kernel stood down (unwrapped input), else the listed tiles
template <bool TRI, int MODE, bool SLOT = false>
__global__ __launch_bounds__(256) void k_neighbor_mop(SortedView sv, const int *__restrict__ cell_start, int64_t N, DBox b, Grid g, double rc,
                                                      int *__restrict__ verlet, double *__restrict__ dist, int *__restrict__ nn, int64_t M,
                                                      int *__restrict__ max_count, TileFilter tf, SlotSpill sp)
{
    if (tf.listed_sink && blockIdx.x == 0 && threadIdx.x == 0)
        *tf.listed_sink = min(*tf.any, tf.list_cap); // (pinned host memory: the next build of this (N, grid) launches the slice pass if anything was listed)
    if (tf.big_sink && blockIdx.x == 0 && threadIdx.x == 0)
        *tf.big_sink = *tf.big_stamp == tf.big_gen ? 1 : 0; // (pinned host memory: the history of the slot grid, CellGrid::big_sink)
    if (tf.moved && *tf.moved != 0) neighbor_atoms_body<TRI, MODE, SLOT>(sv, cell_start, N, b, g, rc, verlet, dist, nn, M, max_count, tf, sp);
    else neighbor_tiles_body<TRI, MODE, SLOT>(sv, cell_start, b, g, rc, verlet, dist, nn, M, max_count, tf, sp);
}

template <int MODE>
static void launch_neighbor(hipStream_t st, const CellGrid &cg, int64_t N, const DBox &b, double rc, int *verlet,
                            double *dist, int *nn, int64_t M, int *max_count, TileFilter tf = TileFilter{})
{
    // behind a tile kernel that lists its leftovers this launch only stands by for unwrapped input (device flag): a small grid
    // then, whose workgroups stride over the atoms if they do have to take the call (10 -> 3 us when they leave at once)
    dim3 grid(std::min(grid_for(N, 256), tf.list ? 2048 : 8192)), block(256);
    const SlotSpill sp{cg.spill, cg.n_spill, cg.slot_hi};
    // (TRI, SLOT: the cell view's form, CellGrid::slot_cap)
#define MDH_MOP(KERNEL, TRI, SLOT, ...) hipLaunchKernelGGL((KERNEL<TRI, MODE, SLOT>), grid, block, 0, st, view_of(cg), cg.cell_start, __VA_ARGS__, b, cg.g, rc, verlet, dist, nn, M, max_count, tf, sp)
    if (tf.list) { // behind a tile kernel with a list (at most list_cap entries): both stand-bys in one launch
        if (cg.slot_cap) { if (b.tri) MDH_MOP(k_neighbor_mop, true, true, N); else MDH_MOP(k_neighbor_mop, false, true, N); }
        else { if (b.tri) MDH_MOP(k_neighbor_mop, true, false, N); else MDH_MOP(k_neighbor_mop, false, false, N); }
        return;
    }
    if (cg.slot_cap) { if (b.tri) MDH_MOP(k_neighbor, true, true, N); else MDH_MOP(k_neighbor, false, true, N); }
    else { if (b.tri) MDH_MOP(k_neighbor, true, false, N); else MDH_MOP(k_neighbor, false, false, N); }
#undef MDH_MOP
}

// ----------------------------------------------------------------------------
// small row-wise helpers
// ----------------------------------------------------------------------------
// neighbor.cpp:745-775: selection of the first k entries by strict '<' over all M columns.
// One wave per workgroup, 64/L consecutive rows of it, L lanes to a row (L = 1 ... 16, the smallest that keeps the LDS copy
// of the rows near 10 KB: 12+ waves per CU, where 64 rows of 50 entries — build_neighbor(5.0, 50), the published workflow —
// left one wave per SIMD and the list read at 0.8 TB/s).  The rows are one contiguous piece of memory: read with 16-byte
// loads into LDS (element c of row r at [c * ROWS + r]; lane j * ROWS + r walks columns a+1+j, a+1+j+L, ...: consecutive
// words, conflict-free), selected there — every lane starts from entry a and only takes a strictly smaller one, the L
// partial results meet by (distance, column): the first of the smallest, as the serial loop has it — and only written back
// when something moved: the rows of a k-nearest search arrive sorted, and every analysis that borrows them "sorts" them
// again (the reference does the same); for those the kernel is one read of the list.
template <int L>
__global__ __launch_bounds__(64) void k_sort_rows(int *__restrict__ verlet, double *__restrict__ dist, int64_t N, int M, int k,
                                                  unsigned inv_m)
{
    constexpr int ROWS = 64 / L;
    extern __shared__ __attribute__((aligned(16))) unsigned char sort_lds[];
    double *ld = reinterpret_cast<double *>(sort_lds);        // [M][ROWS]
    int *lv = reinterpret_cast<int *>(ld + (size_t)M * ROWS); // [M][ROWS]
    const int64_t row0 = (int64_t)blockIdx.x * ROWS;
    const int rows = (int)((N - row0) < ROWS ? (N - row0) : ROWS);
    const int total = rows * M;
    const int t = threadIdx.x;
    double *__restrict__ gd = dist + row0 * M;
    int *__restrict__ gv = verlet + row0 * M;
    // e -> (row, column): e < 2^16 and M < 2^16, so the high word of e * ceil(2^32 / M) is e / M exactly
    auto slot = [&](int e) {
        const int r = (int)__umulhi((unsigned)e, inv_m);
        return (e - r * M) * ROWS + r;
    };
    const bool vec = rows == ROWS && ((reinterpret_cast<uintptr_t>(dist) | reinterpret_cast<uintptr_t>(verlet)) & 15) == 0; // (ROWS * M is a multiple of 4)
    if (vec) {
        {
            const double2 *gd2 = reinterpret_cast<const double2 *>(gd);
            const int4 *gv4 = reinterpret_cast<const int4 *>(gv);
#pragma unroll 4
            for (int p = t; p < (total >> 1); p += 64) {
                const double2 v = gd2[p];
                ld[slot(2 * p)] = v.x; ld[slot(2 * p + 1)] = v.y;
            }
#pragma unroll 4
            for (int p = t; p < (total >> 2); p += 64) {
                const int4 v = gv4[p];
                lv[slot(4 * p)] = v.x; lv[slot(4 * p + 1)] = v.y; lv[slot(4 * p + 2)] = v.z; lv[slot(4 * p + 3)] = v.w;
            }
        }
    } else {
        for (int e = t; e < total; e += 64) { const int s = slot(e); ld[s] = gd[e]; lv[s] = gv[e]; }
    }
    __syncthreads();
    const int r = t & (ROWS - 1), j = t / ROWS;
    const bool live = r < rows;
    const double *lr = ld + r;
    // One walk first: entries 0 ... p-1 stay where they are if they ascend and nothing behind them is smaller — rows that
    // arrive sorted (a k-nearest list; the same list sorted for the analysis before this one) are done after this walk,
    // rows sorted to 12 and now wanted to 14 start at 12.  (s: the smallest entry behind a; '<' only, as the selection.)
    int first = k;
    if (live) {
        double s = __builtin_inf();
        for (int c = k + j; c < M; c += L) {
            const double v = lr[c * ROWS];
            if (v < s) s = v;
        }
#pragma unroll
        for (int w = ROWS; w < 64; w <<= 1) {
            const double o = __shfl_xor(s, w);
            if (o < s) s = o;
        }
        for (int a = k - 1; a >= 0; --a) {
            const double v = lr[a * ROWS];
            if (s < v) first = a;
            if (v < s) s = v;
        }
    }
#pragma unroll
    for (int w = 1; w < 64; w <<= 1) {
        const int o = __shfl_xor(first, w);
        first = o < first ? o : first;
    }
    bool moved = false;
    for (int a = first; a < k; ++a) {
        int best = a;
        double db = live ? lr[a * ROWS] : 0.0;
        if (live) {
            int c = a + 1 + j;
            for (; c + 3 * L < M; c += 4 * L) {
                const double v0 = lr[c * ROWS], v1 = lr[(c + L) * ROWS], v2 = lr[(c + 2 * L) * ROWS], v3 = lr[(c + 3 * L) * ROWS];
                if (v0 < db) { db = v0; best = c; }
                if (v1 < db) { db = v1; best = c + L; }
                if (v2 < db) { db = v2; best = c + 2 * L; }
                if (v3 < db) { db = v3; best = c + 3 * L; }
            }
            for (; c < M; c += L) {
                const double v = lr[c * ROWS];
                if (v < db) { db = v; best = c; }
            }
        }
#pragma unroll
        for (int w = ROWS; w < 64; w <<= 1) { // the other lanes of this row are w, 2w, ... lanes away
            const double od = __shfl_xor(db, w);
            const int ob = __shfl_xor(best, w);
            if (od < db || (od == db && ob < best)) { db = od; best = ob; }
        }
        if (live && j == 0 && best != a) {
            const double td = ld[a * ROWS + r];
            ld[a * ROWS + r] = db; ld[best * ROWS + r] = td;
            const int tv = lv[a * ROWS + r];
            lv[a * ROWS + r] = lv[best * ROWS + r]; lv[best * ROWS + r] = tv;
            moved = true;
        }
        if (L > 1) __syncthreads(); // (one wave: the writes above are in LDS before the next column walk of the row's other lanes)
    }
    if (!__syncthreads_or(moved ? 1 : 0))
        return;
    if (vec) {
        double2 *gd2 = reinterpret_cast<double2 *>(gd);
        int4 *gv4 = reinterpret_cast<int4 *>(gv);
#pragma unroll 4
        for (int p = t; p < (total >> 1); p += 64)
            gd2[p] = make_double2(ld[slot(2 * p)], ld[slot(2 * p + 1)]);
#pragma unroll 4
        for (int p = t; p < (total >> 2); p += 64)
            gv4[p] = make_int4(lv[slot(4 * p)], lv[slot(4 * p + 1)], lv[slot(4 * p + 2)], lv[slot(4 * p + 3)]);
    } else {
        for (int e = t; e < total; e += 64) { const int s = slot(e); gd[e] = ld[s]; gv[e] = lv[s]; }
    }
}

// the same in place in HBM, for rows too wide for the LDS copy
__global__ __launch_bounds__(256) void k_sort_rows_wide(int *__restrict__ verlet, double *__restrict__ dist, int64_t N,
                                                        int64_t M, int k)
{
    int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= N)
        return;
    int *v = verlet + i * M;
    double *d = dist + i * M;
    for (int a = 0; a < k; ++a) {
        int best = a;
        double db = d[a];
        for (int c = a + 1; c < M; ++c) {
            double t = d[c];
            if (t < db) { db = t; best = c; }
        }
        if (best != a) {
            double td = d[a]; d[a] = db; d[best] = td;
            int tv = v[a]; v[a] = v[best]; v[best] = tv;
        }
    }
}

// whole rows of up to SORT_BLOCK_MAX entries, one workgroup per row: a bitonic network over (distance, index) keys in LDS
// (the selection sort above is quadratic in the row length: a 36 000-wide row — surface atoms of a slab looking across
// its vacuum — took minutes)
constexpr int SORT_BLOCK_MAX = 8192;
constexpr int SORT_LDS_WIDEST = 1024; // the selection kernel above with 16 lanes to a row: 4 rows of 1024 entries in 48 KB
__global__ __launch_bounds__(256) void k_sort_rows_block(int *__restrict__ verlet, double *__restrict__ dist, int64_t M, int P)
{
    extern __shared__ double sort_block_lds[];
    double *ld = sort_block_lds;
    int *lv = (int *)(sort_block_lds + P);
    const int64_t row = blockIdx.x;
    const int t = threadIdx.x;
    for (int c = t; c < P; c += 256) {
        ld[c] = c < M ? dist[row * M + c] : 1.0e300;
        lv[c] = c < M ? verlet[row * M + c] : 0x7fffffff;
    }
    __syncthreads();
    for (int size = 2; size <= P; size <<= 1)
        for (int stride = size >> 1; stride > 0; stride >>= 1) {
            for (int e = t; e < (P >> 1); e += 256) {
                const int lo = ((e & ~(stride - 1)) << 1) | (e & (stride - 1)), hi = lo | stride;
                const bool up = (lo & size) == 0;
                const double a = ld[lo], c = ld[hi];
                const int va = lv[lo], vc = lv[hi];
                const bool gt = a > c || (a == c && va > vc);
                if (gt == up) { ld[lo] = c; ld[hi] = a; lv[lo] = vc; lv[hi] = va; }
            }
            __syncthreads();
        }
    for (int c = t; c < M; c += 256) {
        dist[row * M + c] = ld[c];
        verlet[row * M + c] = lv[c];
    }
}

template <bool TRI>
__global__ __launch_bounds__(256) void k_wrap(double *__restrict__ x, double *__restrict__ y, double *__restrict__ z,
                                              int64_t N, DBox b)
{
    int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= N)
        return;
    double xi = x[i], yi = y[i], zi = z[i];
    wrap<TRI>(b, xi, yi, zi); // neighbor.cpp:695 (unconditional)
    x[i] = xi; y[i] = yi; z[i] = zi;
}

// (the rows of the workgroup a chunk at a time through LDS: common.hpp stage_row_chunk)
__global__ __launch_bounds__(64) void k_average(double rc, const int *__restrict__ verlet,
                                                const double *__restrict__ dist, const int *__restrict__ nn,
                                                int64_t N, int64_t M, const double *__restrict__ value,
                                                double *__restrict__ out, int include_self)
{
    __shared__ int ids[ROW_CHUNK * 64];
    __shared__ double dst[ROW_CHUNK * 64];
    const int64_t row0 = (int64_t)blockIdx.x * 64, i = row0 + threadIdx.x;
    const bool on = i < N;
    double s = 0.0;
    int cnt = 0;
    if (on && include_self) { s += value[i]; ++cnt; }
    const int n = on ? min(nn[i], (int)M) : 0;
    const int most = wave_max(n);
    for (int c0 = 0; c0 < most; c0 += ROW_CHUNK) {
        __syncthreads();
        stage_row_chunk<true>(verlet, dist, N, M, row0, c0, ids, dst);
        __syncthreads();
        // neighbor.cpp:729-736 (sequential sum in list order); the values of a chunk's entries requested together
        double val[ROW_CHUNK];
#pragma unroll
        for (int q = 0; q < ROW_CHUNK; ++q)
            val[q] = (c0 + q < n && dst[q * 64 + threadIdx.x] <= rc) ? value[safe_id(ids[q * 64 + threadIdx.x], i, N)] : 0.0;
#pragma unroll
        for (int q = 0; q < ROW_CHUNK; ++q)
            if (c0 + q < n && dst[q * 64 + threadIdx.x] <= rc) { s += val[q]; ++cnt; }
    }
    if (on) out[i] = cnt > 0 ? s / cnt : 0.0;
}

// filter_overlap_atom (neighbor.cpp:390-486): keep[j] = 0 iff some atom i < j lies within rc of j.  The reference lets
// every centre i mark its higher-numbered neighbours; here every atom j looks for a lower-numbered i and evaluates the
// very expression centre i would: raw x[j] - wrapped x[i], folded, squared, compared with rc^2.  The 27-cell
// neighbourhood is symmetric, so the same pairs are examined.
template <bool TRI>
__global__ __launch_bounds__(256) void k_filter_overlap(const double *__restrict__ xs, const double *__restrict__ ys,
                                                        const double *__restrict__ zs, const int *__restrict__ order,
                                                        const int *__restrict__ cell_start, int64_t N, DBox b, Grid g,
                                                        double rc, unsigned char *__restrict__ keep)
{
    const int64_t p = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (p >= N)
        return;
    const double xr = xs[p], yr = ys[p], zr = zs[p]; // raw position of j
    double xw = xr, yw = yr, zw = zr;
    if (b.anypbc)
        wrap<TRI>(b, xw, yw, zw);
    int c0, c1, c2;
    cell_coords<TRI>(b, g, xw, yw, zw, c0, c1, c2);
    const int j = order[p];
    const double rcsq = rc * rc;
    bool hit = false;
    for (int a = c0 - 1; a <= c0 + 1 && !hit; ++a) {
        const int ca = pmod(a, g.nc[0]);
        for (int bb = c1 - 1; bb <= c1 + 1 && !hit; ++bb) {
            const int64_t base = ((int64_t)ca * g.nc[1] + pmod(bb, g.nc[1])) * g.nc[2];
            for (int cc = c2 - 1; cc <= c2 + 1 && !hit; ++cc) {
                const int64_t cell = base + pmod(cc, g.nc[2]);
                for (int q = cell_start[cell]; q < cell_start[cell + 1]; ++q) {
                    if (order[q] >= j)
                        continue;
                    double xi = xs[q], yi = ys[q], zi = zs[q]; // the lower-numbered atom is the centre: wrapped (:430-436)
                    if (b.anypbc)
                        wrap<TRI>(b, xi, yi, zi);
                    double dx = xr - xi, dy = yr - yi, dz = zr - zi;
                    pbc<TRI>(b, dx, dy, dz);
                    if (dx * dx + dy * dy + dz * dz <= rcsq) { hit = true; break; }
                }
            }
        }
    }
    keep[j] = hit ? 0 : 1;
}

__global__ __launch_bounds__(256) void k_max_i32(const int *__restrict__ v, int64_t n, int *__restrict__ out)
{
    int m = 0;
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x) m = max(m, v[i]);
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) m = max(m, __shfl_xor(m, d, 64));
    if ((threadIdx.x & 63) == 0 && m > __hip_atomic_load(out, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT)) atomicMax(out, m);
}

// last exact row width seen for a (N, grid) signature; set < 0: query only
static int width_hint(int64_t N, int64_t ncell, int set)
{
    struct Entry { int64_t N, ncell; int width; };
    static std::mutex mu;
    static std::vector<Entry> table;
    std::lock_guard<std::mutex> lk(mu);
    for (auto &e : table)
        if (e.N == N && e.ncell == ncell) {
            if (set >= 0) e.width = set;
            return e.width;
        }
    if (set > 0) {
        if (table.size() >= 64) table.erase(table.begin());
        table.push_back(Entry{N, ncell, set});
    }
    return 0;
}

// One pass over a built cell grid (RowsRequest, grid.hpp).  The tile kernel where it applies, the round-1 tiled kernel for cells
// too full for it, the thread-per-atom code for the rest.
// labelled: the request's fixed-cutoff CNA labels were written by the tile kernel (the leftovers of its mop-up kernels are listed in
// todo); false: nothing was labelled, the whole analysis runs on the finished rows (launch_labels)
struct RowsDone { bool labelled = false; };
static int neighbor_pass(Scope &sc, const CellGrid &cg, const DBox &b, int64_t N, double rc, const RowsRequest &rows, RowsDone &out)
{
    hipStream_t st = sc.stream();
    const bool count = rows.pads == RowsRequest::COUNT_ONLY;
    out.labelled = false;
    if (!cg.flags_fresh) MDH_HIP(hipMemsetAsync(cg.flags + 2, 0, sizeof(int) * 2, st)); // the tile lists of this pass (flags[0], unwrapped input, stays)
    cg.flags_fresh = false;
    TileFilter tf{};
    tf.big_stamp = cg.big_stamp; tf.big_gen = cg.big_gen; tf.big_sink = cg.big_sink;
    bool done = false;
    if (g_neighbor_variant == 0) { // tile kernel (orthogonal and triclinic boxes); the thread-per-atom code below then only mops up what it listed
        GridStats gs;
        MDH_TRY(grid_stats_hint(sc, cg, N, &gs));
        const bool cna = rows.pattern && !count;
        const LanePlan lp = plan_lane(b, cg.g, N, count ? 1 : rows.M, gs, rc, cna, count);
        if (lp.txy) {
            if (cna) tf.cna_todo = rows.todo;
            MDH_TRY(launch_neighbor_lane(sc, cg, lp, N, b, rc, rows, tf));
            done = true;
            out.labelled = cna;
        }
    }
    // cells too full for the kernel above (or forced): the round-1 tiled kernel (a slot grid it does not read: the thread-per-atom kernel then)
    if (!done && !count && g_neighbor_variant != 1 && !b.tri && !cg.slot_cap) {
        int64_t occ = 0;
        MDH_TRY(occupied_cells_hint(sc, cg, N, &occ));
        const TiledPlan plan = plan_tiled(b, cg.g, N, rows.M, occ);
        if (plan.tile) {
            MDH_TRY(ensure_unpacked(sc, const_cast<CellGrid &>(cg), N));
            MDH_TRY(launch_neighbor_tiled(sc, cg, plan, N, b, rc, rows, tf));
        }
    }
    if (count) launch_neighbor<0>(st, cg, N, b, rc, nullptr, nullptr, rows.nn, 1, rows.max_count, tf);
    else if (rows.pads == RowsRequest::WRITE_PADS) launch_neighbor<2>(st, cg, N, b, rc, rows.verlet, rows.dist, rows.nn, rows.M, nullptr, tf);
    else launch_neighbor<1>(st, cg, N, b, rc, rows.verlet, rows.dist, rows.nn, rows.M, nullptr, tf);
    if (g_moved_probe) // mdh_debug_track_counters(1): the build's "image codes not valid" flag, for mdh_debug_counters
        MDH_HIP(hipMemcpyAsync(g_moved_probe, cg.flags, sizeof(int), hipMemcpyDeviceToHost, st));
    MDH_HIP(hipGetLastError());
    return MDH_OK;
}

// the grid of a build of neighbor rows of `row_width` slots (0: not known, or counting): atoms wrapped, cells in reference order
static GridRequest rows_grid(const int64_t *key, int64_t row_width)
{
    GridRequest rq;
    rq.wrap_first = rq.sort_desc = true; rq.sort_key = key; rq.atoms = GridRequest::FOR_ROWS;
    rq.row_width = (int)std::min<int64_t>(row_width, 1 << 20);
    rq.slots_ok = true; // (every kernel behind neighbor_pass reads a slot grid)
    return rq;
}

// The fixed-cutoff CNA labels behind a pass that was asked for them: of the atoms the tile kernel left on its to-do list where it
// labelled its own centres, of all atoms from the finished rows otherwise.  done: the kept block todo sits in
static int launch_labels(Scope &sc, const DBox &b, const double *dx, const double *dy, const double *dz, int64_t N, const RowsRequest &rows,
                          double rc, int *done, const RowsDone &pass)
{
    ProfRange pr("k_fcna", sc.stream());
    if (pass.labelled) launch_fcna_listed(sc.stream(), b, dx, dy, dz, N, rows.verlet, rows.M, rows.nn, rows.pattern, rc, rows.todo, done);
    else launch_fcna_all(sc.stream(), b, dx, dy, dz, N, rows.verlet, rows.M, rows.nn, rows.pattern, rc, rows.todo, done);
    MDH_HIP(hipGetLastError());
    sc.keep_confirm(done); // (the list's walker leaves the counters zero)
    return MDH_OK;
}

// grid.hpp
int neighbor_rows_device(Scope &sc, const double *dx, const double *dy, const double *dz, int64_t N, const DBox &b, double rc, int *dv,
                         double *dd, int *dn, int64_t M, const int64_t *dkey, bool ids_only)
{
    CellGrid cg;
    MDH_TRY(neighbor_grid_dims(b, rc, cg.g));
    MDH_TRY(build_cell_grid(sc, dx, dy, dz, N, b, rows_grid(dkey, M), cg));
    // pads written (the tile kernel then stores whole 16-byte groups; leaving the pads out measured SLOWER: 2.96 against 2.54 ms
    // at 10 M atoms, rc 3.8, 24 slots); distances wanted or not (rows of more than 16 slots: the wide instance skips them)
    RowsRequest rows;
    rows.verlet = dv; rows.dist = dd; rows.nn = dn; rows.M = M;
    rows.pads = RowsRequest::WRITE_PADS; rows.ids_only = ids_only;
    RowsDone pass;
    return neighbor_pass(sc, cg, b, N, rc, rows, pass);
}

int moved_probe(int enable) // enable > 0: start tracking; 0: stop; < 0: the last value (-1: none)
{
    if (enable > 0 && !g_moved_probe) {
        if (hipHostMalloc(reinterpret_cast<void **>(&g_moved_probe), sizeof(int), hipHostMallocDefault) != hipSuccess) { g_moved_probe = nullptr; return -1; }
        *g_moved_probe = -1;
    } else if (enable == 0 && g_moved_probe) {
        int *p = g_moved_probe;
        g_moved_probe = nullptr;
        (void)hipDeviceSynchronize();
        (void)hipHostFree(p);
    }
    return g_moved_probe ? *(volatile int *)g_moved_probe : -1;
}

} // namespace mdh

using namespace mdh;

extern "C" {

int mdh_build_neighbor(const double *x, const double *y, const double *z, int64_t N, const double *box9,
                       const double *origin3, const int *boundary3, double rc, int *verlet, double *dist, int *nn,
                       int64_t max_neigh, int fill_pads, int space, void *stream)
{
    return mdh_build_neighbor_keyed(x, y, z, N, box9, origin3, boundary3, rc, verlet, dist, nn, max_neigh, fill_pads, nullptr,
                                    space, stream);
}

// key (N) i64, or NULL: the atoms of a cell are listed by descending key instead of descending index
int mdh_build_neighbor_keyed(const double *x, const double *y, const double *z, int64_t N, const double *box9,
                             const double *origin3, const int *boundary3, double rc, int *verlet, double *dist, int *nn,
                             int64_t max_neigh, int fill_pads, const int64_t *key, int space, void *stream)
{
    return mdh_build_neighbor_fcna(x, y, z, N, box9, origin3, boundary3, rc, verlet, dist, nn, max_neigh, fill_pads, nullptr, key,
                                   space, stream);
}

// pattern (N) i32: mdh_build_neighbor followed by mdh_fcna with the same rc, in one pass over the tiles where the tile kernel
// applies; NULL: the rows alone (the two entry points above)
int mdh_build_neighbor_fcna(const double *x, const double *y, const double *z, int64_t N, const double *box9,
                            const double *origin3, const int *boundary3, double rc, int *verlet, double *dist, int *nn,
                            int64_t max_neigh, int fill_pads, int *pattern, const int64_t *key, int space, void *stream)
{
    if (N < 0 || N >= 2147483647LL || !(rc > 0) || max_neigh <= 0) { set_error(pattern ? "mdh_build_neighbor_fcna: invalid N, rc or max_neigh" : "mdh_build_neighbor: invalid N, rc or max_neigh"); return MDH_ERR_ARG; }
    DBox b;
    MDH_TRY(make_box(b, box9, origin3, boundary3));
    if (N == 0)
        return MDH_OK;
    Scope sc(stream);
    const double *dx = sc.stage_in(x, (size_t)N, space), *dy = sc.stage_in(y, (size_t)N, space), *dz = sc.stage_in(z, (size_t)N, space);
    RowsRequest rows;
    // host space + reference semantics: pads come from the caller's buffers, so they are uploaded too
    rows.verlet = sc.stage(verlet, (size_t)(N * max_neigh), space, !fill_pads, true);
    rows.dist = sc.stage(dist, (size_t)(N * max_neigh), space, !fill_pads, true);
    rows.nn = sc.stage(nn, (size_t)N, space, false, true);
    rows.M = max_neigh; rows.pads = fill_pads ? RowsRequest::WRITE_PADS : RowsRequest::KEEP_PADS;
    int *done = nullptr;
    if (pattern) {
        rows.pattern = sc.stage(pattern, (size_t)N, space, true, true); // atoms without 12 or 14 neighbours keep the caller's value (cna.cpp:456)
        // the to-do list of the labels (count first) in a kept block whose two counters — workgroups done (word 0), length (word 64) — are
        // zero whenever it is idle (the kernel that walks the list clears them when it leaves, cna.hip k_fcna): no memset per call
        done = static_cast<int *>(sc.alloc_kept(sizeof(int) * ((size_t)N + 1 + 64), Scope::KEEP_TODO));
        rows.todo = done ? done + 64 : nullptr;
    }
    const int64_t *dkey = key ? sc.stage_in(key, (size_t)N, space) : nullptr;
    if (sc.failed())
        return sc.error();
    CellGrid cg;
    MDH_TRY(neighbor_grid_dims(b, rc, cg.g));
    {
        ProfRange pr("cell_grid", sc.stream());
        MDH_TRY(build_cell_grid(sc, dx, dy, dz, N, b, rows_grid(dkey, max_neigh), cg));
    }
    RowsDone pass;
    {
        ProfRange pr("k_neighbor", sc.stream());
        MDH_TRY(neighbor_pass(sc, cg, b, N, rc, rows, pass));
    }
    if (pattern) MDH_TRY(launch_labels(sc, b, dx, dy, dz, N, rows, rc, done, pass));
    return sc.finish(space);
}

int mdh_debug_set_neighbor_variant(int v)
{
    g_neighbor_variant = v;
    return MDH_OK;
}

int mdh_neighbor_count(const double *x, const double *y, const double *z, int64_t N, const double *box9,
                       const double *origin3, const int *boundary3, double rc, int *nn, int *max_count, int space,
                       void *stream)
{
    if (N < 0 || N >= 2147483647LL || !(rc > 0) || !max_count) { set_error("mdh_neighbor_count: invalid N or rc"); return MDH_ERR_ARG; }
    DBox b;
    MDH_TRY(make_box(b, box9, origin3, boundary3));
    *max_count = 0;
    if (N == 0)
        return MDH_OK;
    Scope sc(stream);
    const double *dx = sc.stage_in(x, (size_t)N, space), *dy = sc.stage_in(y, (size_t)N, space), *dz = sc.stage_in(z, (size_t)N, space);
    int *dn = sc.stage(nn, (size_t)N, space, false, true);
    int *dmax = sc.alloc_n<int>(1);
    if (sc.failed())
        return sc.error();
    MDH_HIP(hipMemsetAsync(dmax, 0, sizeof(int), sc.stream()));
    CellGrid cg;
    MDH_TRY(neighbor_grid_dims(b, rc, cg.g));
    MDH_TRY(build_cell_grid(sc, dx, dy, dz, N, b, rows_grid(nullptr, 0), cg));
    RowsRequest counts;
    counts.nn = dn; counts.pads = RowsRequest::COUNT_ONLY; counts.max_count = dmax;
    RowsDone pass;
    MDH_TRY(neighbor_pass(sc, cg, b, N, rc, counts, pass));
    MDH_HIP(hipMemcpyAsync(max_count, dmax, sizeof(int), hipMemcpyDeviceToHost, sc.stream()));
    MDH_TRY(sc.finish(space));
    MDH_HIP(hipStreamSynchronize(sc.stream()));
    return MDH_OK;
}

// _neighbor.build_neighbor_without_max_neigh in one call: ONE cell grid serves the counting pass and the build
int mdh_build_neighbor_exact(const double *x, const double *y, const double *z, int64_t N, const double *box9,
                             const double *origin3, const int *boundary3, double rc, int *nn, int64_t *width,
                             mdh_alloc_rows_fn alloc, void *user, int space, void *stream)
{
    return mdh_build_neighbor_exact_keyed(x, y, z, N, box9, origin3, boundary3, rc, nn, width, alloc, user, nullptr, space, stream);
}

// key (N) i64, or NULL: as in mdh_build_neighbor_keyed
int mdh_build_neighbor_exact_keyed(const double *x, const double *y, const double *z, int64_t N, const double *box9,
                                   const double *origin3, const int *boundary3, double rc, int *nn, int64_t *width,
                                   mdh_alloc_rows_fn alloc, void *user, const int64_t *key, int space, void *stream)
{
    return mdh_build_neighbor_exact_fcna(x, y, z, N, box9, origin3, boundary3, rc, nn, width, alloc, user, nullptr, key, space, stream);
}

// pattern (N) i32 or NULL: the fixed-cutoff CNA labels of the same cutoff as well (mdh_build_neighbor_fcna at the exact width)
int mdh_build_neighbor_exact_fcna(const double *x, const double *y, const double *z, int64_t N, const double *box9,
                                  const double *origin3, const int *boundary3, double rc, int *nn, int64_t *width,
                                  mdh_alloc_rows_fn alloc, void *user, int *pattern, const int64_t *key, int space, void *stream)
{
    if (N < 0 || N >= 2147483647LL || !(rc > 0) || !width || !alloc) { set_error("mdh_build_neighbor_exact: invalid N, rc, width or allocator"); return MDH_ERR_ARG; }
    DBox b;
    MDH_TRY(make_box(b, box9, origin3, boundary3));
    int *verlet = nullptr;
    double *dist = nullptr;
    *width = 1; // neighbor.cpp:301-304: at least one column
    if (N == 0) {
        if (alloc(user, 0, 1, &verlet, &dist) != 0) { set_error("mdh_build_neighbor_exact: the row allocator failed"); return MDH_ERR_NOMEM; }
        return MDH_OK;
    }
    Scope sc(stream);
    const double *dx = sc.stage_in(x, (size_t)N, space), *dy = sc.stage_in(y, (size_t)N, space), *dz = sc.stage_in(z, (size_t)N, space);
    int *dn = sc.stage(nn, (size_t)N, space, false, true);
    int *dmax = sc.alloc_n<int>(1);
    const int64_t *dkey = key ? sc.stage_in(key, (size_t)N, space) : nullptr;
    RowsRequest rows; // the build at a width (pads written); verlet, dist and M are set when the rows exist
    rows.nn = dn;
    rows.pattern = pattern ? sc.stage(pattern, (size_t)N, space, true, true) : nullptr; // atoms without 12 or 14 neighbours keep the caller's value (cna.cpp:456)
    int *done = pattern ? static_cast<int *>(sc.alloc_kept(sizeof(int) * ((size_t)N + 1 + 64), Scope::KEEP_TODO)) : nullptr; // (as in mdh_build_neighbor_fcna)
    rows.todo = done ? done + 64 : nullptr;
    RowsRequest counts;
    counts.nn = dn; counts.pads = RowsRequest::COUNT_ONLY; counts.max_count = dmax;
    if (sc.failed())
        return sc.error();
    hipStream_t st = sc.stream();
    MDH_HIP(hipMemsetAsync(dmax, 0, sizeof(int), st));
    // an absent atom (x = NaN) takes no cell and no kernel writes its count: 0, not what the caller's buffer held — the width below is
    // the largest count of ALL N entries, and the labels behind the build read every atom's
    MDH_HIP(hipMemsetAsync(dn, 0, (size_t)N * sizeof(int), st));
    CellGrid cg;
    MDH_TRY(neighbor_grid_dims(b, rc, cg.g));
    {
        ProfRange pr("cell_grid", st);
        // (row width: what the last build of this (N, grid) found; 0: none yet)
        MDH_TRY(build_cell_grid(sc, dx, dy, dz, N, b, rows_grid(dkey, width_hint(N, cg.g.ncell, -1)), cg));
    }
    RowsDone pass;
    // Width hint: the largest count the previous call with the same (N, grid) found.  A sequence of calls on one system (a
    // trajectory, the same analysis repeated) almost always finds the same maximum again, so the rows are built at that
    // width at once and the counts written by the build confirm it — the counting pass is skipped.  A wrong hint costs one
    // wasted build (the counts are then known) and is replaced; results never depend on it.
    int hmax = 0;
    const int hint = space == MDH_DEVICE ? width_hint(N, cg.g.ncell, -1) : 0; // (host buffers: a discarded first allocation would still be a copy-back target)
    bool built = false;
    // rows of width M from the caller's allocator, the build, its labels.  confirm: the largest count goes to hmax behind the build
    auto build_rows = [&](int64_t M, bool confirm) {
        if (alloc(user, N, M, &verlet, &dist) != 0 || !verlet || !dist) { set_error("mdh_build_neighbor_exact: the row allocator failed"); return MDH_ERR_NOMEM; }
        rows.verlet = sc.stage(verlet, (size_t)(N * M), space, false, true);
        rows.dist = sc.stage(dist, (size_t)(N * M), space, false, true);
        rows.M = M;
        if (sc.failed())
            return sc.error();
        {
            ProfRange pr("k_neighbor", st);
            MDH_TRY(neighbor_pass(sc, cg, b, N, rc, rows, pass));
            if (confirm) {
                hipLaunchKernelGGL(k_max_i32, dim3(1024), dim3(256), 0, st, dn, N, dmax);
                MDH_HIP(hipMemcpyAsync(&hmax, dmax, sizeof(int), hipMemcpyDeviceToHost, st));
            }
        }
        return pattern ? launch_labels(sc, b, dx, dy, dz, N, rows, rc, done, pass) : MDH_OK;
    };
    if (hint > 0) {
        // (the labels are enqueued before the width is known: with a confirmed hint — the usual case — the call has no idle gap; after a
        // wrong one the second build labels again, and a label depends on the atom's neighbours only, not on the width of the rows: an
        // atom the wasted pass labelled had its 12 or 14 neighbours listed in full, anything else it left to the list)
        MDH_TRY(build_rows(hint, /*confirm=*/true));
        MDH_HIP(hipStreamSynchronize(st));
        built = (hmax > 1 ? hmax : 1) == hint;
    } else {
        ProfRange pr("k_neighbor_count", st);
        MDH_TRY(neighbor_pass(sc, cg, b, N, rc, counts, pass));
        MDH_HIP(hipMemcpyAsync(&hmax, dmax, sizeof(int), hipMemcpyDeviceToHost, st));
        MDH_HIP(hipStreamSynchronize(st));
    }
    const int64_t M = hmax > 1 ? hmax : 1;
    *width = M;
    width_hint(N, cg.g.ncell, (int)(M <= 4096 ? M : 0));
    if (!built) MDH_TRY(build_rows(M, /*confirm=*/false));
    MDH_HIP(hipGetLastError());
    return sc.finish(space);
}

int mdh_filter_overlap_atom(const double *x, const double *y, const double *z, int64_t N, const double *box9,
                            const double *origin3, const int *boundary3, double rc, unsigned char *keep, int space,
                            void *stream)
{
    if (N < 0 || N >= 2147483647LL || !(rc > 0)) { set_error("mdh_filter_overlap_atom: invalid N or rc"); return MDH_ERR_ARG; }
    DBox b;
    MDH_TRY(make_box(b, box9, origin3, boundary3));
    if (N == 0)
        return MDH_OK;
    Scope sc(stream);
    const double *dx = sc.stage_in(x, (size_t)N, space), *dy = sc.stage_in(y, (size_t)N, space), *dz = sc.stage_in(z, (size_t)N, space);
    unsigned char *dk = sc.stage(keep, (size_t)N, space, false, true);
    if (sc.failed())
        return sc.error();
    CellGrid cg;
    MDH_TRY(neighbor_grid_dims(b, rc, cg.g));
    GridRequest rq; rq.wrap_first = true; // sorted coordinate arrays, cells in any order
    MDH_TRY(build_cell_grid(sc, dx, dy, dz, N, b, rq, cg));
    if (b.tri)
        hipLaunchKernelGGL(k_filter_overlap<true>, dim3(grid_for(N, 256)), dim3(256), 0, sc.stream(), cg.xs, cg.ys, cg.zs, cg.order, cg.cell_start, N, b, cg.g, rc, dk);
    else
        hipLaunchKernelGGL(k_filter_overlap<false>, dim3(grid_for(N, 256)), dim3(256), 0, sc.stream(), cg.xs, cg.ys, cg.zs, cg.order, cg.cell_start, N, b, cg.g, rc, dk);
    return sc.finish(space);
}

int mdh_sort_verlet_by_distance(int *verlet, double *dist, int64_t N, int64_t M, int sort_num, int space, void *stream)
{
    if (N < 0 || M <= 0) { set_error("mdh_sort_verlet_by_distance: invalid shape"); return MDH_ERR_ARG; }
    if (N == 0 || sort_num <= 0)
        return MDH_OK;
    Scope sc(stream);
    int *dv = sc.stage(verlet, (size_t)(N * M), space, true, true);
    double *dd = sc.stage(dist, (size_t)(N * M), space, true, true);
    if (sc.failed())
        return sc.error();
    const int k = (int)(sort_num < M ? sort_num : M);
    if (M == 1)
        return sc.finish(space);
    if (M > SORT_LDS_WIDEST) { // (the reference's selection sort, neighbor.cpp: its order among EQUAL distances — a perfect lattice — is part of the result)
        hipLaunchKernelGGL(k_sort_rows_wide, dim3(grid_for(N, 256)), dim3(256), 0, sc.stream(), dv, dd, N, M, k);
        return sc.finish(space);
    }
    int L = 1; // lanes to a row: the fewest that keep the rows of a wave within ~10 KB of LDS
    while (L < 16 && (size_t)(64 / L) * M * 12 > 10 * 1024) L <<= 1;
    const size_t lds = (size_t)(64 / L) * M * 12;
    const unsigned inv_m = (unsigned)((0x100000000ull + (uint64_t)M - 1) / (uint64_t)M);
    const dim3 grid(grid_for(N, 64 / L)), block(64);
    switch (L) {
    case 1: hipLaunchKernelGGL(k_sort_rows<1>, grid, block, lds, sc.stream(), dv, dd, N, (int)M, k, inv_m); break;
    case 2: hipLaunchKernelGGL(k_sort_rows<2>, grid, block, lds, sc.stream(), dv, dd, N, (int)M, k, inv_m); break;
    case 4: hipLaunchKernelGGL(k_sort_rows<4>, grid, block, lds, sc.stream(), dv, dd, N, (int)M, k, inv_m); break;
    case 8: hipLaunchKernelGGL(k_sort_rows<8>, grid, block, lds, sc.stream(), dv, dd, N, (int)M, k, inv_m); break;
    default: hipLaunchKernelGGL(k_sort_rows<16>, grid, block, lds, sc.stream(), dv, dd, N, (int)M, k, inv_m); break;
    }
    return sc.finish(space);
}

extern "C++" {
namespace mdh {
// Whole rows in HBM by ascending distance, equal distances by id — NOT the reference's order among equal distances (that is the
// selection sort above, quadratic in the row length): for the Voronoi search lists, whose cells do not depend on the order of
// equidistant planes.  Rows of 161 ... 8192 entries: one workgroup per row, a bitonic network in LDS.
int sort_rows_any_tie_order(int *dv, double *dd, int64_t N, int64_t M, void *stream)
{
    if (N <= 0 || M <= 0)
        return MDH_OK;
    if (M <= 80 || M > SORT_BLOCK_MAX) // (whole rows: the selection is quadratic in the row length, the network is not)
        return mdh_sort_verlet_by_distance(dv, dd, N, M, (int)M, MDH_DEVICE, stream);
    int P = 256;
    while (P < M) P <<= 1;
    const size_t bytes = (size_t)P * 12;
    if (bytes > 48 * 1024)
        MDH_HIP(hipFuncSetAttribute((const void *)k_sort_rows_block, hipFuncAttributeMaxDynamicSharedMemorySize, (int)bytes));
    hipLaunchKernelGGL(k_sort_rows_block, dim3((unsigned)N), dim3(256), bytes, static_cast<hipStream_t>(stream), dv, dd, M, P);
    MDH_HIP(hipGetLastError());
    return MDH_OK;
}
} // namespace mdh
} // extern "C++"

int mdh_wrap_positions(double *x, double *y, double *z, int64_t N, const double *box9, const double *origin3,
                       const int *boundary3, int space, void *stream)
{
    DBox b;
    MDH_TRY(make_box(b, box9, origin3, boundary3));
    if (N <= 0)
        return MDH_OK;
    Scope sc(stream);
    double *dx = sc.stage(x, (size_t)N, space, true, true), *dy = sc.stage(y, (size_t)N, space, true, true), *dz = sc.stage(z, (size_t)N, space, true, true);
    if (sc.failed())
        return sc.error();
    if (b.tri)
        hipLaunchKernelGGL(k_wrap<true>, dim3(grid_for(N, 256)), dim3(256), 0, sc.stream(), dx, dy, dz, N, b);
    else
        hipLaunchKernelGGL(k_wrap<false>, dim3(grid_for(N, 256)), dim3(256), 0, sc.stream(), dx, dy, dz, N, b);
    return sc.finish(space);
}

int mdh_average_by_neighbor(double rc, const int *verlet, const double *dist, const int *nn, int64_t N, int64_t M,
                            const double *value, double *value_ave, int include_self, int space, void *stream)
{
    if (N <= 0)
        return MDH_OK;
    Scope sc(stream);
    const int *dv = sc.stage_in(verlet, (size_t)(N * M), space);
    const double *dd = sc.stage_in(dist, (size_t)(N * M), space);
    const int *dn = sc.stage_in(nn, (size_t)N, space);
    const double *dval = sc.stage_in(value, (size_t)N, space);
    double *dout = sc.stage(value_ave, (size_t)N, space, false, true);
    if (sc.failed())
        return sc.error();
    hipLaunchKernelGGL(k_average, dim3(grid_for(N, 64)), dim3(64), 0, sc.stream(), rc, dv, dd, dn, N, M, dval, dout, include_self);
    return sc.finish(space);
}
}

MDH_WARM_UNIT(neighbor)

