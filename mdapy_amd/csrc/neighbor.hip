// neighbor.hip — cell-list cutoff neighbor search on gfx950: the thread-per-atom and wave-per-atom kernels, the pass over a built
// cell grid (cell_grid.hip) that chooses among them and the tile kernels (neighbor_lane.hip, neighbor_tiled.hip), and the C entry
// points of the build.  Replaces src/neighbor.cpp of the reference (build_verlet_list :102-187, build_neighbor :351-388, the
// exact-width variant :189-349); the row utilities behind a finished list are in rows.hip.
//
// Data layout in HBM: x,y,z f64[N] (SoA, original atom order); verlet int32[N][M], dist f64[N][M], nn int32[N] —
// rows in ORIGINAL atom order; scratch: the cell grid (CellGrid in grid.hpp).
#include "common.hpp"
#include "grid.hpp"
#include "cna_core.hpp"
#include <algorithm>

namespace mdh {

static int *g_moved_probe = nullptr; // pinned: flags[0] of the last tracked neighbor pass (mdh_debug_track_counters)
int g_neighbor_variant = 0; // 0 = automatic, 1 = force the thread-per-atom kernel, any other value = no tile kernel of neighbor_lane.hip: the round-1 LDS-tiled kernel where it applies (tests pass 2)

// ----------------------------------------------------------------------------
// 27-cell scan, one thread per centre atom (centres taken in cell order so the
// lanes of a wave share their candidate cells through L1/L2), or one wave.
//   MODE 0: count only            (first pass of the exact-width variant)
//   MODE 1: reference semantics   (write valid slots only, caller pre-filled pads)
//   MODE 2: also write the pads   (-1, rc + 1)
// The cells come through a CellView (grid.hpp): the walk and the grid's two forms are there, the row's semantics here.
// ----------------------------------------------------------------------------
// one centre atom, wrapped (neighbor.cpp:139-142), and its row: the candidate test, the row store and the epilogue of neighbor.cpp:139-177
template <bool TRI, int MODE>
struct Centre {
    const DBox &b;
    int i; // its id
    double xi, yi, zi, rcsq;
    int *__restrict__ verlet;
    double *__restrict__ dist;
    int64_t row, M; // the row starts at verlet[row], dist[row]

    __device__ __forceinline__ Centre(const DBox &b_, int i_, double x, double y, double z, double rc, int *v, double *d, int64_t M_)
        : b(b_), i(i_), xi(x), yi(y), zi(z), rcsq(rc * rc), verlet(v), dist(d), row((int64_t)i_ * M_), M(M_) {} // neighbor.cpp:127
    // is atom j at (xq, yq, zq) a neighbour?  d2: its squared distance
    __device__ __forceinline__ bool hit(int j, double xq, double yq, double zq, double &d2) const
    {
        double dx = xq - xi, dy = yq - yi, dz = zq - zi; // raw x[j] - wrapped centre, :164-166
        pbc<TRI>(b, dx, dy, dz);
        d2 = dx * dx + dy * dy + dz * dz;
        return j != i && d2 <= rcsq;
    }
    // neighbour number `col` of the row (the count keeps running past M, the row does not)
    __device__ __forceinline__ void store(int64_t col, int j, double d2) const
    {
        if (MODE != 0 && col < M) {
            verlet[row + col] = j;
            dist[row + col] = sqrt(d2);
        }
    }
    // the count, and the pads behind it: lane `lane` of `stride` that share the row (a thread: 0 of 1, a wave: lane of 64)
    __device__ __forceinline__ void finish(int *__restrict__ nn, double rc, int cnt, int lane, int stride) const
    {
        if (lane == 0) nn[i] = cnt;
        if (MODE == 2) {
            const double pad = rc + 1.0;
            for (int64_t n = cnt + lane; n < M; n += stride) {
                verlet[row + n] = -1;
                dist[row + n] = pad;
            }
        }
    }
};

// an overflowed cell of a slot grid: its atoms one by one in descending id, by a thread or by every lane of a wave alike; store: this
// lane writes the row (a wave: lane 0).  Returns the running count
template <bool TRI, int MODE, bool SLOT>
__device__ __forceinline__ int overflowed_cell(const CellView<SLOT> &cv, const Centre<TRI, MODE> &c, int64_t cell, int cnt, bool store)
{
    for (int j = cv.next_id_below(cell, 0x7fffffff); j >= 0; j = cv.next_id_below(cell, j)) {
        double d2;
        if (!c.hit(j, cv.sv.xs[j], cv.sv.ys[j], cv.sv.zs[j], d2))
            continue;
        if (store) c.store(cnt, j, d2);
        ++cnt;
    }
    return cnt;
}

// the reference's 27-cell walk by one thread
template <bool TRI, int MODE, bool SLOT>
__device__ __forceinline__ int neighbor_one(const CellView<SLOT> &cv, const Grid &g, const Centre<TRI, MODE> &c, double rc,
                                            int *__restrict__ nn, int c0, int c1, int c2)
{
    int cnt = 0;
    cv.for_each_piece(g, c0, c1, c2, [&](const CellPiece &pc) {
        if (cv.overflowed(pc)) {
            cnt = overflowed_cell(cv, c, pc.at, cnt, true);
            return;
        }
        // four candidates per trip, their loads issued together (SortedView::get4): with one candidate per trip every one of them is a
        // dependent L2 round trip (the loop carries the row count through a store), and a thread of the mop-up kernel in
        // a fat cell at the box's far faces walks a thousand of them — 0.54 ms for the 3 % of a 3.4 M-atom box at rc = 5 A
        for (int k0 = 0; k0 < pc.n; k0 += 4) {
            double xq[4], yq[4], zq[4], d2;
            int jq[4];
            int64_t q[4];
#pragma unroll
            for (int u = 0; u < 4; ++u) q[u] = cv.pos(pc, min(k0 + u, pc.n - 1)); // (past the end of the piece: its last candidate again, not looked at)
            cv.sv.get4(q, xq, yq, zq, jq);
#pragma unroll
            for (int u = 0; u < 4; ++u)
                if (k0 + u < pc.n && c.hit(jq[u], xq[u], yq[u], zq[u], d2)) c.store(cnt++, jq[u], d2);
        }
    });
    c.finish(nn, rc, cnt, 0, 1);
    return cnt;
}

// The same walk by a whole wavefront for ONE atom: 64 candidates per trip, the hits' slots from a ballot (candidate order = row
// order, as above).  For the listed tiles of the mop-up kernel: their atoms sit in the fat last cells of the box, a thread walks
// 300 ... 1000 candidates there four at a time (80 ... 380 dependent trips), a wave 9 runs of one to three trips.
template <bool TRI, int MODE, bool SLOT>
__device__ __forceinline__ int neighbor_one_wave(const CellView<SLOT> &cv, const Grid &g, const Centre<TRI, MODE> &c, double rc,
                                                 int *__restrict__ nn, int c0, int c1, int c2)
{
    const int lane = (int)(threadIdx.x & 63);
    int cnt = 0;
    cv.for_each_piece(g, c0, c1, c2, [&](const CellPiece &pc) {
        if (cv.overflowed(pc)) { // every lane walks the same candidates and counts, lane 0 writes
            cnt = overflowed_cell(cv, c, pc.at, cnt, lane == 0);
            return;
        }
        for (int k0 = 0; k0 < pc.n; k0 += 64) { // (a cell's slots: one trip)
            const int k = k0 + lane;
            bool hit = false;
            int j = -1;
            double d2 = 0.0;
            if (k < pc.n) {
                double xq, yq, zq;
                cv.sv.get(cv.pos(pc, k), xq, yq, zq, j);
                hit = c.hit(j, xq, yq, zq, d2);
            }
            const unsigned long long m = __ballot(hit);
            if (hit) c.store(cnt + __popcll(m & ((1ull << lane) - 1ull)), j, d2);
            cnt += __popcll(m);
        }
    });
    c.finish(nn, rc, cnt, lane, 64);
    return cnt;
}

template <bool TRI, int MODE, bool SLOT>
__device__ __forceinline__ void neighbor_atoms_body(const CellView<SLOT> &cv, int64_t N, const DBox &b, const Grid &g,
                                                  double rc, int *__restrict__ verlet, double *__restrict__ dist,
                                                  int *__restrict__ nn, int64_t M, int *__restrict__ max_count,
                                                  const TileFilter &tf)
{
    const bool take_all = tf.moved && *tf.moved != 0; // the tiled kernel stood down: this kernel does the whole call
    if (tf.flag && !take_all && (tf.list || *tf.any == 0)) // nothing to mop up here (flagged tiles go to k_neighbor_tiles when listed)
        return;
    int cnt = 0;
    // the grid is capped (a stand-by launch then costs a few thousand workgroups that leave at once, not N / 256 of them):
    // a workgroup strides over the centres
    N = cv.centres(N, g);
    for (int64_t base = (int64_t)blockIdx.x * blockDim.x; base < N; base += (int64_t)gridDim.x * blockDim.x) {
        const int64_t p = base + threadIdx.x;
        int i = -1, c0 = 0, c1 = 0, c2 = 0;
        double xi = 0, yi = 0, zi = 0;
        if (p < N) i = cv.centre(p, xi, yi, zi);
        bool mine = i >= 0;
        if (mine) {
            if (b.anypbc) // neighbor.cpp:139-142
                wrap<TRI>(b, xi, yi, zi);
            cell_coords<TRI>(b, g, xi, yi, zi, c0, c1, c2);
            if (tf.flag) { // fallback pass: only atoms of tiles the LDS-tiled kernel could not hold (or all of them when it stood down)
                const int t = ((c0 / tf.tile) * tf.nt[1] + (c1 / tf.tile)) * tf.nt[2] + (c2 / tf.tile_z);
                mine = take_all || tf.flag[t] != 0;
            }
        }
        if (mine) {
            cnt = max(cnt, neighbor_one(cv, g, Centre<TRI, MODE>(b, i, xi, yi, zi, rc, verlet, dist, M), rc, nn, c0, c1, c2));
            if (tf.cna_todo) defer(tf.cna_todo, i);
        }
    }
    if (MODE == 0) raise_max(max_count, wave_max(cnt));
}

// mop-up of the tiles the wave kernel listed (halo over the LDS budget, atoms far outside the box): a workgroup per listed
// tile, its threads over the tile's centre atoms — the cost follows the number of listed tiles, not N
template <bool TRI, int MODE, bool SLOT>
__global__ __launch_bounds__(256) void k_neighbor(SortedView sv, const int *__restrict__ cell_start, int64_t N, DBox b, Grid g, double rc,
                                                  int *__restrict__ verlet, double *__restrict__ dist, int *__restrict__ nn, int64_t M,
                                                  int *__restrict__ max_count, TileFilter tf, SlotSpill sp)
{
    if (tf.big_sink && blockIdx.x == 0 && threadIdx.x == 0)
        *tf.big_sink = *tf.big_stamp == tf.big_gen ? 1 : 0; // (pinned host memory: the history of the slot grid, CellGrid::big_sink)
    neighbor_atoms_body<TRI, MODE>(CellView<SLOT>{sv, cell_start, sp}, N, b, g, rc, verlet, dist, nn, M, max_count, tf);
}

template <bool TRI, int MODE, bool SLOT>
__device__ __forceinline__ void neighbor_tiles_body(const CellView<SLOT> &cv, const DBox &b, const Grid &g, double rc,
                                                        int *__restrict__ verlet, double *__restrict__ dist, int *__restrict__ nn,
                                                        int64_t M, int *__restrict__ max_count, const TileFilter &tf)
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
        if (a >= g.nc[0] || c >= g.nc[1])
            continue;
        // this wave takes every (nwave * MOP_CHUNKS)-th centre of the column
        cv.for_each_column_centre(((int64_t)a * g.nc[1] + c) * g.nc[2], z0, z1, chunk * nwave + wave, nwave * MOP_CHUNKS, [&](int64_t p) {
            double xi, yi, zi;
            const int i = cv.centre(p, xi, yi, zi);
            if (i < 0)
                return;
            if (b.anypbc)
                wrap<TRI>(b, xi, yi, zi);
            int c0, c1, c2;
            cell_coords<TRI>(b, g, xi, yi, zi, c0, c1, c2);
            best = max(best, neighbor_one_wave(cv, g, Centre<TRI, MODE>(b, i, xi, yi, zi, rc, verlet, dist, M), rc, nn, c0, c1, c2));
            if (tf.cna_todo && (threadIdx.x & 63) == 0) defer(tf.cna_todo, i);
        });
    }
    if (MODE == 0) raise_max(max_count, wave_max(best));
}

template <bool TRI, int MODE, bool SLOT>
__global__ __launch_bounds__(256) void k_neighbor_tiles(SortedView sv, const int *__restrict__ cell_start, DBox b, Grid g, double rc,
                                                        int *__restrict__ verlet, double *__restrict__ dist, int *__restrict__ nn, int64_t M,
                                                        int *__restrict__ max_count, TileFilter tf, SlotSpill sp)
{
    neighbor_tiles_body<TRI, MODE>(CellView<SLOT>{sv, cell_start, sp}, b, g, rc, verlet, dist, nn, M, max_count, tf);
}

// the two stand-bys behind a tile kernel that lists its leftovers, as ONE launch (a launch that finds nothing to do costs
// ~4 us): the whole call atom by atom if the tile kernel stood down (unwrapped input), else the listed tiles
template <bool TRI, int MODE, bool SLOT>
__global__ __launch_bounds__(256) void k_neighbor_mop(SortedView sv, const int *__restrict__ cell_start, int64_t N, DBox b, Grid g, double rc,
                                                      int *__restrict__ verlet, double *__restrict__ dist, int *__restrict__ nn, int64_t M,
                                                      int *__restrict__ max_count, TileFilter tf, SlotSpill sp)
{
    if (tf.listed_sink && blockIdx.x == 0 && threadIdx.x == 0)
        *tf.listed_sink = min(*tf.any, tf.list_cap); // (pinned host memory: the next build of this (N, grid) launches the slice pass if anything was listed)
    if (tf.big_sink && blockIdx.x == 0 && threadIdx.x == 0)
        *tf.big_sink = *tf.big_stamp == tf.big_gen ? 1 : 0; // (pinned host memory: the history of the slot grid, CellGrid::big_sink)
    const CellView<SLOT> cv{sv, cell_start, sp};
    if (tf.moved && *tf.moved != 0) neighbor_atoms_body<TRI, MODE>(cv, N, b, g, rc, verlet, dist, nn, M, max_count, tf);
    else neighbor_tiles_body<TRI, MODE>(cv, b, g, rc, verlet, dist, nn, M, max_count, tf);
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

__global__ __launch_bounds__(256) void k_max_i32(const int *__restrict__ v, int64_t n, int *__restrict__ out)
{
    int m = 0;
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x) m = max(m, v[i]);
    raise_max(out, wave_max(m));
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
    const int variant = g_neighbor_variant;
    GridStats gs; // both planners size their tiles by the signature's statistics
    if (variant != 1) MDH_TRY(grid_stats_hint(sc, cg, &gs));
    const bool cna = rows.pattern && !count;
    LanePlan lp{};
    if (variant == 0) lp = plan_lane_memo(lane_plan_in(b, cg.g, N, count ? 1 : rows.M, gs, rc, cna, count), gs);
    TiledPlan tp{};
    if (!lp.txy && variant != 1) { // (the tile kernel's plan, where there is one, is taken whatever this would say)
        TiledPlanIn ti{};
        for (int d = 0; d < 3; ++d) { ti.nc[d] = cg.g.nc[d]; ti.pbc[d] = b.pbc[d]; }
        ti.mode = cg.g.mode; ti.tri = b.tri; ti.ncell = cg.g.ncell; ti.N = N; ti.M = rows.M; ti.occupied_cells = gs.v[0];
        tp = plan_tiled(ti);
    }
    switch (choose_rows_front(variant, count, b.tri != 0, cg.slot_cap != 0, lp.txy != 0, tp.tile != 0)) {
    case RowsFront::LANE:
        if (cna) tf.cna_todo = rows.todo;
        MDH_TRY(launch_neighbor_lane(sc, cg, lp, gs, N, b, rc, rows, tf));
        out.labelled = cna;
        break;
    case RowsFront::TILED:
        MDH_TRY(ensure_unpacked(sc, const_cast<CellGrid &>(cg), N));
        MDH_TRY(launch_neighbor_tiled(sc, cg, tp, N, b, rc, rows, tf));
        break;
    case RowsFront::ATOMS_ONLY:
        break;
    }
    if (count) launch_neighbor<0>(st, cg, N, b, rc, nullptr, nullptr, rows.nn, 1, rows.max_count, tf);
    else if (rows.pads == RowsRequest::WRITE_PADS) launch_neighbor<2>(st, cg, N, b, rc, rows.verlet, rows.dist, rows.nn, rows.M, nullptr, tf);
    else launch_neighbor<1>(st, cg, N, b, rc, rows.verlet, rows.dist, rows.nn, rows.M, nullptr, tf);
    if (g_moved_probe) // mdh_debug_track_counters(1): the build's "image codes not valid" flag, for mdh_debug_counters
        MDH_HIP(hipMemcpyAsync(g_moved_probe, cg.flags, sizeof(int), hipMemcpyDeviceToHost, st));
    MDH_HIP(hipGetLastError());
    return MDH_OK;
}

// the grid of a build of neighbor rows of `row_width` slots (0: not known, or counting; < 0: GridRequest::row_width): atoms wrapped, cells in reference order
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
        // (row width: what the last build of this signature found, GridFeedback::width)
        MDH_TRY(build_cell_grid(sc, dx, dy, dz, N, b, rows_grid(dkey, -1), cg));
    }
    RowsDone pass;
    // Width hint: the largest count the previous call with the same (N, grid) found.  A sequence of calls on one system (a
    // trajectory, the same analysis repeated) almost always finds the same maximum again, so the rows are built at that
    // width at once and the counts written by the build confirm it — the counting pass is skipped.  A wrong hint costs one
    // wasted build (the counts are then known) and is replaced; results never depend on it.
    int hmax = 0;
    const int hint = space == MDH_DEVICE ? cg.fb->width.load(std::memory_order_relaxed) : 0; // (host buffers: a discarded first allocation would still be a copy-back target)
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
    cg.fb->width.store((int)(M <= 4096 ? M : 0), std::memory_order_relaxed);
    if (!built) MDH_TRY(build_rows(M, /*confirm=*/false));
    MDH_HIP(hipGetLastError());
    return sc.finish(space);
}
}

MDH_WARM_UNIT(neighbor)

