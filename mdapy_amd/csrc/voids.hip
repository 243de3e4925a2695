// voids.hip — void analysis (src/mdapy/void_analysis.py; _neighbor._fill_cell_for_void, src/neighbor.cpp:780-839): which cells of
// the rc-wide grid hold no atom, the centres of those cells as an ordered list of points, and — after the points have been
// clustered — the points of the clusters of more than one point, renumbered.  DESIGN.md 5i.
//
// Nothing here depends on the order in which threads run: the occupancy kernel's lanes all store the same value, the two
// compactions take a point's slot from a prefix sum over the flags in index order (never from a counter that hands out slots as
// threads arrive), and the cluster sizes are integer sums.  The same input gives the same bits on every run.
#include "grid.hpp"
#include <cmath>

namespace mdh {

// ---- occupancy: one thread per atom; wrap (iff any axis is periodic, neighbor.cpp:818-821), cell (neighbor.cpp:29-62: the
// arithmetic of the cutoff neighbour build — common.hpp wrap, grid.hpp cell_coords, mode 0), a plain 32-bit store of 1.  Every
// lane that hits a cell stores the same word: no atomics.  A NaN coordinate lands in plane 0 of its axis (cell_coords); every
// offset is inside the grid whatever the position, because cell_coords clamps in floating point before it converts.
template <bool TRI>
__global__ __launch_bounds__(256) void k_void_fill(const double *__restrict__ x, const double *__restrict__ y, const double *__restrict__ z,
                                                   int64_t N, DBox b, Grid g, int *__restrict__ cells)
{
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= N)
        return;
    double xi = x[i], yi = y[i], zi = z[i];
    if (b.anypbc) wrap<TRI>(b, xi, yi, zi);
    int c0, c1, c2;
    cell_coords<TRI>(b, g, xi, yi, zi, c0, c1, c2);
    cells[((int64_t)c0 * g.nc[1] + c1) * g.nc[2] + c2] = 1;
}

// flag[i] = 1 where cell i is empty (what the prefix sum ranks); any non-zero word counts as occupied
__global__ __launch_bounds__(256) void k_void_empty(const int *__restrict__ cells, int64_t n, unsigned *__restrict__ flag)
{
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) flag[i] = cells[i] == 0 ? 1u : 0u;
}

struct VoidGeom {
    double h[9], o[3];
    int n[3];
};

// Point rank[i] of every empty cell i = (i0, i1, i2), row-major: ((i + 0.5) / ncell) @ box + origin (void_analysis.py:77-79) — the
// centre of one of ncell EQUAL cells across the box, not of the rc-wide cell that was tested.  A division per axis (numpy
// divides), then the row-times-matrix sum in index order, then the origin; uncontracted (-ffp-contract=off).
__global__ __launch_bounds__(256) void k_void_points(const unsigned *__restrict__ flag, const int *__restrict__ rank, int64_t n, VoidGeom v,
                                                     double *__restrict__ cx, double *__restrict__ cy, double *__restrict__ cz,
                                                     int *__restrict__ cell, int64_t cap)
{
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n || !flag[i])
        return;
    const int64_t k = rank[i];
    if (k < 0 || k >= cap)
        return;
    const int64_t t = i / v.n[2];
    const int i2 = (int)(i - t * v.n[2]), i1 = (int)(t % v.n[1]), i0 = (int)(t / v.n[1]);
    const double f0 = ((double)i0 + 0.5) / (double)v.n[0], f1 = ((double)i1 + 0.5) / (double)v.n[1], f2 = ((double)i2 + 0.5) / (double)v.n[2];
    cx[k] = ((f0 * v.h[0] + f1 * v.h[3]) + f2 * v.h[6]) + v.o[0];
    cy[k] = ((f0 * v.h[1] + f1 * v.h[4]) + f2 * v.h[7]) + v.o[1];
    cz[k] = ((f0 * v.h[2] + f1 * v.h[5]) + f2 * v.h[8]) + v.o[2];
    if (cell) cell[k] = (int)i;
}

// ---- prune: sizes[c] = points of cluster c (ids 1 .. C; any other id belongs to no cluster and is dropped).  Points come in
// row-major cell order and a void's cells sit next to each other, so the lanes of a wave mostly name one or two clusters — and one
// void of half the box has every point of the system adding to ONE word, which takes ~90 adds per microsecond.  A wave therefore
// counts before it adds: per group of 64 points the first pending lane's id is broadcast and the lanes that share it are counted
// by a ballot; the count joins the wave's running (id, count) pair while the id stays the same, over VOID_SPAN groups (their
// loads issued together), and the pair is added when the id changes and at the end — one add per run of equal ids and wave.
// The pruning of the 911 217 points of one void: 0.197 ms with one add per group of 64, 0.056 ms this way (profiles/void.md).
constexpr int VOID_SPAN = 8;
__global__ __launch_bounds__(256) void k_void_sizes(const int *__restrict__ cid, int64_t M, int C, unsigned *__restrict__ sizes)
{
    const int lane = threadIdx.x & 63;
    const int64_t wave = ((int64_t)blockIdx.x * blockDim.x + threadIdx.x) >> 6;
    const int64_t base = wave * (64 * VOID_SPAN) + lane;
    int ids[VOID_SPAN];
#pragma unroll
    for (int g = 0; g < VOID_SPAN; ++g) {
        const int64_t i = base + 64 * g;
        ids[g] = i < M ? cid[i] : 0;
    }
    int run_id = 0; // (no cluster: the first id met starts a run, and nothing is added for this one)
    unsigned run = 0;
#pragma unroll
    for (int g = 0; g < VOID_SPAN; ++g) {
        const int id = ids[g];
        const bool on = (unsigned)id - 1u < (unsigned)C;
        unsigned long long todo = __ballot(on);
        while (todo) { // (wave-uniform)
            const int lid = __builtin_amdgcn_readfirstlane(__shfl(id, __builtin_ctzll(todo), 64));
            const unsigned long long same = __ballot(on && id == lid);
            const unsigned n = (unsigned)__builtin_popcountll(same);
            if (lid == run_id) {
                run += n;
            } else {
                if (run && lane == 0) atomicAdd(&sizes[run_id], run);
                run_id = lid;
                run = n;
            }
            todo &= ~same;
        }
    }
    if (run && lane == 0) atomicAdd(&sizes[run_id], run);
}

// keep[c] = 1 for the clusters of more than one point, c = 0 .. C (keep[0] = 0: ids start at 1); the prefix sum over it, plus 1,
// is a surviving cluster's new id: 1 .. k in ascending old id (void_analysis.py:92-93)
__global__ __launch_bounds__(256) void k_void_keep(const unsigned *__restrict__ sizes, int C, unsigned *__restrict__ keep)
{
    const int c = blockIdx.x * blockDim.x + threadIdx.x;
    if (c <= C) keep[c] = (c >= 1 && sizes[c] > 1u) ? 1u : 0u;
}

__global__ __launch_bounds__(256) void k_void_point_keep(const int *__restrict__ cid, int64_t M, int C, const unsigned *__restrict__ sizes,
                                                         unsigned *__restrict__ flag)
{
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= M)
        return;
    const int id = cid[i];
    flag[i] = ((unsigned)id - 1u < (unsigned)C && sizes[id] > 1u) ? 1u : 0u;
}

// the kept points in the order they had (void_analysis.py:96-98), with their cluster's new id
__global__ __launch_bounds__(256) void k_void_compact(const double *__restrict__ x, const double *__restrict__ y, const double *__restrict__ z,
                                                      const int *__restrict__ cid, const unsigned *__restrict__ flag, const int *__restrict__ rank,
                                                      const int *__restrict__ newid, int64_t M, double *__restrict__ ox, double *__restrict__ oy,
                                                      double *__restrict__ oz, int *__restrict__ oid)
{
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= M || !flag[i])
        return;
    const int64_t k = rank[i]; // (< M: a prefix sum of at most i ones)
    ox[k] = x[i]; oy[k] = y[i]; oz[k] = z[i];
    oid[k] = newid[cid[i]] + 1;
}

// the box of a void grid: rc > 0 and a cell that spans a volume, refused as ARGUMENT errors (the reference divides by both)
static int void_box(const char *who, const double *box9, const double *origin3, const int *boundary3, double rc, DBox &b, Grid &g)
{
    const std::string me(who);
    if (!box9 || !origin3 || !boundary3) { set_error(me + ": box, origin or boundary is NULL"); return MDH_ERR_ARG; }
    if (!(rc > 0.0) || !std::isfinite(rc)) { set_error(me + ": rc must be a positive number"); return MDH_ERR_ARG; }
    const double *m = box9;
    const double det = m[0] * (m[4] * m[8] - m[5] * m[7]) - m[1] * (m[3] * m[8] - m[5] * m[6]) + m[2] * (m[3] * m[7] - m[4] * m[6]);
    if (!std::isfinite(det) || std::fabs(det) < 1e-12) { set_error(me + ": the box is singular (its volume is zero)"); return MDH_ERR_ARG; }
    MDH_TRY(make_box(b, box9, origin3, boundary3));
    for (int d = 0; d < 3; ++d)
        if (b.thick[d] == 0.0 || !std::isfinite(b.thick[d])) { set_error(me + ": the box is singular (an axis has no thickness)"); return MDH_ERR_ARG; }
    const int rc_ = neighbor_grid_dims(b, rc, g); // max(floor(thickness / rc), 3) per axis; MDH_ERR_ARG beyond what int32 indexes
    if (rc_ != MDH_OK) set_error(me + ": " + std::string(mdh_last_error()));
    return rc_;
}

} // namespace mdh

using namespace mdh;

extern "C" {

int mdh_void_grid_dims(const double *box9, const double *origin3, const int *boundary3, double rc, int *ncell3_host)
{
    DBox b;
    Grid g;
    if (!ncell3_host) { set_error("mdh_void_grid_dims: ncell3_host is NULL"); return MDH_ERR_ARG; }
    MDH_TRY(void_box("mdh_void_grid_dims", box9, origin3, boundary3, rc, b, g));
    for (int d = 0; d < 3; ++d) ncell3_host[d] = g.nc[d];
    return MDH_OK;
}

int mdh_fill_cell_for_void(const double *x, const double *y, const double *z, int64_t N, const double *box9, const double *origin3,
                           const int *boundary3, double rc, int *cells, int64_t ncell, int space, void *stream)
{
    DBox b;
    Grid g;
    MDH_TRY(void_box("mdh_fill_cell_for_void", box9, origin3, boundary3, rc, b, g));
    if (N < 0 || (N > 0 && (!x || !y || !z))) { set_error("mdh_fill_cell_for_void: positions missing"); return MDH_ERR_ARG; }
    if (!cells || ncell != g.ncell) {
        set_error("mdh_fill_cell_for_void: the grid has " + std::to_string(g.ncell) + " cells (mdh_void_grid_dims), the buffer " + std::to_string(ncell));
        return MDH_ERR_ARG;
    }
    if (N > (int64_t)0x7fffffff * 256) { set_error("mdh_fill_cell_for_void: too many atoms for one launch"); return MDH_ERR_ARG; }
    Scope sc(stream);
    hipStream_t st = sc.stream();
    const double *dx = sc.stage_in(x, (size_t)N, space), *dy = sc.stage_in(y, (size_t)N, space), *dz = sc.stage_in(z, (size_t)N, space);
    int *dc = sc.stage(cells, (size_t)ncell, space, false, true);
    if (sc.failed())
        return sc.error();
    MDH_HIP(hipMemsetAsync(dc, 0, (size_t)ncell * sizeof(int), st));
    if (N > 0) {
        ProfRange pr("k_void_fill", st);
        if (b.tri)
            hipLaunchKernelGGL(k_void_fill<true>, dim3(grid_for(N, 256)), dim3(256), 0, st, dx, dy, dz, N, b, g, dc);
        else
            hipLaunchKernelGGL(k_void_fill<false>, dim3(grid_for(N, 256)), dim3(256), 0, st, dx, dy, dz, N, b, g, dc);
    }
    MDH_HIP(hipGetLastError());
    return sc.finish(space);
}

int mdh_void_points(const int *cells, int n0, int n1, int n2, const double *box9, const double *origin3, double *cx, double *cy, double *cz,
                    int *cell, int64_t cap, int64_t *count_host, int space, void *stream)
{
    if (!cells || n0 < 1 || n1 < 1 || n2 < 1) { set_error("mdh_void_points: no grid"); return MDH_ERR_ARG; }
    const double total = (double)n0 * (double)n1 * (double)n2;
    if (total > 2147483000.0) { set_error("mdh_void_points: more cells than int32 indexes"); return MDH_ERR_ARG; }
    if (!box9 || !origin3 || !count_host) { set_error("mdh_void_points: box, origin or count_host is NULL"); return MDH_ERR_ARG; }
    const bool points = cx || cy || cz || cell;
    if (points && (!cx || !cy || !cz || cap < 0)) { set_error("mdh_void_points: cx, cy and cz go together"); return MDH_ERR_ARG; }
    const int64_t n = (int64_t)n0 * n1 * n2;
    *count_host = 0;
    Scope sc(stream);
    hipStream_t st = sc.stream();
    const int *dc = sc.stage_in(cells, (size_t)n, space);
    unsigned *flag = sc.alloc_n<unsigned>((size_t)n);
    int *rank = sc.alloc_n<int>((size_t)n + 1);
    if (sc.failed())
        return sc.error();
    int found = 0;
    {
        ProfRange pr("void_rank", st);
        hipLaunchKernelGGL(k_void_empty, dim3(grid_for(n, 256)), dim3(256), 0, st, dc, n, flag);
        MDH_TRY(exclusive_scan_u32(sc, flag, rank, n));
    }
    MDH_HIP(hipMemcpyAsync(&found, rank + n, sizeof(int), hipMemcpyDeviceToHost, st));
    MDH_HIP(hipStreamSynchronize(st));
    *count_host = found;
    if (!points || found == 0)
        return sc.finish(space);
    if (found > cap) {
        set_error("mdh_void_points: " + std::to_string(found) + " empty cells, room for " + std::to_string(cap));
        return MDH_ERR_ARG;
    }
    double *dx = sc.stage(cx, (size_t)found, space, false, true), *dy = sc.stage(cy, (size_t)found, space, false, true),
           *dz = sc.stage(cz, (size_t)found, space, false, true);
    int *dcell = cell ? sc.stage(cell, (size_t)found, space, false, true) : nullptr;
    if (sc.failed())
        return sc.error();
    VoidGeom v;
    for (int k = 0; k < 9; ++k) v.h[k] = box9[k];
    for (int k = 0; k < 3; ++k) v.o[k] = origin3[k];
    v.n[0] = n0; v.n[1] = n1; v.n[2] = n2;
    {
        ProfRange pr("k_void_points", st);
        hipLaunchKernelGGL(k_void_points, dim3(grid_for(n, 256)), dim3(256), 0, st, flag, rank, n, v, dx, dy, dz, dcell, (int64_t)found);
    }
    MDH_HIP(hipGetLastError());
    return sc.finish(space);
}

int mdh_void_prune(const double *x, const double *y, const double *z, const int *cluster_id, int64_t M, int cluster_number, double *ox,
                   double *oy, double *oz, int *new_id, int64_t *kept_host, int *void_number_host, int space, void *stream)
{
    if (M < 0 || cluster_number < 0 || cluster_number == 0x7fffffff) { set_error("mdh_void_prune: bad sizes"); return MDH_ERR_ARG; }
    if (!kept_host || !void_number_host) { set_error("mdh_void_prune: kept_host or void_number_host is NULL"); return MDH_ERR_ARG; }
    *kept_host = 0;
    *void_number_host = 0;
    if (M == 0 || cluster_number == 0)
        return MDH_OK;
    if (!x || !y || !z || !cluster_id || !ox || !oy || !oz || !new_id) { set_error("mdh_void_prune: an array is NULL"); return MDH_ERR_ARG; }
    if (M > 2147483000) { set_error("mdh_void_prune: more points than int32 indexes"); return MDH_ERR_ARG; }
    const int C = cluster_number;
    Scope sc(stream);
    hipStream_t st = sc.stream();
    const double *dx = sc.stage_in(x, (size_t)M, space), *dy = sc.stage_in(y, (size_t)M, space), *dz = sc.stage_in(z, (size_t)M, space);
    const int *did = sc.stage_in(cluster_id, (size_t)M, space);
    double *dox = sc.stage(ox, (size_t)M, space, false, true), *doy = sc.stage(oy, (size_t)M, space, false, true),
           *doz = sc.stage(oz, (size_t)M, space, false, true);
    int *doid = sc.stage(new_id, (size_t)M, space, false, true);
    unsigned *sizes = sc.alloc_n<unsigned>((size_t)C + 1), *keep = sc.alloc_n<unsigned>((size_t)C + 1), *flag = sc.alloc_n<unsigned>((size_t)M);
    int *newid = sc.alloc_n<int>((size_t)C + 2), *rank = sc.alloc_n<int>((size_t)M + 1);
    if (sc.failed())
        return sc.error();
    const dim3 block(256), pgrid(grid_for(M, 256)), cgrid(grid_for((int64_t)C + 1, 256)), sgrid(grid_for(M, 256 * VOID_SPAN));
    {
        ProfRange pr("void_prune", st);
        MDH_HIP(hipMemsetAsync(sizes, 0, ((size_t)C + 1) * sizeof(unsigned), st));
        hipLaunchKernelGGL(k_void_sizes, sgrid, block, 0, st, did, M, C, sizes);
        hipLaunchKernelGGL(k_void_keep, cgrid, block, 0, st, sizes, C, keep);
        MDH_TRY(exclusive_scan_u32(sc, keep, newid, (int64_t)C + 1));
        hipLaunchKernelGGL(k_void_point_keep, pgrid, block, 0, st, did, M, C, sizes, flag);
        MDH_TRY(exclusive_scan_u32(sc, flag, rank, M));
        hipLaunchKernelGGL(k_void_compact, pgrid, block, 0, st, dx, dy, dz, did, flag, rank, newid, M, dox, doy, doz, doid);
    }
    MDH_HIP(hipGetLastError());
    int voids = 0, kept = 0;
    MDH_HIP(hipMemcpyAsync(&voids, newid + C + 1, sizeof(int), hipMemcpyDeviceToHost, st));
    MDH_HIP(hipMemcpyAsync(&kept, rank + M, sizeof(int), hipMemcpyDeviceToHost, st));
    MDH_HIP(hipStreamSynchronize(st));
    *void_number_host = voids;
    *kept_host = kept;
    return sc.finish(space);
}
}

MDH_WARM_UNIT(voids)
