// rows.hip — the small row-wise helpers around a neighbor list on gfx950: the row sorts, wrap_positions, average_by_neighbor and the
// overlap filter, with their C entry points.  Replaces, of src/neighbor.cpp of the reference, sort_verlet_by_distance :745-775,
// wrap_positions :675-702, average_by_neighbor :704-743 and filter_overlap_atom :390-486.
//
// Data layout in HBM: x,y,z f64[N] (SoA, original atom order); verlet int32[N][M], dist f64[N][M], nn int32[N] —
// rows in ORIGINAL atom order.
#include "common.hpp"
#include "grid.hpp"

namespace mdh {

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

} // namespace mdh

using namespace mdh;

extern "C" {

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

MDH_WARM_UNIT(rows)
