// wigner_seitz.hip — nearest reference SITE of every atom of a current frame, and the occupancy of the sites
//
// Replaces the Tree of src/fast_knn.cpp:924-972 (build_with_coords, query_nearest_batch: k = 1, self never skipped) and the
// numpy tail of src/mdapy/wigner_seitz_defect.py:117-121.  The candidate set and the distance arithmetic are the reference's,
// as in knn.hip (knn_geom.hpp): sites and queries wrapped the reference's way, images +-nimages per periodic axis,
// d = a - (q_wrapped - shift), d2 = dx*dx + dy*dy + dz*dz in f64.
//
// Contract:
//   * the site grid is the CALLER's: mdh_ws_build writes the cell-sorted sites (32-byte records: wrapped x, y, z and the original
//     site index) and the cell starts into buffers the caller owns and hands to every later query; no state lives in the library.
//     The grid's shape is a function of (N, box) alone (ws_geometry), recomputed by the query;
//   * EXACT ties in d2 go to the lowest site index (the reference's answer there depends on its tree's traversal order);
//   * a query with a non-finite coordinate (after the affine map), or a search among no sites, gets index -1: it is counted in no
//     site, its occupancy is 0 and its site type -1.
#include "common.hpp"
#include "grid.hpp"
#include "knn_geom.hpp"

namespace mdh {

// a site as the query reads it: two 16-byte requests per candidate (common.hpp Pos4, with the id in the unused slot)
struct __attribute__((aligned(16))) WsSite { double x, y, z; int id, pad; };
static_assert(sizeof(WsSite) == 32 && sizeof(WsSite) == sizeof(Pos4), "a site record is a Pos4");

struct WsMap { double m[9]; };

// one to two sites per cell: the 27 cells of the first pass hold ~40 candidates, and a site within one cell width of the query
// — any atom of a crystal that has not left its lattice — ends the search there
constexpr double WS_PER_CELL = 1.5;

// images, grid shape and ring limit of a search among N sites in box b: a function of (N, b) alone, so build and query agree
static void ws_geometry(const DBox &b, int64_t N, Grid &g, KnnGeom &kg)
{
    knn_images(b, N, kg);
    knn_size_grid(b, N, WS_PER_CELL, g, kg);
}

template <bool TRI>
__global__ __launch_bounds__(256) void k_ws_wrap_sites(const double *__restrict__ x, const double *__restrict__ y,
                                                       const double *__restrict__ z, int64_t N, DBox b, double *__restrict__ wx,
                                                       double *__restrict__ wy, double *__restrict__ wz)
{
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= N)
        return;
    double px = x[i], py = y[i], pz = z[i];
    knn_wrap_point<TRI>(b, px, py, pz);
    wx[i] = px; wy[i] = py; wz[i] = pz;
}

// the cell-sorted sites as records, and the cell starts, into the caller's buffers
__global__ __launch_bounds__(256) void k_ws_pack(const double *__restrict__ xs, const double *__restrict__ ys, const double *__restrict__ zs,
                                                 const int *__restrict__ order, const int *__restrict__ cell_start, int64_t N,
                                                 int64_t ncell, WsSite *__restrict__ sites, int *__restrict__ starts_out)
{
    const int64_t q = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (q < N) sites[q] = WsSite{xs[q], ys[q], zs[q], order[q], 0};
    if (q <= ncell) starts_out[q] = cell_start[q];
}

// One thread per query.  The best (d2, id) pair lives in registers; a candidate replaces it when it is nearer, or exactly as near
// with a lower site index — so the result does not depend on the order the cells are walked in.  First the 27 cells around the
// query's as nine contiguous z-runs (k_knn_near's walk), then Chebyshev rings of (cell, image) pairs until the stop test passes.
//
// The stop test.  After rings 0 .. R every unvisited (cell, image) differs from the query's cell by at least R + 1 cells along
// some axis d, so a whole slab of R cells of that axis — R * width_d >= R * wmin, widths being PERPENDICULAR widths — lies between
// the query and anything in it: best <= (R * wmin * (1 - 1e-9))^2 ends the search.  That needs the query to lie in the cell it was
// binned into and a site in the cell it is stored in, which holds along periodic axes (both are wrapped; a wrap that rounds onto
// the far face is off by one unit in the last place, the test gives away nine digits; the wrap of a query |q| away loses ~1e-16 |q|,
// so the contract is stated for queries within 1e4 box lengths of the box — mdapy_amd.h).  Along an OPEN axis cell_coords clamps: a
// query (or a site) outside the box is binned into the face cell, and can be arbitrarily far beyond it.  The test stays
// conservative: beyond an open face there are no cells, so an unvisited cell that differs along that axis lies INWARD of the
// query's face cell — the query's distance to the slab boundary it must cross only grows with its distance outside the box; and a
// site clamped into a face cell lies outward of that cell's inner boundary, farther from everything on the other side of it than
// the cell itself.  A clamped query and a clamped site of the same face share the cell index on that axis and are told apart by
// the other axes, or meet in ring 0.  What clamping costs is time, not correctness: a query far outside finds a poor best in its
// face cell and walks rings until R * wmin reaches it.
template <bool TRI, bool MAP>
__global__ __launch_bounds__(256) void k_ws_nearest(const WsSite *__restrict__ sites, const int *__restrict__ cell_start, DBox b, DBox bg,
                                                    Grid g, KnnGeom kg, const double *__restrict__ x, const double *__restrict__ y,
                                                    const double *__restrict__ z, int64_t Q, WsMap a, int *__restrict__ indices)
{
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= Q)
        return;
    double qx = x[i], qy = y[i], qz = z[i];
    if (MAP) { // src/mdapy/wigner_seitz_defect.py:98-108: (x m0k + y m1k) + z m2k, the origin not subtracted
        const double px = qx, py = qy, pz = qz;
        qx = px * a.m[0] + py * a.m[3] + pz * a.m[6];
        qy = px * a.m[1] + py * a.m[4] + pz * a.m[7];
        qz = px * a.m[2] + py * a.m[5] + pz * a.m[8];
    }
    if (!(isfinite(qx) && isfinite(qy) && isfinite(qz))) { // no position: no site
        indices[i] = -1;
        return;
    }
    knn_wrap_point<TRI>(b, qx, qy, qz);
    int c0, c1, c2;
    cell_coords<TRI>(bg, g, qx, qy, qz, c0, c1, c2);
    double best = __builtin_huge_val();
    int best_id = 0x7fffffff;
    // the sites at positions [sb, se) of the cell order, seen from the shifted query w; four records (eight 16-byte requests) in
    // flight.  A slot past the end reads the last site again: offering a candidate twice changes nothing.  A site without a
    // position (NaN) compares false both ways and is never taken.
    auto scan_range = [&](int sb, int se, double w0, double w1, double w2) {
        for (int q0 = sb; q0 < se; q0 += 4) {
            WsSite c[4];
#pragma unroll
            for (int u = 0; u < 4; ++u) c[u] = sites[min(q0 + u, se - 1)];
#pragma unroll
            for (int u = 0; u < 4; ++u) {
                const double dx = c[u].x - w0, dy = c[u].y - w1, dz = c[u].z - w2;
                const double d2 = dx * dx + dy * dy + dz * dz;
                if (d2 < best || (d2 == best && c[u].id < best_id)) { best = d2; best_id = c[u].id; }
            }
        }
    };
    for (int col9 = 0; col9 < 9; ++col9) { // nearest columns first
        const int da = (0x28161 >> (2 * col9) & 3) - 1, db = (0x22215 >> (2 * col9) & 3) - 1; // (0,0) (-1,0) (1,0) (0,-1) (0,1) (-1,-1) (-1,1) (1,-1) (1,1)
        int a0, m0, a1, m1;
        if (!knn_fold_cell(b, g, kg, 0, c0 + da, a0, m0) || !knn_fold_cell(b, g, kg, 1, c1 + db, a1, m1)) continue;
        const int64_t col = ((int64_t)a0 * g.nc[1] + a1) * g.nc[2];
        for (int e2 = c2 - 1; e2 <= c2 + 1;) {
            int a2, m2;
            if (!knn_fold_cell(b, g, kg, 2, e2, a2, m2)) { ++e2; continue; }
            int len = 1; // cells of this column with the same image number: one contiguous piece of the sorted records
            while (e2 + len <= c2 + 1 && a2 + len < g.nc[2]) ++len;
            double s0, s1, s2;
            knn_image_shift<TRI>(b, m0, m1, m2, s0, s1, s2);
            scan_range(cell_start[col + a2], cell_start[col + a2 + len], qx - s0, qy - s1, qz - s2);
            e2 += len;
        }
    }
    // rings 0 and 1 are done (the loop above visits every cell c +- 1 that exists); ring R + 1 while the stop test of ring R fails
    for (int R = 1; R < kg.rmax; ++R) {
        const double reach = (double)R * kg.wmin * (1.0 - 1e-9);
        if (best <= reach * reach)
            break;
        const int S = R + 1;
        for (int da = -S; da <= S; ++da) {
            int a0, m0;
            if (!knn_fold_cell(b, g, kg, 0, c0 + da, a0, m0)) continue;
            const int ada = da < 0 ? -da : da;
            for (int db = -S; db <= S; ++db) {
                int a1, m1;
                if (!knn_fold_cell(b, g, kg, 1, c1 + db, a1, m1)) continue;
                const int adb = db < 0 ? -db : db;
                const bool shell_ab = (ada == S) || (adb == S);
                for (int dc = -S; dc <= S; dc += shell_ab ? 1 : 2 * S) { // interior of the cube was done by earlier rings
                    int a2, m2;
                    if (!knn_fold_cell(b, g, kg, 2, c2 + dc, a2, m2)) continue;
                    double s0, s1, s2;
                    knn_image_shift<TRI>(b, m0, m1, m2, s0, s1, s2);
                    const int64_t cell = ((int64_t)a0 * g.nc[1] + a1) * g.nc[2] + a2;
                    scan_range(cell_start[cell], cell_start[cell + 1], qx - s0, qy - s1, qz - s2);
                }
            }
        }
    }
    indices[i] = best_id == 0x7fffffff ? -1 : best_id;
}

// site_occupancy[idx] += 1, one vector atomic per atom (the indices differ from lane to lane, so nothing is merged; several atoms
// on one site are rare).  A pass of its own rather than the tail of the query: the raw Tree query (the reference's interface) has
// no occupancy to write, and the pass reads four bytes per atom.
__global__ __launch_bounds__(256) void k_ws_count(const int *__restrict__ idx, int64_t Q, int64_t N, int *__restrict__ occ)
{
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= Q)
        return;
    const int j = idx[i];
    if ((unsigned)j < (unsigned)N) atomicAdd(&occ[j], 1);
}

__device__ __forceinline__ int wave_sum(int v)
{
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) v += __shfl_xor(v, d, 64);
    return v;
}

// thread i < Q: the occupancy and the type code of atom i's site (index -1: occupancy 0, type -1); thread i < N: site i's share
// of counts[0] = #(occ == 0) and counts[1] = sum max(occ - 1, 0), summed over the wave, one atomic per wave and count
__global__ __launch_bounds__(256) void k_ws_gather(const int *__restrict__ idx, int64_t Q, int64_t N, const int *__restrict__ occ,
                                                   const int *__restrict__ site_type, int *__restrict__ atom_occ,
                                                   int *__restrict__ atom_type, int *__restrict__ counts)
{
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i < Q) {
        const int j = idx[i];
        const bool ok = (unsigned)j < (unsigned)N;
        atom_occ[i] = ok ? occ[j] : 0;
        if (atom_type) atom_type[i] = ok ? site_type[j] : -1;
    }
    int vac = 0, extra = 0;
    if (i < N) {
        const int o = occ[i];
        vac = o == 0 ? 1 : 0;
        extra = o > 1 ? o - 1 : 0;
    }
    vac = wave_sum(vac);
    extra = wave_sum(extra);
    if ((threadIdx.x & 63) == 0) {
        if (vac) atomicAdd(&counts[0], vac);
        if (extra) atomicAdd(&counts[1], extra);
    }
}

static bool ws_count_ok(int64_t n, const char *who)
{
    if (n < 0 || n >= 2147483647LL) { set_error(std::string(who) + ": invalid number of atoms"); return false; }
    return true;
}

// the records are read in 16-byte requests: a device buffer is used where it lies and must be aligned for them (a host buffer is
// staged into scratch, which is)
static bool ws_records_ok(const double *records, int space, const char *who)
{
    if (space == MDH_DEVICE && (reinterpret_cast<uintptr_t>(records) & 15) != 0) {
        set_error(std::string(who) + ": site_records must be 16-byte aligned");
        return false;
    }
    return true;
}

} // namespace mdh

using namespace mdh;

extern "C" {

int mdh_ws_grid_cells(int64_t N, const double *box9, const double *origin3, const int *boundary3, int64_t *ncell)
{
    if (!ws_count_ok(N, "mdh_ws_grid_cells"))
        return MDH_ERR_ARG;
    DBox b;
    MDH_TRY(make_box(b, box9, origin3, boundary3));
    *ncell = 0;
    if (N == 0)
        return MDH_OK;
    Grid g;
    KnnGeom kg;
    ws_geometry(b, N, g, kg);
    *ncell = g.ncell;
    return MDH_OK;
}

int mdh_ws_build(const double *x, const double *y, const double *z, int64_t N, const double *box9, const double *origin3,
                 const int *boundary3, double *site_records, int *cell_start, int space, void *stream)
{
    if (!ws_count_ok(N, "mdh_ws_build") || !ws_records_ok(site_records, space, "mdh_ws_build"))
        return MDH_ERR_ARG;
    DBox b;
    MDH_TRY(make_box(b, box9, origin3, boundary3));
    if (N == 0)
        return MDH_OK;
    CellGrid cg;
    KnnGeom kg;
    ws_geometry(b, N, cg.g, kg);
    Scope sc(stream);
    hipStream_t st = sc.stream();
    const double *dx = sc.stage_in(x, (size_t)N, space), *dy = sc.stage_in(y, (size_t)N, space), *dz = sc.stage_in(z, (size_t)N, space);
    double *rec = sc.stage(site_records, (size_t)N * 4, space, false, true);
    int *starts = sc.stage(cell_start, (size_t)cg.g.ncell + 1, space, false, true);
    double *wx = sc.alloc_n<double>((size_t)N), *wy = sc.alloc_n<double>((size_t)N), *wz = sc.alloc_n<double>((size_t)N);
    if (sc.failed())
        return sc.error();
    ProfRange pr("ws_build", st);
    if (b.tri)
        hipLaunchKernelGGL(k_ws_wrap_sites<true>, dim3(grid_for(N, 256)), dim3(256), 0, st, dx, dy, dz, N, b, wx, wy, wz);
    else
        hipLaunchKernelGGL(k_ws_wrap_sites<false>, dim3(grid_for(N, 256)), dim3(256), 0, st, dx, dy, dz, N, b, wx, wy, wz);
    DBox bg = b;
    if (b.tri) bg.o[0] = bg.o[1] = bg.o[2] = 0.0; // the triclinic wrap is anchored at 0, not at the origin
    MDH_TRY(build_cell_grid(sc, wx, wy, wz, N, bg, GridRequest{}, cg));
    const int64_t threads = std::max<int64_t>(N, cg.g.ncell + 1);
    hipLaunchKernelGGL(k_ws_pack, dim3(grid_for(threads, 256)), dim3(256), 0, st, cg.xs, cg.ys, cg.zs, cg.order, cg.cell_start, N,
                       cg.g.ncell, reinterpret_cast<WsSite *>(rec), starts);
    MDH_HIP(hipGetLastError());
    return sc.finish(space);
}

int mdh_ws_query(const double *site_records, const int *cell_start, int64_t N, const double *box9, const double *origin3,
                 const int *boundary3, const double *qx, const double *qy, const double *qz, int64_t Q, const double *map9_host,
                 int *indices, int space, void *stream)
{
    if (!ws_count_ok(N, "mdh_ws_query") || !ws_count_ok(Q, "mdh_ws_query") || !ws_records_ok(site_records, space, "mdh_ws_query"))
        return MDH_ERR_ARG;
    DBox b;
    MDH_TRY(make_box(b, box9, origin3, boundary3));
    if (Q == 0)
        return MDH_OK;
    Scope sc(stream);
    hipStream_t st = sc.stream();
    int *di = sc.stage(indices, (size_t)Q, space, false, true);
    if (N == 0) { // no sites: every query gets -1
        if (sc.failed())
            return sc.error();
        MDH_HIP(hipMemsetAsync(di, 0xff, sizeof(int) * (size_t)Q, st));
        return sc.finish(space);
    }
    Grid g;
    KnnGeom kg;
    ws_geometry(b, N, g, kg);
    const double *dx = sc.stage_in(qx, (size_t)Q, space), *dy = sc.stage_in(qy, (size_t)Q, space), *dz = sc.stage_in(qz, (size_t)Q, space);
    const WsSite *sites = reinterpret_cast<const WsSite *>(sc.stage_in(site_records, (size_t)N * 4, space));
    const int *starts = sc.stage_in(cell_start, (size_t)g.ncell + 1, space);
    if (sc.failed())
        return sc.error();
    DBox bg = b;
    if (b.tri) bg.o[0] = bg.o[1] = bg.o[2] = 0.0;
    WsMap a{};
    if (map9_host)
        for (int k = 0; k < 9; ++k) a.m[k] = map9_host[k];
    ProfRange pr("ws_query", st);
    const dim3 grid(grid_for(Q, 256)), block(256);
#define MDH_WS_NEAREST(TRI, MAP) hipLaunchKernelGGL((k_ws_nearest<TRI, MAP>), grid, block, 0, st, sites, starts, b, bg, g, kg, dx, dy, dz, Q, a, di)
    if (b.tri) { if (map9_host) MDH_WS_NEAREST(true, true); else MDH_WS_NEAREST(true, false); }
    else { if (map9_host) MDH_WS_NEAREST(false, true); else MDH_WS_NEAREST(false, false); }
#undef MDH_WS_NEAREST
    MDH_HIP(hipGetLastError());
    return sc.finish(space);
}

int mdh_ws_occupancy(const int *indices, int64_t Q, int64_t N, const int *site_type, int *site_occupancy, int *atom_occupancy,
                     int *atom_site_type, int *counts2_host, int space, void *stream)
{
    if (!ws_count_ok(N, "mdh_ws_occupancy") || !ws_count_ok(Q, "mdh_ws_occupancy"))
        return MDH_ERR_ARG;
    if (N > 0 && Q > 0 && (site_type == nullptr) != (atom_site_type == nullptr)) { // (an array of no entries may have no address)
        set_error("mdh_ws_occupancy: site_type and atom_site_type go together");
        return MDH_ERR_ARG;
    }
    counts2_host[0] = counts2_host[1] = 0;
    if (N == 0 && Q == 0)
        return MDH_OK;
    Scope sc(stream);
    hipStream_t st = sc.stream();
    const int *di = Q ? sc.stage_in(indices, (size_t)Q, space) : nullptr;
    const int *dt = (site_type && N) ? sc.stage_in(site_type, (size_t)N, space) : nullptr;
    int *occ = N ? sc.stage(site_occupancy, (size_t)N, space, false, true) : nullptr;
    int *aocc = Q ? sc.stage(atom_occupancy, (size_t)Q, space, false, true) : nullptr;
    int *atype = (atom_site_type && Q) ? sc.stage(atom_site_type, (size_t)Q, space, false, true) : nullptr;
    int *counts = sc.alloc_n<int>(2);
    if (sc.failed())
        return sc.error();
    ProfRange pr("ws_occupancy", st);
    MDH_HIP(hipMemsetAsync(counts, 0, 2 * sizeof(int), st));
    if (N) MDH_HIP(hipMemsetAsync(occ, 0, sizeof(int) * (size_t)N, st));
    if (Q && N) hipLaunchKernelGGL(k_ws_count, dim3(grid_for(Q, 256)), dim3(256), 0, st, di, Q, N, occ);
    hipLaunchKernelGGL(k_ws_gather, dim3(grid_for(std::max(Q, N), 256)), dim3(256), 0, st, di, Q, N, occ, dt, aocc, atype, counts);
    MDH_HIP(hipGetLastError());
    // the two counts: the one small copy of the analysis
    MDH_HIP(hipMemcpyAsync(counts2_host, counts, 2 * sizeof(int), hipMemcpyDeviceToHost, st));
    MDH_HIP(hipStreamSynchronize(st));
    return sc.finish(space);
}
}

MDH_WARM_UNIT(wigner_seitz)
