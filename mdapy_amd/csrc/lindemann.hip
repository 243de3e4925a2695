// lindemann.hip — Lindemann index of a trajectory: the relative fluctuation of every pair distance, summed over pairs.
// Replaces _lindemann.compute_global (src/lindemann.cpp:20-74) and _lindemann.compute_all (:85-146).  DESIGN.md section 5g.
//
// The reference keeps two N x N tables (the running sums, or the Welford mean and variance, of every pair) and walks them once
// per frame.  Here a workgroup of 256 threads owns a 64 x 64 tile of pairs, a thread a 4 x 4 micro-tile of it, and the pair state
// stays in registers while the workgroup walks the frames: positions of the tile's 64 i and 64 j atoms go through LDS frame by
// frame (two buffers; the next frame's loads are issued before the current frame's arithmetic), and nothing N x N is stored
// unless the caller asks for the tables.
//
// Arithmetic: every per-pair operation is the reference's, in its order, in IEEE binary64 (no contraction; `/` and sqrt
// correctly rounded), so the tables carry the reference's bits and the tests `var > 0` / `delta > 0` fall the same way.  The
// SUMS of pair terms are taken in another — fixed — order than the reference's (in a thread, across 16 lanes, across j blocks,
// across segments), and a sum is divided once where the reference divides every term: results agree to a few ulps per level of
// that tree and are the same bits on every run.  No floating-point atomics.
#include <algorithm>

#include "common.hpp"

namespace mdh {

constexpr int LD_T = 64;       // tile edge (atoms)
constexpr int LD_M = 4;        // micro-tile edge: thread (ty, tx) owns atoms ty + 16 a of the i block and tx + 16 b of the j block
constexpr int LD_THREADS = 256;
constexpr int64_t LD_MAX_ATOMS = 1 << 20;
constexpr size_t LD_PARTIAL_CAP = (size_t)256 << 20; // bytes of segments x F x N row sums (mdh_lindemann_all)

// One frame of a tile in LDS: [i block / j block][x, y, z][atom].  A wave's read of the j atoms is 16 consecutive doubles, the
// same for each of its four ty rows (a broadcast): one pass over 32 banks; its read of the i atoms is 4 addresses.
typedef double LdStage[2][3][LD_T];

// Walks the frames of one tile: body(f, xi, yi, zi, xj, yj, zj) is called for f = 0 .. F-1 in order with the positions of the
// thread's 4 i atoms and 4 j atoms (0.0 for an atom past the end).  All 256 threads call it together.
template <class Body>
__device__ __forceinline__ void ld_walk_frames(const double *__restrict__ pos, int64_t F, int64_t N, int64_t i0, int64_t j0,
                                               LdStage *s, Body body)
{
    const int t = threadIdx.x, ty = t >> 4, tx = t & 15;
    // a block's 64 atoms of one frame are 192 consecutive doubles: thread t < 192 brings in one of each block's
    const int64_t n3 = N * 3, ei = i0 * 3 + t, ej = j0 * 3 + t;
    const bool loader = t < 3 * LD_T, hi = loader && ei < n3, hj = loader && ej < n3;
    const int c = t % 3, at = t / 3;
    double a = hi ? pos[ei] : 0.0, b = hj ? pos[ej] : 0.0;
    if (loader) { s[0][0][c][at] = a; s[0][1][c][at] = b; }
    __syncthreads();
    for (int64_t f = 0; f < F; ++f) {
        const int buf = (int)(f & 1);
        const bool more = f + 1 < F;
        if (more) {
            const double *next = pos + (f + 1) * n3;
            a = hi ? next[ei] : 0.0;
            b = hj ? next[ej] : 0.0;
        }
        double xi[LD_M], yi[LD_M], zi[LD_M], xj[LD_M], yj[LD_M], zj[LD_M];
#pragma unroll
        for (int k = 0; k < LD_M; ++k) {
            xi[k] = s[buf][0][0][ty + 16 * k]; yi[k] = s[buf][0][1][ty + 16 * k]; zi[k] = s[buf][0][2][ty + 16 * k];
            xj[k] = s[buf][1][0][tx + 16 * k]; yj[k] = s[buf][1][1][tx + 16 * k]; zj[k] = s[buf][1][2][tx + 16 * k];
        }
        body(f, xi, yi, zi, xj, yj, zj);
        if (more && loader) { s[buf ^ 1][0][c][at] = a; s[buf ^ 1][1][c][at] = b; }
        __syncthreads(); // every wave is done reading s[buf]; s[buf ^ 1] is complete
    }
}

// src/lindemann.cpp:42-45 / :107-110
__device__ __forceinline__ double ld_distance(double xi, double yi, double zi, double xj, double yj, double zj)
{
    const double dx = xi - xj, dy = yi - yj, dz = zi - zj;
    return sqrt(dx * dx + dy * dy + dz * dz);
}

// the sum of v over the 16 lanes that share a ty (every lane gets the same bits: the adds of a butterfly commute)
__device__ __forceinline__ double ld_sum16(double v)
{
#pragma unroll
    for (int d = 1; d <= 8; d <<= 1) v = v + __shfl_xor(v, d, 64);
    return v;
}

// ---------------------------------------------------------------------------------------------------------------------------
// compute_all: grid (i blocks, segments).  Workgroup (bi, seg) walks the j blocks of its segment in order; for each it walks
// the frames and adds the 64 row sums of the frame's pair terms into partial[seg][f][bi * 64 ...] — written by the first j
// block, read and written back by the later ones, by the same thread each time.
// ---------------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(LD_THREADS) void k_lindemann_all(const double *__restrict__ pos, int64_t F, int64_t N, int64_t nb,
                                                              int segments, double *__restrict__ partial,
                                                              double *__restrict__ pair_mean, double *__restrict__ pair_var)
{
    __shared__ LdStage s[2];
    const int t = threadIdx.x, ty = t >> 4, tx = t & 15;
    const int64_t bi = blockIdx.x, seg = blockIdx.y;
    const int64_t jb_first = seg * nb / segments, jb_end = (seg + 1) * nb / segments;
    const int64_t i0 = bi * LD_T;
    double *mine = partial + seg * F * N;
    for (int64_t jb = jb_first; jb < jb_end; ++jb) {
        const int64_t j0 = jb * LD_T;
        const bool first = jb == jb_first;
        unsigned counted = 0; // bit 4 a + b: pair (a, b) of the micro-tile is a pair of two different atoms
#pragma unroll
        for (int a = 0; a < LD_M; ++a)
#pragma unroll
            for (int b = 0; b < LD_M; ++b) {
                const int64_t i = i0 + ty + 16 * a, j = j0 + tx + 16 * b;
                if (i < N && j < N && i != j) counted |= 1u << (4 * a + b);
            }
        double mean[LD_M][LD_M], var[LD_M][LD_M];
#pragma unroll
        for (int a = 0; a < LD_M; ++a)
#pragma unroll
            for (int b = 0; b < LD_M; ++b) mean[a][b] = var[a][b] = 0.0;
        ld_walk_frames(pos, F, N, i0, j0, s,
                       [&](int64_t f, const double *xi, const double *yi, const double *zi, const double *xj, const double *yj,
                           const double *zj) {
                           const double frames = (double)(f + 1);
                           double row[LD_M];
#pragma unroll
                           for (int a = 0; a < LD_M; ++a) {
                               row[a] = 0.0;
#pragma unroll
                               for (int b = 0; b < LD_M; ++b) {
                                   const double r = ld_distance(xi[a], yi[a], zi[a], xj[b], yj[b], zj[b]);
                                   // Welford, :113-118
                                   const double delta = r - mean[a][b];
                                   mean[a][b] = mean[a][b] + delta / frames;
                                   var[a][b] = var[a][b] + delta * (r - mean[a][b]);
                                   // :133-134
                                   const bool on = ((counted >> (4 * a + b)) & 1u) && var[a][b] > 0.0;
                                   const double term = sqrt(var[a][b] / frames) / mean[a][b];
                                   row[a] = row[a] + (on ? term : 0.0);
                               }
                           }
#pragma unroll
                           for (int a = 0; a < LD_M; ++a) {
                               const double sum = ld_sum16(row[a]);
                               const int64_t i = i0 + ty + 16 * a;
                               if (tx == 0 && i < N) {
                                   double *p = mine + f * N + i;
                                   *p = first ? sum : *p + sum;
                               }
                           }
                       });
        if (pair_mean) { // the state after the last frame, :117-122 (the diagonal holds the zeros the reference never touches)
#pragma unroll
            for (int a = 0; a < LD_M; ++a)
#pragma unroll
                for (int b = 0; b < LD_M; ++b) {
                    const int64_t i = i0 + ty + 16 * a, j = j0 + tx + 16 * b;
                    if (i < N && j < N) {
                        pair_mean[i * N + j] = mean[a][b];
                        pair_var[i * N + j] = var[a][b];
                    }
                }
        }
    }
}

// One workgroup per frame: the segments' row sums added in index order, lindemann_atom[f, i] = sum / (N - 1) (:136 divides each
// term), lindemann_frame[f] = the sum over the atoms — thread t takes atoms t, t + 256, ... in order, then a binary tree over
// the 256 threads — / (N (N - 1)) (:143).
__global__ __launch_bounds__(LD_THREADS) void k_lindemann_rows(const double *__restrict__ partial, int64_t F, int64_t N,
                                                               int segments, double others, double pairs,
                                                               double *__restrict__ lindemann_frame,
                                                               double *__restrict__ lindemann_atom)
{
    __shared__ double tree[LD_THREADS];
    const int t = threadIdx.x;
    const int64_t f = blockIdx.x;
    double acc = 0.0;
    for (int64_t i = t; i < N; i += LD_THREADS) {
        double sum = partial[f * N + i];
        for (int sg = 1; sg < segments; ++sg) sum = sum + partial[((int64_t)sg * F + f) * N + i];
        lindemann_atom[f * N + i] = sum / others;
        acc = acc + sum;
    }
    tree[t] = acc;
    __syncthreads();
    for (int half = LD_THREADS / 2; half >= 1; half >>= 1) {
        if (t < half) tree[t] = tree[t] + tree[t + half];
        __syncthreads();
    }
    if (t == 0) lindemann_frame[f] = tree[0] / pairs;
}

// ---------------------------------------------------------------------------------------------------------------------------
// compute_global: one workgroup per tile (bi, bj >= bi), tiles numbered row by row.  S1 and S2 of the tile's pairs i < j in
// registers over all frames, then the pair terms, their sum to partial[tile].
// ---------------------------------------------------------------------------------------------------------------------------
__device__ __forceinline__ int64_t ld_row_start(int64_t bi, int64_t nb) { return bi * nb - bi * (bi - 1) / 2; }

__global__ __launch_bounds__(LD_THREADS) void k_lindemann_global(const double *__restrict__ pos, int64_t F, int64_t N, int64_t nb,
                                                                 double *__restrict__ partial, double *__restrict__ pair_sum,
                                                                 double *__restrict__ pair_sumsq)
{
    __shared__ LdStage s[2];
    __shared__ double waves[LD_THREADS / 64];
    const int t = threadIdx.x, ty = t >> 4, tx = t & 15;
    const int64_t tile = blockIdx.x;
    // row bi of the triangle starts at tile bi nb - bi (bi - 1) / 2: an estimate from the quadratic, then exact steps
    const double edge = 2.0 * (double)nb + 1.0;
    int64_t bi = (int64_t)((edge - sqrt(edge * edge - 8.0 * (double)tile)) * 0.5);
    bi = bi < 0 ? 0 : (bi > nb - 1 ? nb - 1 : bi);
    while (bi > 0 && ld_row_start(bi, nb) > tile) --bi;
    while (bi + 1 < nb && ld_row_start(bi + 1, nb) <= tile) ++bi;
    const int64_t bj = bi + (tile - ld_row_start(bi, nb));
    const int64_t i0 = bi * LD_T, j0 = bj * LD_T;
    double s1[LD_M][LD_M], s2[LD_M][LD_M];
#pragma unroll
    for (int a = 0; a < LD_M; ++a)
#pragma unroll
        for (int b = 0; b < LD_M; ++b) s1[a][b] = s2[a][b] = 0.0;
    ld_walk_frames(pos, F, N, i0, j0, s,
                   [&](int64_t, const double *xi, const double *yi, const double *zi, const double *xj, const double *yj,
                       const double *zj) {
#pragma unroll
                       for (int a = 0; a < LD_M; ++a)
#pragma unroll
                           for (int b = 0; b < LD_M; ++b) {
                               const double r = ld_distance(xi[a], yi[a], zi[a], xj[b], yj[b], zj[b]);
                               s1[a][b] = s1[a][b] + r;     // :47
                               s2[a][b] = s2[a][b] + r * r; // :48
                           }
                   });
    const double frames = (double)F;
    double sum = 0.0;
#pragma unroll
    for (int a = 0; a < LD_M; ++a)
#pragma unroll
        for (int b = 0; b < LD_M; ++b) {
            const int64_t i = i0 + ty + 16 * a, j = j0 + tx + 16 * b;
            if (i < j && j < N) {
                if (pair_sum) pair_sum[i * N + j] = s1[a][b];
                if (pair_sumsq) pair_sumsq[i * N + j] = s2[a][b];
                // :63-69
                const double sq_mean = s2[a][b] / frames;
                const double r_mean = s1[a][b] / frames;
                const double delta = sq_mean - r_mean * r_mean;
                if (delta > 0.0) sum = sum + sqrt(delta) / r_mean;
            }
        }
#pragma unroll
    for (int d = 1; d <= 32; d <<= 1) sum = sum + __shfl_xor(sum, d, 64);
    if ((t & 63) == 0) waves[t >> 6] = sum;
    __syncthreads();
    if (t == 0) partial[tile] = ((waves[0] + waves[1]) + waves[2]) + waves[3];
}

// the tiles' sums in a fixed order (thread t takes tiles t, t + 256, ...; a binary tree over the threads), / (N (N - 1) / 2) (:73)
__global__ __launch_bounds__(LD_THREADS) void k_lindemann_total(const double *__restrict__ partial, int64_t tiles, double pairs,
                                                                double *__restrict__ result)
{
    __shared__ double tree[LD_THREADS];
    const int t = threadIdx.x;
    double acc = 0.0;
    for (int64_t k = t; k < tiles; k += LD_THREADS) acc = acc + partial[k];
    tree[t] = acc;
    __syncthreads();
    for (int half = LD_THREADS / 2; half >= 1; half >>= 1) {
        if (t < half) tree[t] = tree[t] + tree[t + half];
        __syncthreads();
    }
    if (t == 0) *result = tree[0] / pairs;
}

static bool ld_args_ok(const double *pos, int64_t F, int64_t N, const char *who)
{
    if (pos == nullptr) { set_error(std::string(who) + ": pos is NULL"); return false; }
    if (F < 1) { set_error(std::string(who) + ": needs at least one frame"); return false; }
    if (N < 2) { set_error(std::string(who) + ": needs at least two atoms"); return false; }
    if (N > LD_MAX_ATOMS) { set_error(std::string(who) + ": more than 1 048 576 atoms"); return false; }
    if (F > (int64_t)1 << 30) { set_error(std::string(who) + ": too many frames"); return false; }
    return true;
}

// segments of compute_all: asked > 0 is taken as it is, 0 = enough workgroups for three to a CU on 256 CUs; never more than
// there are j blocks, and lowered until the row sums fit LD_PARTIAL_CAP.  (Forced counts of 16-32 measured 5-20 % faster
// than this choice at 4 000 and 16 000 atoms — profiles/lindemann.md; the rule has not been retuned yet.)
static int ld_segments(int asked, int64_t nb, int64_t F, int64_t N)
{
    int64_t sg = asked > 0 ? asked : (768 + nb - 1) / nb;
    sg = std::min(sg, nb);
    const size_t one = (size_t)F * (size_t)N * sizeof(double);
    while (sg > 1 && (size_t)sg * one > LD_PARTIAL_CAP) --sg;
    return (int)sg;
}

} // namespace mdh

using namespace mdh;

extern "C" {

int mdh_lindemann_global(const double *pos, int64_t F, int64_t N, double *pair_sum, double *pair_sumsq, double *result_host,
                         int space, void *stream)
{
    if (!ld_args_ok(pos, F, N, "mdh_lindemann_global"))
        return MDH_ERR_ARG;
    if (result_host == nullptr) { set_error("mdh_lindemann_global: result_host is NULL"); return MDH_ERR_ARG; }
    const int64_t nb = (N + LD_T - 1) / LD_T, tiles = nb * (nb + 1) / 2;
    Scope sc(stream);
    hipStream_t st = sc.stream();
    const double *dpos = sc.stage_in(pos, (size_t)F * (size_t)N * 3, space);
    // a host table goes up and comes back whole: only its upper triangle is written
    double *dsum = sc.stage(pair_sum, (size_t)N * (size_t)N, space, true, true);
    double *dsq = sc.stage(pair_sumsq, (size_t)N * (size_t)N, space, true, true);
    double *partial = sc.alloc_n<double>((size_t)tiles + 1);
    if (sc.failed() || !partial)
        return sc.error();
    double *result = partial + tiles;
    const double pairs = static_cast<double>(N * (N - 1)) / 2.0; // :58
    {
        ProfRange pr("lindemann_global", st);
        hipLaunchKernelGGL(k_lindemann_global, dim3((unsigned)tiles), dim3(LD_THREADS), 0, st, dpos, F, N, nb, partial, dsum, dsq);
        hipLaunchKernelGGL(k_lindemann_total, dim3(1), dim3(LD_THREADS), 0, st, partial, tiles, pairs, result);
    }
    MDH_HIP(hipGetLastError());
    MDH_HIP(hipMemcpyAsync(result_host, result, sizeof(double), hipMemcpyDeviceToHost, st));
    MDH_HIP(hipStreamSynchronize(st));
    return sc.finish(space);
}

int mdh_lindemann_all(const double *pos, int64_t F, int64_t N, double *pair_mean, double *pair_var, double *lindemann_frame,
                      double *lindemann_atom, int segments, int space, void *stream)
{
    if (!ld_args_ok(pos, F, N, "mdh_lindemann_all"))
        return MDH_ERR_ARG;
    if (lindemann_frame == nullptr || lindemann_atom == nullptr) {
        set_error("mdh_lindemann_all: lindemann_frame and lindemann_atom are required");
        return MDH_ERR_ARG;
    }
    if ((pair_mean == nullptr) != (pair_var == nullptr)) {
        set_error("mdh_lindemann_all: pair_mean and pair_var go together");
        return MDH_ERR_ARG;
    }
    if (segments < 0) { set_error("mdh_lindemann_all: segments is negative"); return MDH_ERR_ARG; }
    const int64_t nb = (N + LD_T - 1) / LD_T;
    const int sg = ld_segments(segments, nb, F, N);
    Scope sc(stream);
    hipStream_t st = sc.stream();
    const double *dpos = sc.stage_in(pos, (size_t)F * (size_t)N * 3, space);
    double *dmean = sc.stage(pair_mean, (size_t)N * (size_t)N, space, false, true);
    double *dvar = sc.stage(pair_var, (size_t)N * (size_t)N, space, false, true);
    double *dframe = sc.stage(lindemann_frame, (size_t)F, space, false, true);
    double *datom = sc.stage(lindemann_atom, (size_t)F * (size_t)N, space, false, true);
    double *partial = sc.alloc_n<double>((size_t)sg * (size_t)F * (size_t)N);
    if (sc.failed() || !partial)
        return sc.error();
    const double others = static_cast<double>(N - 1), pairs = static_cast<double>(N * (N - 1)); // :136, :100
    {
        ProfRange pr("lindemann_all", st);
        hipLaunchKernelGGL(k_lindemann_all, dim3((unsigned)nb, (unsigned)sg), dim3(LD_THREADS), 0, st, dpos, F, N, nb, sg, partial,
                           dmean, dvar);
        hipLaunchKernelGGL(k_lindemann_rows, dim3((unsigned)F), dim3(LD_THREADS), 0, st, partial, F, N, sg, others, pairs, dframe,
                           datom);
    }
    MDH_HIP(hipGetLastError());
    return sc.finish(space);
}
}

MDH_WARM_UNIT(lindemann)
