// sample.hip — what consumes per-atom descriptors: farthest-point sampling and the two device halves of a PCA.
// Replaces fps_sample and PCA.fit_transform of the reference's potential_tool.py (:354-445), which are numpy.  DESIGN.md section 5p.
//
// Farthest-point sampling keeps, for every row of an (N, D) table, the smallest squared distance to the rows picked so far, and
// picks the row where that minimum is largest.  One pick is one pass over the table: 8 N D bytes in, 16 N bytes for the minima.
//
// The pinned sum.  The squared distance of a row a to the current point b is
//     acc = 0;  for k = 0 .. D-1:  acc = acc + (a_k - b_k) * (a_k - b_k)
// one accumulator, ascending k, IEEE binary64, no contraction (the library is built with -ffp-contract=off).  Every path below
// evaluates exactly this, whatever the launch shape or the way the features are cut into chunks, so the paths give the same bits.
// The arg-max takes the lowest row index among equal values — (value, index) pairs are totally ordered, so the order in which
// lanes, waves and workgroups are reduced cannot change the result.
//
// The table is row-major: a lane that walked its own row in memory would stride by 8 D bytes.  A wave's 64 rows are one
// contiguous piece of memory instead; it is brought into LDS with consecutive lanes on consecutive doubles, at most 32 features
// (one chunk) of every row at a time, each row padded to an odd number of doubles: lane r then reads [r * stride + k], and an odd
// stride puts the 32 lanes of a half-wave on 32 different pairs of banks.
//
// Grid path: one launch per pick.  A workgroup updates the minima of its rows, reduces (value, lowest index) over its two waves,
// stores its candidate and takes a ticket with one atomic; the workgroup that draws the last ticket reduces the candidates, stores
// the next pick and puts the ticket back to zero.  Nothing waits on another workgroup, and the launches of a call are queued on
// the stream without the host looking in between: a launch reads the current pick from where the previous one left it.
// One-workgroup path: for a small table, one launch of eight waves loops over all the picks with __syncthreads() only.
//
// PCA: column means, then the covariance of the centred table, both as per-workgroup partial sums (rows in index order) that are
// added in workgroup order — fixed orders, no floating-point atomics, the same bits on every run; then (X - mean) @ components.
#include <algorithm>
#include <climits>
#include <cmath>

#include "common.hpp"

namespace mdh {

constexpr int FPS_GRID_THREADS = 128;  // grid path: two waves to a workgroup, 128 rows to a tile
constexpr int FPS_BLOCK_THREADS = 512; // one-workgroup path: eight waves, 512 rows to a tile
constexpr int FPS_MAX_GRID = 2048;     // workgroups of a pass = candidates the last one reduces
constexpr int FPS_MAX_CHUNK = 32;      // features staged at a time
constexpr int FPS_BATCH = 16;          // loads a lane has in flight before it writes them to LDS
constexpr int FPS_LDS_BUDGET = 60 * 1024;
constexpr int FPS_LDS_MISC = 256;      // 16 doubles + 32 ints of reduction scratch
constexpr int64_t FPS_MAX_D = 1024;
constexpr int64_t FPS_MAX_N = (int64_t)INT_MAX - 1024;
constexpr int64_t FPS_BLOCK_MAX_D = 512;
// the one-workgroup path accepts tables up to this many entries (8 MiB: they stay in L2) ...
constexpr int64_t FPS_BLOCK_MAX_ELEMS = (int64_t)1 << 20;
// ... and is chosen up to this many.  Measured on an MI355X (tools/fps_bench.py, profiles/fps.md; 30 columns, 65 picks, time
// per pick with the call's fixed costs in both): 512 rows = 15 360 entries 8.8 us against the grid path's 10.7; 1 024 rows =
// 30 720 entries 15.2 against 11.2 — one workgroup's tiles wait for their loads one after the other (7 us more per 512 rows),
// a launch with its ticket costs about 10 us whatever the size.  The crossover lies between the two.
constexpr int64_t FPS_BLOCK_AUTO_ELEMS = 16384;

// How a wave's 64 rows go through LDS: nch chunks of kcw features (the last one may be shorter), rows `stride` doubles apart.
struct FpsPlan {
    int kcw, nch, stride;
    int off_misc, off_stage; // byte offsets into the dynamic LDS: [current row | misc | one stage per wave]
    int lds;                 // bytes in all
};

static FpsPlan fps_plan(int64_t D, int waves, bool with_row)
{
    FpsPlan p;
    const int row_bytes = with_row ? (int)((D * 8 + 15) / 16 * 16) : 0;
    int smax = (FPS_LDS_BUDGET - row_bytes - FPS_LDS_MISC) / (waves * 64 * 8);
    if ((smax & 1) == 0) --smax;
    const int kmax = std::min(FPS_MAX_CHUNK, smax);
    p.nch = (int)((D + kmax - 1) / kmax);
    p.kcw = (int)((D + p.nch - 1) / p.nch);
    p.stride = p.kcw | 1;
    p.off_misc = row_bytes;
    p.off_stage = row_bytes + FPS_LDS_MISC;
    p.lds = p.off_stage + waves * 64 * p.stride * 8;
    return p;
}

// Features [k0, k0 + kcw) of rows [r0, r0 + 64) into the wave's stage: element e = r * kcw + k of that piece is taken by lane
// e % 64 in round e / 64, so the lanes of a round read consecutive doubles of each row.  (r, k) of a lane advance by
// (64 / kcw, 64 % kcw) per round.  Rows past N and features past D read nothing and stage 0.  CENTRE: minus mean[feature].
template <bool CENTRE>
__device__ __forceinline__ void fps_stage(const double *__restrict__ x, int64_t N, int D, int64_t r0, int k0, const FpsPlan &p,
                                          double *__restrict__ st, const double *__restrict__ mean)
{
    const int lane = threadIdx.x & 63;
    const int qs = 64 / p.kcw, ms = 64 % p.kcw;
    int r = lane / p.kcw, k = lane % p.kcw;
    for (int it0 = 0; it0 < p.kcw; it0 += FPS_BATCH) {
        double v[FPS_BATCH];
        int o[FPS_BATCH];
#pragma unroll
        for (int j = 0; j < FPS_BATCH; ++j) {
            v[j] = 0.0;
            o[j] = -1;
            if (it0 + j < p.kcw) {
                const int64_t i = r0 + r;
                const int f = k0 + k;
                if (i < N && f < D) {
                    v[j] = x[i * D + f];
                    if (CENTRE) v[j] = v[j] - mean[f];
                }
                o[j] = r * p.stride + k;
                r += qs;
                k += ms;
                if (k >= p.kcw) { k -= p.kcw; ++r; }
            }
        }
#pragma unroll
        for (int j = 0; j < FPS_BATCH; ++j)
            if (o[j] >= 0) st[o[j]] = v[j];
    }
}

// The pinned sum of this lane's row (r0 + lane) against cur[0 .. D), all lanes of the workgroup together (two barriers per
// chunk).  FIRST: also says whether the row holds a value that is not finite.
template <bool FIRST>
__device__ __forceinline__ double fps_row_d2(const double *__restrict__ x, int64_t N, int D, int64_t r0, const FpsPlan &p,
                                             const double *cur, double *st, bool &bad)
{
    const int lane = threadIdx.x & 63;
    double acc = 0.0;
    for (int ch = 0; ch < p.nch; ++ch) {
        const int k0 = ch * p.kcw, kc = min(p.kcw, D - k0);
        fps_stage<false>(x, N, D, r0, k0, p, st, nullptr);
        __syncthreads();
        const double *mine = st + lane * p.stride;
        for (int k = 0; k < kc; ++k) {
            const double a = mine[k], d = a - cur[k0 + k];
            if (FIRST) bad = bad || !(fabs(a) <= 1.7976931348623157e308);
            acc = acc + d * d;
        }
        __syncthreads();
    }
    return acc;
}

struct FpsBest { double v; int i; };

__device__ __forceinline__ bool fps_better(double v2, int i2, const FpsBest &b) { return v2 > b.v || (v2 == b.v && i2 < b.i); }

__device__ __forceinline__ FpsBest fps_wave_best(FpsBest b)
{
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) {
        const double v2 = __shfl_xor(b.v, d, 64);
        const int i2 = __shfl_xor(b.i, d, 64);
        if (fps_better(v2, i2, b)) { b.v = v2; b.i = i2; }
    }
    return b;
}

// the workgroup's best in thread 0 (misc_v / misc_i: one slot per wave; a barrier inside, and the slots are free again after the
// caller's next barrier)
__device__ __forceinline__ FpsBest fps_block_best(FpsBest b, double *misc_v, int *misc_i)
{
    const int t = threadIdx.x, waves = blockDim.x >> 6;
    b = fps_wave_best(b);
    if ((t & 63) == 0) { misc_v[t >> 6] = b.v; misc_i[t >> 6] = b.i; }
    __syncthreads();
    if (t == 0)
        for (int w = 1; w < waves; ++w)
            if (fps_better(misc_v[w], misc_i[w], b)) { b.v = misc_v[w]; b.i = misc_i[w]; }
    return b;
}

// ctl: word 0 the ticket, word 1 "a value is not finite".  Also min_d2 = inf where no pass will write it (n_sample == 1).
__global__ __launch_bounds__(256) void k_fps_init(unsigned *ctl, int *picks, int start, double *min_d2, int64_t fill)
{
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i == 0) { ctl[0] = 0u; ctl[1] = 0u; ctl[2] = 0u; ctl[3] = 0u; picks[0] = start; }
    if (i < fill) min_d2[i] = INFINITY;
}

template <bool FIRST>
__global__ __launch_bounds__(FPS_GRID_THREADS) void k_fps_pass(const double *__restrict__ x, int64_t N, int D, FpsPlan p,
                                                               double *__restrict__ min_d2, double *cand_v, int *cand_i,
                                                               unsigned *ctl, int *picks, int64_t step)
{
    extern __shared__ __attribute__((aligned(16))) char smem[];
    double *cur = reinterpret_cast<double *>(smem);
    double *misc_v = reinterpret_cast<double *>(smem + p.off_misc);
    int *misc_i = reinterpret_cast<int *>(misc_v + 16);
    const int t = threadIdx.x, wave = t >> 6, lane = t & 63;
    double *st = reinterpret_cast<double *>(smem + p.off_stage) + wave * 64 * p.stride;

    int64_t c = picks[step]; // left there by the previous launch of this stream (k_fps_init for step 0)
    if (c < 0 || c >= N) c = 0;
    for (int k = t; k < D; k += FPS_GRID_THREADS) cur[k] = x[c * D + k];
    __syncthreads();

    FpsBest best{-1.0, INT_MAX};
    bool bad = false;
    const int64_t ntiles = (N + FPS_GRID_THREADS - 1) / FPS_GRID_THREADS;
    for (int64_t tile = blockIdx.x; tile < ntiles; tile += gridDim.x) { // (the same trips for both waves: barriers inside)
        const int64_t r0 = tile * FPS_GRID_THREADS + wave * 64, i = r0 + lane;
        const double d2 = fps_row_d2<FIRST>(x, N, D, r0, p, cur, st, bad);
        if (i < N) {
            double m = d2;
            if (!FIRST) { const double old = min_d2[i]; m = d2 < old ? d2 : old; }
            min_d2[i] = m;
            if (m > best.v) { best.v = m; best.i = (int)i; } // rows ascend: the first of equal values stays
        }
    }
    if (FIRST && bad) __hip_atomic_store(&ctl[1], 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);

    best = fps_block_best(best, misc_v, misc_i);
    if (t == 0) {
        __hip_atomic_store(&cand_v[blockIdx.x], best.v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        __hip_atomic_store(&cand_i[blockIdx.x], best.i, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        // publish, then the ticket: the release first, the wait after it, the atomic last
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "agent");
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        const unsigned ticket = __hip_atomic_fetch_add(&ctl[0], 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        misc_i[15] = ticket == gridDim.x - 1 ? 1 : 0;
    }
    __syncthreads();
    if (misc_i[15] == 0)
        return;
    // the last workgroup of this pass: every candidate has been published
    if (t == 0) {
        __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "agent");
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    }
    __syncthreads();
    FpsBest all{-1.0, INT_MAX};
    for (int b = t; b < (int)gridDim.x; b += FPS_GRID_THREADS) {
        const double v2 = __hip_atomic_load(&cand_v[b], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        const int i2 = __hip_atomic_load(&cand_i[b], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        if (fps_better(v2, i2, all)) { all.v = v2; all.i = i2; }
    }
    all = fps_block_best(all, misc_v, misc_i);
    if (t == 0) {
        picks[step + 1] = (all.i >= 0 && (int64_t)all.i < N) ? all.i : 0; // (only a table of NaNs leaves no candidate)
        __hip_atomic_store(&ctl[0], 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
}

__global__ __launch_bounds__(FPS_BLOCK_THREADS) void k_fps_block(const double *__restrict__ x, int64_t N, int D, FpsPlan p,
                                                                 double *__restrict__ min_d2, unsigned *ctl, int *picks,
                                                                 int64_t n_sample)
{
    extern __shared__ __attribute__((aligned(16))) char smem[];
    double *cur = reinterpret_cast<double *>(smem);
    double *misc_v = reinterpret_cast<double *>(smem + p.off_misc);
    int *misc_i = reinterpret_cast<int *>(misc_v + 16);
    const int t = threadIdx.x, wave = t >> 6, lane = t & 63;
    double *st = reinterpret_cast<double *>(smem + p.off_stage) + wave * 64 * p.stride;
    const int64_t ntiles = (N + FPS_BLOCK_THREADS - 1) / FPS_BLOCK_THREADS;

    if (t == 0) misc_i[15] = picks[0];
    __syncthreads();
    bool bad = false;
    for (int64_t s = 0; s + 1 < n_sample; ++s) {
        int64_t c = misc_i[15];
        if (c < 0 || c >= N) c = 0;
        for (int k = t; k < D; k += FPS_BLOCK_THREADS) cur[k] = x[c * D + k];
        __syncthreads();
        FpsBest best{-1.0, INT_MAX};
        for (int64_t tile = 0; tile < ntiles; ++tile) {
            const int64_t r0 = tile * FPS_BLOCK_THREADS + wave * 64, i = r0 + lane;
            const double d2 = s == 0 ? fps_row_d2<true>(x, N, D, r0, p, cur, st, bad) : fps_row_d2<false>(x, N, D, r0, p, cur, st, bad);
            if (i < N) {
                double m = d2;
                if (s > 0) { const double old = min_d2[i]; m = d2 < old ? d2 : old; } // (this thread's own store of the pass before)
                min_d2[i] = m;
                if (m > best.v) { best.v = m; best.i = (int)i; }
            }
        }
        best = fps_block_best(best, misc_v, misc_i);
        if (t == 0) {
            const int pick = (best.i >= 0 && (int64_t)best.i < N) ? best.i : 0;
            picks[s + 1] = pick;
            misc_i[15] = pick;
        }
        __syncthreads();
    }
    if (bad) __hip_atomic_store(&ctl[1], 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

// ---------------------------------------------------------------------------------------------------------------------------
// PCA
// ---------------------------------------------------------------------------------------------------------------------------
constexpr int PCA_THREADS = 256;
constexpr int PCA_ROWS = 32; // rows of a tile
constexpr int64_t PCA_MAX_D = 128;
constexpr int PCA_MAX_BLOCKS = 512;

// partial[b][c] = the sum of column c over the rows of workgroup b, in row order
__global__ __launch_bounds__(PCA_THREADS) void k_pca_colsum(const double *__restrict__ x, int64_t N, int D, int64_t rows_per_block,
                                                            double *__restrict__ partial)
{
    extern __shared__ __attribute__((aligned(16))) char smem[];
    double *tile = reinterpret_cast<double *>(smem);
    const int t = threadIdx.x;
    const int64_t b0 = (int64_t)blockIdx.x * rows_per_block, b1 = min(N, b0 + rows_per_block);
    double acc = 0.0;
    for (int64_t r0 = b0; r0 < b1; r0 += PCA_ROWS) {
        const int nr = (int)min((int64_t)PCA_ROWS, b1 - r0), n = nr * D;
        for (int e = t; e < n; e += PCA_THREADS) tile[e] = x[r0 * D + e];
        __syncthreads();
        if (t < D)
            for (int r = 0; r < nr; ++r) acc = acc + tile[r * D + t];
        __syncthreads();
    }
    if (t < D) partial[(int64_t)blockIdx.x * D + t] = acc;
}

// out[e] = (the sum over the workgroups, in index order, of partial[b][e]) / divisor
__global__ __launch_bounds__(PCA_THREADS) void k_pca_join(const double *__restrict__ partial, int blocks, int entries, double divisor,
                                                          double *__restrict__ out)
{
    const int e = blockIdx.x * PCA_THREADS + threadIdx.x;
    if (e >= entries)
        return;
    double acc = partial[e];
    for (int b = 1; b < blocks; ++b) acc = acc + partial[(int64_t)b * entries + e];
    out[e] = acc / divisor;
}

// partial[blk][a][b] = the sum over the rows of workgroup blk, in row order, of (x[a] - mean[a]) * (x[b] - mean[b]).  Thread
// (ty, tx) of 16 x 16 owns a = ty + 16 i, b = tx + 16 j, i, j < M: 16 M >= D columns.  [a][b] and [b][a] are the same products
// in the same order: the matrix is symmetric to the bit.
template <int M>
__global__ __launch_bounds__(PCA_THREADS) void k_pca_cov(const double *__restrict__ x, int64_t N, int D, int64_t rows_per_block,
                                                         const double *__restrict__ mean, double *__restrict__ partial)
{
    constexpr int DT = 16 * M;
    __shared__ double tile[PCA_ROWS * DT];
    __shared__ double smean[DT];
    const int t = threadIdx.x, ty = t >> 4, tx = t & 15;
    const int64_t b0 = (int64_t)blockIdx.x * rows_per_block, b1 = min(N, b0 + rows_per_block);
    for (int e = t; e < PCA_ROWS * DT; e += PCA_THREADS) tile[e] = 0.0; // the columns D .. DT stay 0
    if (t < DT) smean[t] = t < D ? mean[t] : 0.0;
    double acc[M][M];
#pragma unroll
    for (int i = 0; i < M; ++i)
#pragma unroll
        for (int j = 0; j < M; ++j) acc[i][j] = 0.0;
    __syncthreads();
    for (int64_t r0 = b0; r0 < b1; r0 += PCA_ROWS) {
        const int nr = (int)min((int64_t)PCA_ROWS, b1 - r0), n = nr * D;
        for (int e = t; e < n; e += PCA_THREADS) {
            const int r = e / D, c = e - r * D;
            tile[r * DT + c] = x[r0 * D + e] - smean[c];
        }
        __syncthreads();
        for (int r = 0; r < nr; ++r) {
            double xa[M], xb[M];
#pragma unroll
            for (int i = 0; i < M; ++i) { xa[i] = tile[r * DT + ty + 16 * i]; xb[i] = tile[r * DT + tx + 16 * i]; }
#pragma unroll
            for (int i = 0; i < M; ++i)
#pragma unroll
                for (int j = 0; j < M; ++j) acc[i][j] = acc[i][j] + xa[i] * xb[j];
        }
        __syncthreads();
    }
    double *mine = partial + (int64_t)blockIdx.x * D * D;
#pragma unroll
    for (int i = 0; i < M; ++i)
#pragma unroll
        for (int j = 0; j < M; ++j) {
            const int a = ty + 16 * i, b = tx + 16 * j;
            if (a < D && b < D) mine[a * D + b] = acc[i][j];
        }
}

// out[i][c] = the sum over k = 0 .. D-1, in order, of (x[i][k] - mean[k]) * comp[k][c]; eight components per walk over the row
constexpr int PCA_CG = 8;
__global__ __launch_bounds__(PCA_THREADS) void k_pca_project(const double *__restrict__ x, int64_t N, int D, FpsPlan p,
                                                             const double *__restrict__ mean, const double *__restrict__ comp, int C,
                                                             double *__restrict__ out)
{
    extern __shared__ __attribute__((aligned(16))) char smem[];
    const int t = threadIdx.x, wave = t >> 6, lane = t & 63;
    double *st = reinterpret_cast<double *>(smem + p.off_stage) + wave * 64 * p.stride;
    const int64_t r0 = (int64_t)blockIdx.x * PCA_THREADS + wave * 64, i = r0 + lane;
    for (int c0 = 0; c0 < C; c0 += PCA_CG) {
        double acc[PCA_CG];
#pragma unroll
        for (int j = 0; j < PCA_CG; ++j) acc[j] = 0.0;
        for (int ch = 0; ch < p.nch; ++ch) {
            const int k0 = ch * p.kcw, kc = min(p.kcw, D - k0);
            fps_stage<true>(x, N, D, r0, k0, p, st, mean);
            __syncthreads();
            const double *mine = st + lane * p.stride;
            for (int k = 0; k < kc; ++k) {
                const double a = mine[k];
                const double *row = comp + (int64_t)(k0 + k) * C + c0;
#pragma unroll
                for (int j = 0; j < PCA_CG; ++j)
                    if (c0 + j < C) acc[j] = acc[j] + a * row[j];
            }
            __syncthreads();
        }
        if (i < N) {
#pragma unroll
            for (int j = 0; j < PCA_CG; ++j)
                if (c0 + j < C) out[i * C + c0 + j] = acc[j];
        }
    }
}

static bool pca_args_ok(const char *who, const double *x, int64_t N, int64_t D, int64_t min_rows)
{
    if (x == nullptr) { set_error(std::string(who) + ": x is NULL"); return false; }
    if (N < min_rows) { set_error(std::string(who) + ": needs at least " + std::to_string(min_rows) + " rows"); return false; }
    if (N > FPS_MAX_N) { set_error(std::string(who) + ": too many rows"); return false; }
    if (D < 1 || D > PCA_MAX_D) { set_error(std::string(who) + ": the number of columns must be 1 .. 128"); return false; }
    return true;
}

} // namespace mdh

using namespace mdh;

extern "C" {

int mdh_fps_sample(const double *x, int64_t N, int64_t D, int64_t n_sample, int64_t start, int path, int *picks_host, double *min_d2,
                   int *path_host, int space, void *stream)
{
    if (x == nullptr || picks_host == nullptr) { set_error("mdh_fps_sample: x and picks_host are required"); return MDH_ERR_ARG; }
    if (N < 1 || N > FPS_MAX_N) { set_error("mdh_fps_sample: the number of rows must be 1 .. 2^31 - 1025"); return MDH_ERR_ARG; }
    if (D < 1 || D > FPS_MAX_D) { set_error("mdh_fps_sample: the number of columns must be 1 .. 1024"); return MDH_ERR_ARG; }
    if (n_sample < 1 || n_sample > N) { set_error("mdh_fps_sample: n_sample must be 1 .. N"); return MDH_ERR_ARG; }
    if (start < 0 || start >= N) { set_error("mdh_fps_sample: start is not a row"); return MDH_ERR_ARG; }
    if (path < 0 || path > 2) { set_error("mdh_fps_sample: path must be 0 (the library chooses), 1 (grid) or 2 (one workgroup)"); return MDH_ERR_ARG; }
    const bool block_ok = D <= FPS_BLOCK_MAX_D && N * D <= FPS_BLOCK_MAX_ELEMS;
    if (path == 2 && !block_ok) {
        set_error("mdh_fps_sample: the one-workgroup path takes at most 512 columns and 1 048 576 entries");
        return MDH_ERR_ARG;
    }
    const bool block = path == 2 || (path == 0 && D <= FPS_BLOCK_MAX_D && N * D <= FPS_BLOCK_AUTO_ELEMS);
    if (path_host) *path_host = block ? 2 : 1;

    Scope sc(stream);
    hipStream_t st = sc.stream();
    const double *dx = sc.stage_in(x, (size_t)N * (size_t)D, space);
    double *dmin = min_d2 ? sc.stage(min_d2, (size_t)N, space, false, true) : sc.alloc_n<double>((size_t)N);
    unsigned *ctl = sc.alloc_n<unsigned>(4);
    int *picks = sc.alloc_n<int>((size_t)n_sample);
    double *cand_v = sc.alloc_n<double>(FPS_MAX_GRID);
    int *cand_i = sc.alloc_n<int>(FPS_MAX_GRID);
    if (sc.failed() || !dx || !dmin || !ctl || !picks || !cand_v || !cand_i)
        return sc.error();
    {
        ProfRange pr("fps_sample", st);
        const int64_t fill = n_sample == 1 ? N : 0;
        hipLaunchKernelGGL(k_fps_init, dim3((unsigned)std::max<int64_t>(1, grid_for(fill, 256))), dim3(256), 0, st, ctl, picks, (int)start,
                           dmin, fill);
        if (n_sample > 1 && block) {
            const FpsPlan p = fps_plan(D, FPS_BLOCK_THREADS / 64, true);
            hipLaunchKernelGGL(k_fps_block, dim3(1), dim3(FPS_BLOCK_THREADS), (size_t)p.lds, st, dx, N, (int)D, p, dmin, ctl, picks,
                               n_sample);
        } else if (n_sample > 1) {
            const FpsPlan p = fps_plan(D, FPS_GRID_THREADS / 64, true);
            const int64_t ntiles = (N + FPS_GRID_THREADS - 1) / FPS_GRID_THREADS;
            const unsigned grid = (unsigned)std::min<int64_t>(ntiles, FPS_MAX_GRID);
            hipLaunchKernelGGL(k_fps_pass<true>, dim3(grid), dim3(FPS_GRID_THREADS), (size_t)p.lds, st, dx, N, (int)D, p, dmin, cand_v,
                               cand_i, ctl, picks, (int64_t)0);
            for (int64_t s = 1; s + 1 < n_sample; ++s)
                hipLaunchKernelGGL(k_fps_pass<false>, dim3(grid), dim3(FPS_GRID_THREADS), (size_t)p.lds, st, dx, N, (int)D, p, dmin,
                                   cand_v, cand_i, ctl, picks, s);
        }
    }
    MDH_HIP(hipGetLastError());
    unsigned flags[4] = {0u, 0u, 0u, 0u};
    MDH_HIP(hipMemcpyAsync(picks_host, picks, (size_t)n_sample * sizeof(int), hipMemcpyDeviceToHost, st));
    MDH_HIP(hipMemcpyAsync(flags, ctl, sizeof(flags), hipMemcpyDeviceToHost, st));
    MDH_HIP(hipStreamSynchronize(st));
    MDH_TRY(sc.finish(space));
    if (flags[1] != 0u) {
        set_error("mdh_fps_sample: the table holds a value that is not finite");
        return MDH_ERR_ARG;
    }
    return MDH_OK;
}

int mdh_pca_moments(const double *x, int64_t N, int64_t D, double *mean, double *cov, int space, void *stream)
{
    if (!pca_args_ok("mdh_pca_moments", x, N, D, 2))
        return MDH_ERR_ARG;
    if (mean == nullptr || cov == nullptr) { set_error("mdh_pca_moments: mean and cov are required"); return MDH_ERR_ARG; }
    const int M = D <= 32 ? 2 : (D <= 64 ? 4 : 8);
    const int64_t tiles = (N + PCA_ROWS - 1) / PCA_ROWS;
    const int64_t want = std::min<int64_t>(tiles, M == 8 ? PCA_MAX_BLOCKS / 2 : PCA_MAX_BLOCKS);
    const int64_t rows_per_block = (tiles + want - 1) / want * PCA_ROWS;
    const int blocks = (int)((N + rows_per_block - 1) / rows_per_block);
    const int DD = (int)(D * D);

    Scope sc(stream);
    hipStream_t st = sc.stream();
    const double *dx = sc.stage_in(x, (size_t)N * (size_t)D, space);
    double *dmean = sc.stage(mean, (size_t)D, space, false, true);
    double *dcov = sc.stage(cov, (size_t)DD, space, false, true);
    double *part_m = sc.alloc_n<double>((size_t)blocks * (size_t)D);
    double *part_c = sc.alloc_n<double>((size_t)blocks * (size_t)DD);
    if (sc.failed() || !dx || !dmean || !dcov || !part_m || !part_c)
        return sc.error();
    {
        ProfRange pr("pca_moments", st);
        hipLaunchKernelGGL(k_pca_colsum, dim3((unsigned)blocks), dim3(PCA_THREADS), (size_t)PCA_ROWS * (size_t)D * 8, st, dx, N, (int)D,
                           rows_per_block, part_m);
        hipLaunchKernelGGL(k_pca_join, dim3(1), dim3(PCA_THREADS), 0, st, part_m, blocks, (int)D, (double)N, dmean);
        if (M == 2)
            hipLaunchKernelGGL(k_pca_cov<2>, dim3((unsigned)blocks), dim3(PCA_THREADS), 0, st, dx, N, (int)D, rows_per_block, dmean, part_c);
        else if (M == 4)
            hipLaunchKernelGGL(k_pca_cov<4>, dim3((unsigned)blocks), dim3(PCA_THREADS), 0, st, dx, N, (int)D, rows_per_block, dmean, part_c);
        else
            hipLaunchKernelGGL(k_pca_cov<8>, dim3((unsigned)blocks), dim3(PCA_THREADS), 0, st, dx, N, (int)D, rows_per_block, dmean, part_c);
        hipLaunchKernelGGL(k_pca_join, dim3((unsigned)grid_for(DD, PCA_THREADS)), dim3(PCA_THREADS), 0, st, part_c, blocks, DD,
                           (double)(N - 1), dcov);
    }
    MDH_HIP(hipGetLastError());
    return sc.finish(space);
}

int mdh_pca_project(const double *x, int64_t N, int64_t D, const double *mean, const double *components, int64_t C, double *out,
                    int space, void *stream)
{
    if (!pca_args_ok("mdh_pca_project", x, N, D, 1))
        return MDH_ERR_ARG;
    if (mean == nullptr || components == nullptr || out == nullptr) {
        set_error("mdh_pca_project: mean, components and out are required");
        return MDH_ERR_ARG;
    }
    if (C < 1 || C > D) { set_error("mdh_pca_project: the number of components must be 1 .. D"); return MDH_ERR_ARG; }
    Scope sc(stream);
    hipStream_t st = sc.stream();
    const double *dx = sc.stage_in(x, (size_t)N * (size_t)D, space);
    const double *dmean = sc.stage_in(mean, (size_t)D, space);
    const double *dcomp = sc.stage_in(components, (size_t)D * (size_t)C, space);
    double *dout = sc.stage(out, (size_t)N * (size_t)C, space, false, true);
    if (sc.failed() || !dx || !dmean || !dcomp || !dout)
        return sc.error();
    {
        ProfRange pr("pca_project", st);
        const FpsPlan p = fps_plan(D, PCA_THREADS / 64, false);
        hipLaunchKernelGGL(k_pca_project, dim3((unsigned)grid_for(N, PCA_THREADS)), dim3(PCA_THREADS), (size_t)p.lds, st, dx, N, (int)D, p,
                           dmean, dcomp, (int)C, dout);
    }
    MDH_HIP(hipGetLastError());
    return sc.finish(space);
}
}

MDH_WARM_UNIT(sample)
