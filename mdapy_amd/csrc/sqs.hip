// sqs.hip — special quasirandom structures: cluster correlations of a lattice alloy and a Monte-Carlo search over many
// independent chains.  Replaces _sqs.SQSEngine's correlations / per_channel_delta / objective / run_mc (src/sqs.cpp:246-509).
// DESIGN.md section 5o.
//
// FORMULATION.  An instance is a cluster of n = 2..4 atoms; a GROUP is the set of instances of one (body order, shell); a
// CHANNEL is a group with a non-decreasing tuple of basis functions.  The reference keeps a floating sigma per (instance,
// channel) and adds and subtracts them (order-dependent sums that drift).  Here the state of a group is an INTEGER histogram:
//     h_g[k] = how many instances of g carry species multiset k      (multisets = non-decreasing tuples, lexicographic:
//                                                                     K = C(m + n - 1, n) of them for m species)
//     pi_c   = ( sum_k h_g[k] * tab_c[k] ) / n_inst_g
// tab_c[k] being the channel's basis product on multiset k averaged over the n! assignments (host-computed, _sqs.py).  A swap
// moves +-1 between bins: integer, commutative, undone exactly.  Everything floating is recomputed from the integers in a pinned
// order, so it can be restated in numpy bit for bit (tests/_sqs_ref.py):
//   tab     products left to right, assignments in lexicographic order, summed sequentially, one division (host)
//   pi_c    acc = 0.0; for k ascending: acc = acc + (double)h[k] * tab[k]; pi = acc / (double)n_inst   — no contraction
//   dc_c    fabs(pi_c - target_c)
//   objective, channels in channel order, the passes of src/sqs.cpp:281-341:
//     mode 0: obj = 0; obj = obj + w_abs[c] * dc[c]
//     mode 1: md[p] = maxdist0[p] (host: the body's largest diameter + d_min); for c: if (dc[c] > atat_tol && diam[c] < md[p_c])
//             md[p_c] = diam[c]; d1 = md[0]; for p >= 1: if (!(md[p] < md[p-1])) md[p] = md[p-1]; if (md[p] < d1) d1 = md[p];
//             for c with diam[c] >= d1 - 1e-12: dev = dev + dc[c] * w[c], den = den + w[c]  (w = shell weight * pow(w_npts, n-2),
//             one host-computed number); obj = den > 0 ? dev / den : 0; for p: obj = obj - (reward[p] * md[p]) / d_min
//             (reward[p] = w_dist * pow(w_npts, p), host)
//   Metropolis: delta = new - current; accept if delta <= 0 || u < exp(-delta / T); best is replaced when new < best, strictly.
//
// RANDOM NUMBERS are the library's own (the reference's std::mt19937_64 + libstdc++ distributions are not portable): integer,
// counter-based, every draw a pure function of (seed, replica, purpose, counter):
//     mix(z): z ^= z >> 30; z *= 0xBF58476D1CE4E5B9; z ^= z >> 27; z *= 0x94D049BB133111EB; z ^= z >> 31      (mod 2^64)
//     key  = mix(mix(seed + G) + ((replica << 2) | purpose) * G),  G = 0x9E3779B97F4A7C15
//     x    = mix(key + (counter + 1) * G);   index in [0, n) = ((x >> 32) * n) >> 32;   u = (x >> 11) * 2^-53
//   purpose 0: the initial Fisher-Yates shuffle, for p = N-1 down to 1: q = index(x(counter p), p + 1), swap types[p], types[q]
//   purposes 1, 2, 3 with counter = step: atom i, atom j, u.  A step with i == j or equal species does nothing.
// So a run may be cut into launches anywhere: the state (types, histograms, dc, objectives, best) waits in HBM, no bit changes.
//
// ONE WAVEFRONT = ONE REPLICA (a workgroup of 64).  Types, best types, histograms, dc live in LDS (16 C + 4 H + 2 N bytes and a
// little: a few KiB, many replicas to a CU); the instance tables and tab are read-only and shared by all replicas (L2).  Per step
// the lanes walk the instances of i and those of j that do not hold i, move -1 / +1 with integer LDS atomics, recompute the
// channels of the touched groups one channel per lane, and every lane forms the objective in the pinned order.  A rejected move
// applies the inverse updates.  No floating-point atomics.
//
// LIMITS (MDH_ERR_ARG before any device work): 2 <= N <= 4096, 2 <= m <= 8, bodies 2..4, R >= 1, T > 0, G <= 1024 groups,
// 16 C + 4 H + 4 ceil(G / 32) + 2 (N rounded up to 8) <= 65536 bytes of LDS per replica, tables in host memory (space = MDH_HOST:
// every index in them is checked on the host before a kernel sees it).  With 7 or 8 species and quadruplets the channel
// recomputation is hundreds of channels times hundreds of multisets per step: accepted, not optimised.
#include <vector>

#include "common.hpp"

#pragma clang fp contract(off)

namespace mdh {

constexpr int SQS_MAX_ATOMS = 4096;
constexpr int SQS_MAX_GROUPS = 1024;
constexpr int SQS_LDS_CAP = 65536;
// steps per launch when the caller leaves the choice to the library.  Measured on an MI355X (profiles/sqs.md): a step takes 7 us
// in a 256-atom ternary cell with pairs and triplets and 32 us in a 108-atom quinary cell with quadruplets, so a launch takes
// 26-44 ms and 130-193 ms there with 1 to 4096 replicas — well under a second
constexpr int64_t SQS_LAUNCH_STEPS = 4096;
constexpr uint64_t SQS_G = 0x9E3779B97F4A7C15ULL;

struct SqsModel {
    const int *inst_atoms;  // (I, 4), unused slots -1
    const int *inst_group;  // (I)
    const int *a2i_off;     // (N + 1)
    const int *a2i;         // (a2i_off[N]) instances of an atom, each once
    const int *group_i;     // (G, 6): n_pts, hist_off, chan_first, chan_count, n_inst, K
    const int *chan_i;      // (C, 3): group, n_pts - 2, tab_off
    const double *chan_d;   // (C, 4): target, diameter, w_abs, w_atat
    const double *tab;
    const int *msidx;       // ordered species tuple, base m -> multiset index; sections for n = 2, 3, 4
    int N, m, I, G, C, H;
    int ms_off[5];
    int mode, n_body;
    double tol, d_min, maxdist0[3], reward[3];
};

struct SqsLds {
    double *dc, *bak;
    int *hist;
    unsigned *gmask;
    unsigned char *types, *best;
};

__host__ __device__ inline int sqs_npad(int N) { return (N + 7) & ~7; }
__host__ __device__ inline size_t sqs_lds_bytes(int N, int G, int C, int H)
{
    return (size_t)16 * C + (size_t)4 * H + (size_t)4 * ((G + 31) / 32) + (size_t)2 * sqs_npad(N);
}

__device__ __forceinline__ SqsLds sqs_carve(const SqsModel &M, unsigned char *raw)
{
    SqsLds L;
    L.dc = reinterpret_cast<double *>(raw);
    L.bak = L.dc + M.C;
    L.hist = reinterpret_cast<int *>(L.bak + M.C);
    L.gmask = reinterpret_cast<unsigned *>(L.hist + M.H);
    L.types = reinterpret_cast<unsigned char *>(L.gmask + (M.G + 31) / 32);
    L.best = L.types + sqs_npad(M.N);
    return L;
}

__host__ __device__ inline uint64_t sqs_mix(uint64_t z)
{
    z ^= z >> 30; z *= 0xBF58476D1CE4E5B9ULL;
    z ^= z >> 27; z *= 0x94D049BB133111EBULL;
    z ^= z >> 31;
    return z;
}
__host__ __device__ inline uint64_t sqs_key(uint64_t seed, uint64_t replica, uint64_t purpose)
{
    return sqs_mix(sqs_mix(seed + SQS_G) + ((replica << 2) | purpose) * SQS_G);
}
__host__ __device__ inline uint64_t sqs_draw(uint64_t key, uint64_t counter) { return sqs_mix(key + (counter + 1) * SQS_G); }
__host__ __device__ inline int sqs_index(uint64_t x, int n) { return (int)(((x >> 32) * (uint64_t)n) >> 32); }

// multiset bin (in the group's histogram) of an instance whose atoms carry s0..s3
__device__ __forceinline__ int sqs_bin(const SqsModel &M, int n, int s0, int s1, int s2, int s3)
{
    int key = s0 * M.m + s1;
    if (n > 2) key = key * M.m + s2;
    if (n > 3) key = key * M.m + s3;
    return M.msidx[M.ms_off[n] + key];
}

// the histograms of L.types from nothing
__device__ void sqs_count_hist(const SqsModel &M, const SqsLds &L)
{
    const int lane = threadIdx.x;
    for (int k = lane; k < M.H; k += 64) L.hist[k] = 0;
    __syncthreads();
    for (int e = lane; e < M.I; e += 64) {
        const int4 a = *reinterpret_cast<const int4 *>(M.inst_atoms + 4 * e);
        const int *g = M.group_i + 6 * M.inst_group[e];
        const int n = g[0];
        const int b = sqs_bin(M, n, L.types[a.x], L.types[a.y], n > 2 ? L.types[a.z] : 0, n > 3 ? L.types[a.w] : 0);
        atomicAdd(&L.hist[g[1] + b], 1);
    }
    __syncthreads();
}

__device__ __forceinline__ double sqs_pi(const SqsModel &M, const SqsLds &L, int c)
{
    const int *g = M.group_i + 6 * M.chan_i[3 * c];
    const int *h = L.hist + g[1];
    const double *t = M.tab + M.chan_i[3 * c + 2];
    const int K = g[5];
    double acc = 0.0;
    for (int k = 0; k < K; ++k) acc = acc + (double)h[k] * t[k];
    return acc / (double)g[4];
}

// dc of every channel (and the correlations themselves where somebody wants them)
__device__ void sqs_all_channels(const SqsModel &M, const SqsLds &L, double *__restrict__ corr_out, double *__restrict__ delta_out)
{
    for (int c = threadIdx.x; c < M.C; c += 64) {
        const double pi = sqs_pi(M, L, c);
        const double d = fabs(pi - M.chan_d[4 * c]);
        L.dc[c] = d;
        if (corr_out) corr_out[c] = pi;
        if (delta_out) delta_out[c] = d;
    }
    __syncthreads();
}

// every lane computes the same number from the same LDS words
__device__ double sqs_objective(const SqsModel &M, const double *dc)
{
    const int C = M.C;
    if (M.mode == 0) {
        double obj = 0.0;
        for (int c = 0; c < C; ++c) obj = obj + M.chan_d[4 * c + 2] * dc[c];
        return obj;
    }
    double md0 = M.maxdist0[0], md1 = M.maxdist0[1], md2 = M.maxdist0[2];
    for (int c = 0; c < C; ++c) {
        const int p = M.chan_i[3 * c + 1];
        const double d = M.chan_d[4 * c + 1];
        if (dc[c] > M.tol) {
            if (p == 0) { if (d < md0) md0 = d; }
            else if (p == 1) { if (d < md1) md1 = d; }
            else { if (d < md2) md2 = d; }
        }
    }
    double d1 = md0;
    if (M.n_body > 1) {
        if (!(md1 < md0)) md1 = md0;
        if (md1 < d1) d1 = md1;
    }
    if (M.n_body > 2) {
        if (!(md2 < md1)) md2 = md1;
        if (md2 < d1) d1 = md2;
    }
    const double thr = d1 - 1e-12;
    double dev = 0.0, den = 0.0;
    for (int c = 0; c < C; ++c) {
        if (M.chan_d[4 * c + 1] >= thr) {
            const double w = M.chan_d[4 * c + 3];
            dev = dev + dc[c] * w;
            den = den + w;
        }
    }
    double obj = den > 0.0 ? dev / den : 0.0;
    obj = obj - (M.reward[0] * md0) / M.d_min;
    if (M.n_body > 1) obj = obj - (M.reward[1] * md1) / M.d_min;
    if (M.n_body > 2) obj = obj - (M.reward[2] * md2) / M.d_min;
    return obj;
}

// the swap of atoms i (species ti) and j (species tj), L.types still unswapped: sign +1 moves every touched instance from its
// bin before the swap to its bin after it, sign -1 moves it back.  Instances of i, then those of j that do not hold i.
__device__ __forceinline__ void sqs_move(const SqsModel &M, const SqsLds &L, int i, int j, int ti, int tj, int sign)
{
    const int oi = M.a2i_off[i], ni = M.a2i_off[i + 1] - oi, oj = M.a2i_off[j], nj = M.a2i_off[j + 1] - oj;
    for (int e = threadIdx.x; e < ni + nj; e += 64) {
        const int inst = e < ni ? M.a2i[oi + e] : M.a2i[oj + e - ni];
        const int4 a = *reinterpret_cast<const int4 *>(M.inst_atoms + 4 * inst);
        if (e >= ni && (a.x == i || a.y == i || a.z == i || a.w == i)) continue; // counted among i's
        const int gi = M.inst_group[inst];
        const int *g = M.group_i + 6 * gi;
        const int n = g[0];
        const int az = n > 2 ? a.z : a.x, aw = n > 3 ? a.w : a.x;
        const int s0 = L.types[a.x], s1 = L.types[a.y], s2 = L.types[az], s3 = L.types[aw];
        const int r0 = a.x == i ? tj : (a.x == j ? ti : s0), r1 = a.y == i ? tj : (a.y == j ? ti : s1);
        const int r2 = az == i ? tj : (az == j ? ti : s2), r3 = aw == i ? tj : (aw == j ? ti : s3);
        const int before = sqs_bin(M, n, s0, s1, s2, s3), after = sqs_bin(M, n, r0, r1, r2, r3);
        if (before != after) {
            atomicAdd(&L.hist[g[1] + before], -sign);
            atomicAdd(&L.hist[g[1] + after], sign);
            atomicOr(&L.gmask[gi >> 5], 1u << (gi & 31));
        }
    }
}

// ---------------------------------------------------------------------------------------------------------------------------
// mdh_sqs_count: one wavefront per type vector
// ---------------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(64) void k_sqs_count(SqsModel M, const int *__restrict__ types, int *__restrict__ hist_out,
                                                  double *__restrict__ corr_out, double *__restrict__ delta_out,
                                                  double *__restrict__ obj_out)
{
    extern __shared__ __attribute__((aligned(16))) unsigned char sqs_raw[];
    const SqsLds L = sqs_carve(M, sqs_raw);
    const int64_t r = blockIdx.x;
    for (int a = threadIdx.x; a < M.N; a += 64) L.types[a] = (unsigned char)types[r * M.N + a];
    __syncthreads();
    sqs_count_hist(M, L);
    if (hist_out)
        for (int k = threadIdx.x; k < M.H; k += 64) hist_out[r * M.H + k] = L.hist[k];
    sqs_all_channels(M, L, corr_out ? corr_out + r * M.C : nullptr, delta_out ? delta_out + r * M.C : nullptr);
    const double obj = sqs_objective(M, L.dc);
    if (obj_out && threadIdx.x == 0) obj_out[r] = obj;
}

// ---------------------------------------------------------------------------------------------------------------------------
// mdh_sqs_run.  The chain state in HBM: types, best (R, N) u8; hist (R, H) i32; dc (R, C) f64; obj (R, 2) f64 = current, best.
// ---------------------------------------------------------------------------------------------------------------------------
struct SqsState {
    unsigned char *types, *best;
    int *hist;
    double *dc, *obj;
};

__global__ __launch_bounds__(64) void k_sqs_init(SqsModel M, SqsState S, const int *__restrict__ types0, uint64_t seed, int shuffle)
{
    extern __shared__ __attribute__((aligned(16))) unsigned char sqs_raw[];
    const SqsLds L = sqs_carve(M, sqs_raw);
    const int64_t r = blockIdx.x;
    const int lane = threadIdx.x;
    for (int a = lane; a < M.N; a += 64) L.types[a] = (unsigned char)types0[a];
    __syncthreads();
    if (shuffle && lane == 0) {
        const uint64_t key = sqs_key(seed, (uint64_t)r, 0);
        for (int p = M.N - 1; p >= 1; --p) {
            const int q = sqs_index(sqs_draw(key, (uint64_t)p), p + 1);
            const unsigned char t = L.types[p];
            L.types[p] = L.types[q];
            L.types[q] = t;
        }
    }
    __syncthreads();
    sqs_count_hist(M, L);
    sqs_all_channels(M, L, nullptr, nullptr);
    const double obj = sqs_objective(M, L.dc);
    for (int a = lane; a < M.N; a += 64) {
        S.types[r * M.N + a] = L.types[a];
        S.best[r * M.N + a] = L.types[a];
    }
    for (int k = lane; k < M.H; k += 64) S.hist[r * M.H + k] = L.hist[k];
    for (int c = lane; c < M.C; c += 64) S.dc[r * M.C + c] = L.dc[c];
    if (lane == 0) { S.obj[2 * r] = obj; S.obj[2 * r + 1] = obj; }
}

__global__ __launch_bounds__(64) void k_sqs_steps(SqsModel M, SqsState S, uint64_t seed, int64_t step0, int64_t nsteps, double T)
{
    extern __shared__ __attribute__((aligned(16))) unsigned char sqs_raw[];
    const SqsLds L = sqs_carve(M, sqs_raw);
    const int64_t r = blockIdx.x;
    const int lane = threadIdx.x;
    const int GW = (M.G + 31) / 32;
    for (int a = lane; a < M.N; a += 64) {
        L.types[a] = S.types[r * M.N + a];
        L.best[a] = S.best[r * M.N + a];
    }
    for (int k = lane; k < M.H; k += 64) L.hist[k] = S.hist[r * M.H + k];
    for (int c = lane; c < M.C; c += 64) L.dc[c] = S.dc[r * M.C + c];
    for (int w = lane; w < GW; w += 64) L.gmask[w] = 0u;
    double cur = S.obj[2 * r], best = S.obj[2 * r + 1];
    __syncthreads();
    const uint64_t ki = sqs_key(seed, (uint64_t)r, 1), kj = sqs_key(seed, (uint64_t)r, 2), ku = sqs_key(seed, (uint64_t)r, 3);
    for (int64_t s = step0; s < step0 + nsteps; ++s) {
        const int i = sqs_index(sqs_draw(ki, (uint64_t)s), M.N), j = sqs_index(sqs_draw(kj, (uint64_t)s), M.N);
        const int ti = L.types[i], tj = L.types[j];
        if (i == j || ti == tj) continue; // (the same for every lane)
        sqs_move(M, L, i, j, ti, tj, 1);
        __syncthreads();
        for (int c = lane; c < M.C; c += 64) {
            const int g = M.chan_i[3 * c];
            if ((L.gmask[g >> 5] >> (g & 31)) & 1u) {
                L.bak[c] = L.dc[c];
                L.dc[c] = fabs(sqs_pi(M, L, c) - M.chan_d[4 * c]);
            }
        }
        __syncthreads();
        const double now = sqs_objective(M, L.dc);
        const double delta = now - cur;
        const double u = (double)(sqs_draw(ku, (uint64_t)s) >> 11) * 0x1p-53;
        const bool accept = delta <= 0.0 || u < exp(-delta / T);
        if (accept) {
            cur = now;
            if (lane == 0) { L.types[i] = (unsigned char)tj; L.types[j] = (unsigned char)ti; }
            __syncthreads();
            if (now < best) {
                best = now;
                for (int a = lane; a < M.N; a += 64) L.best[a] = L.types[a];
            }
        } else {
            sqs_move(M, L, i, j, ti, tj, -1);
            for (int c = lane; c < M.C; c += 64) {
                const int g = M.chan_i[3 * c];
                if ((L.gmask[g >> 5] >> (g & 31)) & 1u) L.dc[c] = L.bak[c];
            }
        }
        __syncthreads();
        for (int w = lane; w < GW; w += 64) L.gmask[w] = 0u;
        __syncthreads();
    }
    for (int a = lane; a < M.N; a += 64) {
        S.types[r * M.N + a] = L.types[a];
        S.best[r * M.N + a] = L.best[a];
    }
    for (int k = lane; k < M.H; k += 64) S.hist[r * M.H + k] = L.hist[k];
    for (int c = lane; c < M.C; c += 64) S.dc[r * M.C + c] = L.dc[c];
    if (lane == 0) { S.obj[2 * r] = cur; S.obj[2 * r + 1] = best; }
}

// the winner — the lowest best objective, the lowest replica on a tie (the reference's ascending `<` scan, src/sqs.cpp:498-501) —
// its types, and its correlations counted from them
__global__ __launch_bounds__(64) void k_sqs_pick(SqsModel M, SqsState S, int64_t R, int *__restrict__ winner_out,
                                                 int *__restrict__ types_out, double *__restrict__ corr_out,
                                                 double *__restrict__ objectives_out)
{
    extern __shared__ __attribute__((aligned(16))) unsigned char sqs_raw[];
    const SqsLds L = sqs_carve(M, sqs_raw);
    const int lane = threadIdx.x;
    double v = 0.0;
    int64_t at = -1;
    for (int64_t r = lane; r < R; r += 64) {
        const double o = S.obj[2 * r + 1];
        objectives_out[r] = o;
        if (at < 0 || o < v) { v = o; at = r; }
    }
#pragma unroll
    for (int d = 1; d <= 32; d <<= 1) {
        const double ov = __shfl_xor(v, d, 64);
        const int64_t oat = (int64_t)__shfl_xor((long long)at, d, 64);
        if (oat >= 0 && (at < 0 || ov < v || (ov == v && oat < at))) { v = ov; at = oat; }
    }
    for (int a = lane; a < M.N; a += 64) {
        const unsigned char t = S.best[at * M.N + a];
        L.types[a] = t;
        types_out[a] = t;
    }
    __syncthreads();
    sqs_count_hist(M, L);
    sqs_all_channels(M, L, corr_out, nullptr);
    if (lane == 0) winner_out[0] = (int)at;
}

// ---------------------------------------------------------------------------------------------------------------------------
// host: every index of the tables is checked here, before a kernel dereferences it
// ---------------------------------------------------------------------------------------------------------------------------
static int sqs_bad(const std::string &who, const std::string &what)
{
    set_error(who + ": " + what);
    return MDH_ERR_ARG;
}

static int64_t sqs_multisets(int m, int n)
{
    int64_t k = 1;
    for (int q = 1; q <= n; ++q) k = k * (m + q - 1) / q;
    return k;
}

struct SqsHostTables {
    const int *inst_atoms, *inst_group, *a2i_off, *a2i, *group_i, *chan_i;
    const double *chan_d, *tab;
    const int *msidx;
    const double *objp;
};

// dims_host: N, m, I, G, C, H, n_tab, A (entries of a2i).  objp (10): mode, atat_tol, d_min, n_body, maxdist0[3], reward[3].
static int sqs_check(const char *who, const int64_t *dims, const SqsHostTables &t, int space, SqsModel &M)
{
    if (space != MDH_HOST) return sqs_bad(who, "the tables and results live in host memory (space must be MDH_HOST)");
    if (!dims || !t.inst_atoms || !t.inst_group || !t.a2i_off || !t.a2i || !t.group_i || !t.chan_i || !t.chan_d || !t.tab ||
        !t.msidx || !t.objp)
        return sqs_bad(who, "a table is NULL");
    const int64_t N = dims[0], m = dims[1], I = dims[2], G = dims[3], C = dims[4], H = dims[5], n_tab = dims[6], A = dims[7];
    if (N < 2 || N > SQS_MAX_ATOMS) return sqs_bad(who, "needs 2 <= N <= 4096 atoms");
    if (m < 2 || m > 8) return sqs_bad(who, "needs 2 <= m <= 8 species");
    if (I < 1 || I > (int64_t)1 << 26) return sqs_bad(who, "needs between 1 and 2^26 cluster instances");
    if (G < 1 || G > SQS_MAX_GROUPS) return sqs_bad(who, "needs between 1 and 1024 (body, shell) groups");
    if (C < 1 || C > (int64_t)1 << 20 || H < 1 || H > (int64_t)1 << 20 || n_tab < 1 || A < 0 || A > 4 * I)
        return sqs_bad(who, "inconsistent table sizes");
    if (sqs_lds_bytes((int)N, (int)G, (int)C, (int)H) > (size_t)SQS_LDS_CAP)
        return sqs_bad(who, "the state of one replica (16 C + 4 H + 4 ceil(G / 32) + 2 N bytes for C channels, H histogram bins) exceeds 65536 bytes of LDS");
    int64_t K[5] = {0, 0, sqs_multisets((int)m, 2), sqs_multisets((int)m, 3), sqs_multisets((int)m, 4)};
    int64_t chans = 0, insts = 0;
    for (int64_t g = 0; g < G; ++g) {
        const int *gi = t.group_i + 6 * g;
        if (gi[0] < 2 || gi[0] > 4) return sqs_bad(who, "a cluster body is outside 2..4");
        if (gi[5] != K[gi[0]] || gi[1] < 0 || (int64_t)gi[1] + gi[5] > H) return sqs_bad(who, "a group's histogram lies outside the H bins");
        if (gi[2] != chans || gi[3] < 1) return sqs_bad(who, "the groups' channels are not consecutive");
        if (gi[4] < 1) return sqs_bad(who, "a group without instances");
        chans += gi[3];
        insts += gi[4];
    }
    if (chans != C || insts != I) return sqs_bad(who, "the groups do not add up to the channels and instances");
    for (int64_t c = 0; c < C; ++c) {
        const int *ci = t.chan_i + 3 * c;
        if (ci[0] < 0 || ci[0] >= G) return sqs_bad(who, "a channel names no group");
        const int *gi = t.group_i + 6 * ci[0];
        if (c < gi[2] || c >= (int64_t)gi[2] + gi[3] || ci[1] != gi[0] - 2) return sqs_bad(who, "a channel does not belong to its group");
        if (ci[2] < 0 || (int64_t)ci[2] + gi[5] > n_tab) return sqs_bad(who, "a channel's table lies outside tab");
    }
    std::vector<int> seen((size_t)G, 0);
    for (int64_t e = 0; e < I; ++e) {
        const int g = t.inst_group[e];
        if (g < 0 || g >= G) return sqs_bad(who, "an instance names no group");
        seen[(size_t)g] += 1;
        const int n = t.group_i[6 * g];
        for (int p = 0; p < 4; ++p) {
            const int a = t.inst_atoms[4 * e + p];
            if (p < n ? (a < 0 || a >= N) : a != -1) return sqs_bad(who, "atom index out of range in instance");
        }
    }
    for (int64_t g = 0; g < G; ++g)
        if (seen[(size_t)g] != t.group_i[6 * g + 4]) return sqs_bad(who, "a group's instance count is wrong");
    if (t.a2i_off[0] != 0 || t.a2i_off[N] != A) return sqs_bad(who, "a2i_off does not span a2i");
    for (int64_t a = 0; a < N; ++a) {
        if (t.a2i_off[a + 1] < t.a2i_off[a]) return sqs_bad(who, "a2i_off decreases");
        for (int q = t.a2i_off[a]; q < t.a2i_off[a + 1]; ++q)
            if (t.a2i[q] < 0 || t.a2i[q] >= I) return sqs_bad(who, "a2i names no instance");
    }
    int64_t off = 0, pw = m;
    for (int n = 2; n <= 4; ++n) {
        pw *= m;
        M.ms_off[n] = (int)off;
        for (int64_t q = 0; q < pw; ++q)
            if (t.msidx[off + q] < 0 || t.msidx[off + q] >= K[n]) return sqs_bad(who, "msidx names no multiset");
        off += pw;
    }
    M.ms_off[0] = M.ms_off[1] = 0;
    const int mode = (int)t.objp[0], n_body = (int)t.objp[3];
    if (mode < 0 || mode > 1 || n_body < 1 || n_body > 3) return sqs_bad(who, "objective mode must be 0 or 1, with 1 to 3 bodies");
    for (int64_t c = 0; c < C; ++c)
        if (t.chan_i[3 * c + 1] >= n_body) return sqs_bad(who, "a channel's body is beyond n_body");
    M.N = (int)N; M.m = (int)m; M.I = (int)I; M.G = (int)G; M.C = (int)C; M.H = (int)H;
    M.mode = mode; M.n_body = n_body;
    M.tol = t.objp[1]; M.d_min = t.objp[2];
    for (int p = 0; p < 3; ++p) { M.maxdist0[p] = t.objp[4 + p]; M.reward[p] = t.objp[7 + p]; }
    return MDH_OK;
}

static bool sqs_types_ok(const int *types, int64_t count, int64_t m)
{
    for (int64_t a = 0; a < count; ++a)
        if (types[a] < 0 || types[a] >= m) return false;
    return true;
}

static void sqs_upload(Scope &sc, const int64_t *dims, const SqsHostTables &t, SqsModel &M)
{
    const size_t N = (size_t)dims[0], m = (size_t)dims[1], I = (size_t)dims[2], G = (size_t)dims[3], C = (size_t)dims[4];
    M.inst_atoms = sc.stage_in(t.inst_atoms, 4 * I, MDH_HOST);
    M.inst_group = sc.stage_in(t.inst_group, I, MDH_HOST);
    M.a2i_off = sc.stage_in(t.a2i_off, N + 1, MDH_HOST);
    M.a2i = sc.stage_in(t.a2i, (size_t)dims[7] ? (size_t)dims[7] : 1, MDH_HOST);
    M.group_i = sc.stage_in(t.group_i, 6 * G, MDH_HOST);
    M.chan_i = sc.stage_in(t.chan_i, 3 * C, MDH_HOST);
    M.chan_d = sc.stage_in(t.chan_d, 4 * C, MDH_HOST);
    M.tab = sc.stage_in(t.tab, (size_t)dims[6], MDH_HOST);
    M.msidx = sc.stage_in(t.msidx, m * m + m * m * m + m * m * m * m, MDH_HOST);
}

} // namespace mdh

using namespace mdh;

extern "C" {

int mdh_sqs_count(const int64_t *dims_host, const int *inst_atoms, const int *inst_group, const int *a2i_off, const int *a2i,
                  const int *group_i, const int *chan_i, const double *chan_d, const double *tab, const int *msidx,
                  const double *objp, const int *types, int64_t R, int *hist, double *corr, double *delta, double *objective,
                  int space, void *stream)
{
    const char *who = "mdh_sqs_count";
    const SqsHostTables t{inst_atoms, inst_group, a2i_off, a2i, group_i, chan_i, chan_d, tab, msidx, objp};
    SqsModel M{};
    MDH_TRY(sqs_check(who, dims_host, t, space, M));
    if (R < 1 || R > (int64_t)1 << 20) return sqs_bad(who, "needs between 1 and 2^20 type vectors");
    if (types == nullptr) return sqs_bad(who, "types is NULL");
    if (!sqs_types_ok(types, R * M.N, M.m)) return sqs_bad(who, "a species is outside [0, m)");
    Scope sc(stream);
    hipStream_t st = sc.stream();
    sqs_upload(sc, dims_host, t, M);
    const int *dtypes = sc.stage_in(types, (size_t)R * M.N, space);
    int *dhist = sc.stage(hist, (size_t)R * M.H, space, false, true);
    double *dcorr = sc.stage(corr, (size_t)R * M.C, space, false, true);
    double *ddelta = sc.stage(delta, (size_t)R * M.C, space, false, true);
    double *dobj = sc.stage(objective, (size_t)R, space, false, true);
    if (sc.failed())
        return sc.error();
    {
        ProfRange pr("sqs_count", st);
        hipLaunchKernelGGL(k_sqs_count, dim3((unsigned)R), dim3(64), sqs_lds_bytes(M.N, M.G, M.C, M.H), st, M, dtypes, dhist, dcorr,
                           ddelta, dobj);
    }
    MDH_HIP(hipGetLastError());
    return sc.finish(space);
}

int mdh_sqs_run(const int64_t *dims_host, const int *inst_atoms, const int *inst_group, const int *a2i_off, const int *a2i,
                const int *group_i, const int *chan_i, const double *chan_d, const double *tab, const int *msidx,
                const double *objp, const int *types0, int64_t max_steps, double T, int64_t R, uint64_t seed, int64_t launch_steps,
                int *winner, int *best_types, double *best_corr, double *objectives, unsigned char *all_best, int space,
                void *stream)
{
    const char *who = "mdh_sqs_run";
    const SqsHostTables t{inst_atoms, inst_group, a2i_off, a2i, group_i, chan_i, chan_d, tab, msidx, objp};
    SqsModel M{};
    MDH_TRY(sqs_check(who, dims_host, t, space, M));
    if (R < 1 || R > (int64_t)1 << 20) return sqs_bad(who, "needs between 1 and 2^20 replicas");
    if (!(T > 0.0)) return sqs_bad(who, "needs T > 0");
    if (max_steps < 0) return sqs_bad(who, "max_steps is negative");
    if (launch_steps < 0) return sqs_bad(who, "launch_steps is negative (0: the library chooses)");
    if (!types0 || !winner || !best_types || !best_corr || !objectives)
        return sqs_bad(who, "types0, winner, best_types, best_corr and objectives are required");
    if (!sqs_types_ok(types0, M.N, M.m)) return sqs_bad(who, "a species is outside [0, m)");
    const int64_t cut = launch_steps > 0 ? launch_steps : SQS_LAUNCH_STEPS;
    Scope sc(stream);
    hipStream_t st = sc.stream();
    sqs_upload(sc, dims_host, t, M);
    const int *dtypes0 = sc.stage_in(types0, (size_t)M.N, space);
    int *dwinner = sc.stage(winner, 1, space, false, true);
    int *dbest_types = sc.stage(best_types, (size_t)M.N, space, false, true);
    double *dbest_corr = sc.stage(best_corr, (size_t)M.C, space, false, true);
    double *dobjectives = sc.stage(objectives, (size_t)R, space, false, true);
    SqsState S;
    S.best = all_best ? sc.stage(all_best, (size_t)R * M.N, space, false, true) : sc.alloc_n<unsigned char>((size_t)R * M.N);
    S.types = sc.alloc_n<unsigned char>((size_t)R * M.N);
    S.hist = sc.alloc_n<int>((size_t)R * M.H);
    S.dc = sc.alloc_n<double>((size_t)R * M.C);
    S.obj = sc.alloc_n<double>((size_t)R * 2);
    if (sc.failed() || !S.best || !S.types || !S.hist || !S.dc || !S.obj)
        return sc.error();
    const size_t lds = sqs_lds_bytes(M.N, M.G, M.C, M.H);
    {
        ProfRange pr("sqs_run", st);
        hipLaunchKernelGGL(k_sqs_init, dim3((unsigned)R), dim3(64), lds, st, M, S, dtypes0, seed, 1);
        for (int64_t s0 = 0; s0 < max_steps; s0 += cut) {
            const int64_t ns = max_steps - s0 < cut ? max_steps - s0 : cut;
            hipLaunchKernelGGL(k_sqs_steps, dim3((unsigned)R), dim3(64), lds, st, M, S, seed, s0, ns, T);
        }
        hipLaunchKernelGGL(k_sqs_pick, dim3(1), dim3(64), lds, st, M, S, R, dwinner, dbest_types, dbest_corr, dobjectives);
    }
    MDH_HIP(hipGetLastError());
    return sc.finish(space);
}
}

MDH_WARM_UNIT(sqs)
