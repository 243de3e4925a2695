// msd.hip — mean squared displacement of an unwrapped trajectory pos (F, N, 3): the windowed form (every time origin, lags
// 0 .. L-1) and the direct form (against frame 0).  DESIGN.md section 5h.  The reference has no compiled module for this: it
// takes the windowed form through S1 - 2 S2 with the autocorrelation S2 by FFT, which cancels.  Here the definition itself is
// summed in IEEE binary64:
//
//   term(a, b)         = (dx*dx + dy*dy) + dz*dz,  dx = a.x - b.x, ... (no contraction)
//   window  [m, i]     = (sum over t = 0 .. F-m-1, in that order, of term(r[t+m, i], r[t, i])) / (F - m)
//   direct  [t, i]     = term(r[t, i], r[0, i])
//   msd[m]             = (sum over i of particle_msd[m, i]) / N: a butterfly over the 64 atoms of a block, then the blocks
//                        (k_msd_rows: lane l takes blocks l, l + 64, ... in index order, then a butterfly over the lanes)
//
// Every sum has a fixed order and there is no floating-point atomic: the same input gives the same bits, whatever L is and
// whether or not the caller wants the table.
//
// Window kernel.  A workgroup of four waves owns 64 atoms (one per lane) x MSD_LB = 32 lags, wave w the lags m0 + 8 w .. + 7, and
// walks the time origins t in chunks of MSD_C = 8.  A chunk's origins t0 .. t0+7 ("a" frames) and the frames t0+m0 .. t0+m0+38
// they are paired with ("b" frames) lie in LDS as [frame][x, y, z][atom]; the b frames are a ring of five slabs of 8 frames, of
// which a chunk step replaces one.  A lane keeps its atom's 8 a positions and 8 accumulators (one per lag) in registers and
// streams the 15 b frames its lags pair them with: 64 terms for 69 LDS reads, every index static.  The next chunk's 16 frames
// are fetched from global memory (192 consecutive doubles per frame, one per thread) before the arithmetic and stored to LDS
// after it.  Work per lag block falls linearly with the lag, so a workgroup takes block p and then block (blocks - 1 - p):
// every workgroup walks the same number of chunks, to within one.
#include "common.hpp"

namespace mdh {

constexpr int MSD_AB = 64;                        // atoms per workgroup: one per lane
constexpr int MSD_C = 8;                          // time origins per chunk = frames per LDS slab
constexpr int MSD_LW = 8;                         // lags per wave
constexpr int MSD_WAVES = 4;
constexpr int MSD_LB = MSD_LW * MSD_WAVES;        // lags per workgroup
constexpr int MSD_THREADS = 64 * MSD_WAVES;
constexpr int MSD_SLABS = MSD_WAVES + 1;          // b ring: wave w reads slabs w and w + 1 (relative to the chunk)
constexpr int MSD_FRAME = 3 * MSD_AB;             // doubles of one staged frame
constexpr int MSD_SLAB = MSD_C * MSD_FRAME;       // doubles of one slab
constexpr int MSD_DF = 16;                        // direct mode: frames per workgroup
constexpr int64_t MSD_MAX_FRAMES = (int64_t)1 << 24;
constexpr int64_t MSD_MAX_ATOMS = (int64_t)1 << 28;
static_assert(MSD_LW == MSD_C, "a wave's lags span exactly two slabs of the b ring");

__device__ __forceinline__ double msd_term(double ax, double ay, double az, double bx, double by, double bz)
{
    const double dx = ax - bx, dy = ay - by, dz = az - bz;
    return (dx * dx + dy * dy) + dz * dz;
}

// the sum of v over the wave (every lane gets the same bits: the adds of a butterfly commute)
__device__ __forceinline__ double msd_sum64(double v)
{
#pragma unroll
    for (int d = 1; d <= 32; d <<= 1) v = v + __shfl_xor(v, d, 64);
    return v;
}

// One chunk of one wave: acc[j] += term(b[u + j], a[u]) for u = 0 .. 7 in order, j = 0 .. 7.  a: the chunk's slab of origins;
// b0 / b1: the two slabs that hold b frames s = 0 .. 7 / 8 .. 14 of this wave; b frame s is frame `first + s` of the trajectory
// and takes part while that is < F (CHECK: the chunk reaches the end of the trajectory).
template <bool CHECK>
__device__ __forceinline__ void msd_chunk(const double *__restrict__ a, const double *__restrict__ b0, const double *__restrict__ b1,
                                          int lane, int64_t first, int64_t F, double (&acc)[MSD_LW])
{
    double ax[MSD_C], ay[MSD_C], az[MSD_C];
#pragma unroll
    for (int u = 0; u < MSD_C; ++u) {
        ax[u] = a[u * MSD_FRAME + lane];
        ay[u] = a[u * MSD_FRAME + MSD_AB + lane];
        az[u] = a[u * MSD_FRAME + 2 * MSD_AB + lane];
    }
#pragma unroll
    for (int s = 0; s < MSD_C + MSD_LW - 1; ++s) {
        if (!CHECK || first + s < F) {
            const double *b = s < MSD_C ? b0 + s * MSD_FRAME : b1 + (s - MSD_C) * MSD_FRAME;
            const double bx = b[lane], by = b[MSD_AB + lane], bz = b[2 * MSD_AB + lane];
#pragma unroll
            for (int u = 0; u < MSD_C; ++u) {
                const int j = s - u;
                if (j >= 0 && j < MSD_LW) acc[j] = acc[j] + msd_term(bx, by, bz, ax[u], ay[u], az[u]);
            }
        }
    }
}

// grid: atom blocks x pairs of lag blocks, the pair index fastest.  partial[m * nab + ab] = the block's sum of particle_msd[m, .]
__global__ __launch_bounds__(MSD_THREADS, 2) void k_msd_window(const double *__restrict__ pos, int64_t F, int64_t N, int64_t L,
                                                               int64_t nab, int64_t nlb, int64_t npair,
                                                               double *__restrict__ particle, double *__restrict__ partial)
{
    __shared__ double lds[(1 + MSD_SLABS) * MSD_SLAB];
    double *const sa = lds, *const sb = lds + MSD_SLAB;
    const int tid = threadIdx.x, lane = tid & 63, w = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int64_t ab = blockIdx.x / npair, pair = blockIdx.x % npair;
    const int64_t i0 = ab * MSD_AB, n3 = N * 3;
    // staging: thread tid < 192 brings in double tid of the block's 192 of every frame (atom tid / 3, coordinate tid % 3).  A
    // frame past the end is never used in a term and an atom past the end never stored, so their loads are not skipped but
    // clamped to the last frame / the last double: no branch per load.
    const int64_t ge = i0 * 3 + tid < n3 ? i0 * 3 + tid : n3 - 1, last = F - 1;
    const int dst = (tid % 3) * MSD_AB + tid / 3;
    const int64_t i = i0 + lane;

    for (int turn = 0; turn < 2; ++turn) {
        const int64_t lb = turn == 0 ? pair : nlb - 1 - pair;
        if (turn == 1 && lb == pair) break; // the middle block of an odd count
        const int64_t m0 = lb * MSD_LB, mw = m0 + w * MSD_LW;
        const int64_t T = F - m0; // time origins of the block's smallest lag
        const bool busy = mw < L;  // (a wave whose lags are all past L only helps with the staging)
        double acc[MSD_LW];
#pragma unroll
        for (int j = 0; j < MSD_LW; ++j) acc[j] = 0.0;

        // frames 0 .. 7 -> a, frames m0 .. m0 + 39 -> the b ring
        if (tid < MSD_FRAME) {
#pragma unroll
            for (int k = 0; k < MSD_C; ++k) sa[k * MSD_FRAME + dst] = pos[(k < last ? k : last) * n3 + ge];
            for (int k0 = 0; k0 < MSD_SLABS * MSD_C; k0 += MSD_C) {
                double v[MSD_C];
#pragma unroll
                for (int k = 0; k < MSD_C; ++k) {
                    const int64_t f = m0 + k0 + k;
                    v[k] = pos[(f < last ? f : last) * n3 + ge];
                }
#pragma unroll
                for (int k = 0; k < MSD_C; ++k) sb[(k0 + k) * MSD_FRAME + dst] = v[k];
            }
        }
        __syncthreads();

        int slab = 0; // the ring slab that holds b frames t0 + m0 .. + 7: (t0 / 8) % 5
        for (int64_t t0 = 0; t0 < T; t0 += MSD_C) {
            const bool more = t0 + MSD_C < T;
            double na[MSD_C], nb[MSD_C];
            if (more && tid < MSD_FRAME) { // the next chunk's origins and the slab that follows the ring
#pragma unroll
                for (int k = 0; k < MSD_C; ++k) {
                    const int64_t fa = t0 + MSD_C + k, fb = t0 + m0 + MSD_SLABS * MSD_C + k;
                    na[k] = pos[(fa < last ? fa : last) * n3 + ge];
                    nb[k] = pos[(fb < last ? fb : last) * n3 + ge];
                }
            }
            if (busy) {
                int s0 = slab + w;
                s0 = s0 >= MSD_SLABS ? s0 - MSD_SLABS : s0;
                const int s1 = s0 + 1 == MSD_SLABS ? 0 : s0 + 1;
                const int64_t first = t0 + mw;
                if (first + (MSD_C + MSD_LW - 2) < F)
                    msd_chunk<false>(sa, sb + s0 * MSD_SLAB, sb + s1 * MSD_SLAB, lane, first, F, acc);
                else
                    msd_chunk<true>(sa, sb + s0 * MSD_SLAB, sb + s1 * MSD_SLAB, lane, first, F, acc);
            }
            __syncthreads(); // every wave is done with a and with the ring's oldest slab
            if (more && tid < MSD_FRAME) {
#pragma unroll
                for (int k = 0; k < MSD_C; ++k) {
                    sa[k * MSD_FRAME + dst] = na[k];
                    sb[slab * MSD_SLAB + k * MSD_FRAME + dst] = nb[k];
                }
            }
            slab = slab + 1 == MSD_SLABS ? 0 : slab + 1;
            __syncthreads();
        }

        if (busy) {
#pragma unroll
            for (int j = 0; j < MSD_LW; ++j) {
                const int64_t m = mw + j;
                if (m < L) {
                    const double value = acc[j] / (double)(F - m);
                    if (particle && i < N) particle[m * N + i] = value;
                    if (partial) {
                        const double sum = msd_sum64(i < N ? value : 0.0);
                        if (lane == 0) partial[m * nab + ab] = sum;
                    }
                }
            }
        }
    }
}

// direct mode.  grid: atom blocks x groups of MSD_DF frames, the atom block fastest; wave w takes frames w, w + 4, ... of its group
__global__ __launch_bounds__(MSD_THREADS) void k_msd_direct(const double *__restrict__ pos, int64_t F, int64_t N, int64_t nab,
                                                            double *__restrict__ particle, double *__restrict__ partial)
{
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    const int64_t ab = blockIdx.x % nab, group = blockIdx.x / nab;
    const int64_t i = ab * MSD_AB + lane, n3 = N * 3;
    const bool have = i < N;
    const int64_t e = have ? i * 3 : 0;
    const double x0 = pos[e], y0 = pos[e + 1], z0 = pos[e + 2];
    const int64_t end = group * MSD_DF + MSD_DF < F ? group * MSD_DF + MSD_DF : F;
    for (int64_t t = group * MSD_DF + w; t < end; t += MSD_WAVES) {
        const double *r = pos + t * n3 + e;
        const double value = msd_term(r[0], r[1], r[2], x0, y0, z0);
        if (particle && have) particle[t * N + i] = value;
        if (partial) {
            const double sum = msd_sum64(have ? value : 0.0);
            if (lane == 0) partial[t * nab + ab] = sum;
        }
    }
}

// msd[m] = (the sum of the atom blocks' sums) / N, one wave per row: lane l adds blocks l, l + 64, ... in index order (the lanes
// of a load read 64 consecutive doubles), then the butterfly over the lanes.  A fixed order that depends on N alone.
__global__ __launch_bounds__(64) void k_msd_rows(const double *__restrict__ partial, int64_t nab, double atoms, double *__restrict__ msd)
{
    const int lane = threadIdx.x;
    const int64_t m = blockIdx.x;
    const double *p = partial + m * nab;
    double sum = 0.0;
    for (int64_t b = lane; b < nab; b += 64) sum = sum + p[b];
    sum = msd_sum64(sum);
    if (lane == 0) msd[m] = sum / atoms;
}

static bool msd_args_ok(const double *pos, int64_t F, int64_t N, int64_t L, const double *particle, const double *msd, const char *who)
{
    const std::string me(who);
    if (pos == nullptr) { set_error(me + ": pos is NULL"); return false; }
    if (F < 1) { set_error(me + ": needs at least one frame"); return false; }
    if (N < 1) { set_error(me + ": needs at least one atom"); return false; }
    if (L < 1 || L > F) { set_error(me + ": the number of lags must be in 1 .. frames"); return false; }
    if (particle == nullptr && msd == nullptr) { set_error(me + ": particle_msd and msd are both NULL"); return false; }
    if (F > MSD_MAX_FRAMES) { set_error(me + ": more than 16 777 216 frames"); return false; }
    if (N > MSD_MAX_ATOMS) { set_error(me + ": more than 268 435 456 atoms"); return false; }
    return true;
}

} // namespace mdh

using namespace mdh;

extern "C" {

int mdh_msd_window(const double *pos, int64_t F, int64_t N, int64_t L, double *particle_msd, double *msd, int space, void *stream)
{
    if (!msd_args_ok(pos, F, N, L, particle_msd, msd, "mdh_msd_window"))
        return MDH_ERR_ARG;
    const int64_t nab = (N + MSD_AB - 1) / MSD_AB, nlb = (L + MSD_LB - 1) / MSD_LB, npair = (nlb + 1) / 2;
    if (nab * npair > 0x7fffffff) { set_error("mdh_msd_window: atoms x lags is too large for one launch"); return MDH_ERR_ARG; }
    Scope sc(stream);
    hipStream_t st = sc.stream();
    const double *dpos = sc.stage_in(pos, (size_t)F * (size_t)N * 3, space);
    double *dparticle = sc.stage(particle_msd, (size_t)L * (size_t)N, space, false, true);
    double *dmsd = sc.stage(msd, (size_t)L, space, false, true);
    double *partial = msd ? sc.alloc_n<double>((size_t)L * (size_t)nab) : nullptr;
    if (sc.failed() || (msd && !partial))
        return sc.error();
    {
        ProfRange pr("msd_window", st);
        hipLaunchKernelGGL(k_msd_window, dim3((unsigned)(nab * npair)), dim3(MSD_THREADS), 0, st, dpos, F, N, L, nab, nlb, npair,
                           dparticle, partial);
        if (msd)
            hipLaunchKernelGGL(k_msd_rows, dim3((unsigned)L), dim3(64), 0, st, partial, nab, (double)N, dmsd);
    }
    MDH_HIP(hipGetLastError());
    return sc.finish(space);
}

int mdh_msd_direct(const double *pos, int64_t F, int64_t N, double *particle_msd, double *msd, int space, void *stream)
{
    if (!msd_args_ok(pos, F, N, F, particle_msd, msd, "mdh_msd_direct"))
        return MDH_ERR_ARG;
    const int64_t nab = (N + MSD_AB - 1) / MSD_AB, groups = (F + MSD_DF - 1) / MSD_DF;
    if (nab * groups > 0x7fffffff) { set_error("mdh_msd_direct: atoms x frames is too large for one launch"); return MDH_ERR_ARG; }
    Scope sc(stream);
    hipStream_t st = sc.stream();
    const double *dpos = sc.stage_in(pos, (size_t)F * (size_t)N * 3, space);
    double *dparticle = sc.stage(particle_msd, (size_t)F * (size_t)N, space, false, true);
    double *dmsd = sc.stage(msd, (size_t)F, space, false, true);
    double *partial = msd ? sc.alloc_n<double>((size_t)F * (size_t)nab) : nullptr;
    if (sc.failed() || (msd && !partial))
        return sc.error();
    {
        ProfRange pr("msd_direct", st);
        hipLaunchKernelGGL(k_msd_direct, dim3((unsigned)(nab * groups)), dim3(MSD_THREADS), 0, st, dpos, F, N, nab, dparticle, partial);
        if (msd)
            hipLaunchKernelGGL(k_msd_rows, dim3((unsigned)F), dim3(64), 0, st, partial, nab, (double)N, dmsd);
    }
    MDH_HIP(hipGetLastError());
    return sc.finish(space);
}
}

MDH_WARM_UNIT(msd)
