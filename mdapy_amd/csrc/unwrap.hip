// unwrap.hip — wrapped positions pos (F, N, 3) of a trajectory made continuous across the periodic boundaries.  DESIGN.md section
// 5j.  The reference does this in numpy, one frame after the other (src/mdapy/unwrap_trajectory.py:212-255); here it is one
// streaming pass over the trajectory, or two when the frame axis is split.  Everything is IEEE binary64 with no contraction, in
// this order (inv = the inverse of the frame's own cell, rows a, b, c):
//
//   frac[f, i, d]      = (x * inv[f][0][d] + y * inv[f][1][d]) + z * inv[f][2][d]
//   k[f, i, d]         = rint(frac[f-1, i, d] - frac[f, i, d])  on a periodic axis for f >= 1, else 0   (ties to even)
//   s[f, i, :]         = the sum of k[g, i, :] over g <= f, in int64         (minimum-image mode)
//                      = image[f, i, :]                                      (image mode, on all three axes)
//   unwrapped[f, i, d] = p_d + (((double)sx * cell[f][0][d] + (double)sy * cell[f][1][d]) + (double)sz * cell[f][2][d])
//
// One wave owns 64 atoms (lane l the atom i0 + l: the wave's reads and writes of a frame are one run of 64 x 24 bytes) and one
// chunk of frames, which it walks in order, UW_U frames' loads issued ahead of the arithmetic.  The running sum s is a prefix sum
// over time; with C > 1 chunks it is taken in three passes:
//
//   A  k_uw_walk<false>: (chunk c < C - 1, atom) sums its increments -> slot c + 1 of carry (C, N, 3) int64; the first increment
//      of a chunk reads the last frame of the chunk before it
//   B  k_uw_scan: per atom and axis, slot 0 = 0 and slot c += slot c - 1: slot c is what chunks 0 .. c-1 add up to
//   C  k_uw_walk<true>: (chunk, atom) walks its frames again from its carry and writes unwrapped and shifts
//
// The sums are integers, so how the frames are cut changes no bit of the result.  With C == 1 only pass C runs (positions read
// once); image mode is pass C with s read instead of accumulated, the chunks only spreading the frames over the device.
// row_of gathers on the read side in every pass.  A step that is not finite or reaches 2^31 (a NaN position, a degenerate cell)
// and a row_of entry outside [0, N) raise a bit of a flag word instead of being used; the entry point reads the word back.
#include "common.hpp"

namespace mdh {

constexpr int UW_AB = 64;                          // atoms per workgroup: one per lane of its one wave
constexpr int UW_T = 16;                           // chunks = 0 cuts the frames into at most ceil(F / UW_T) chunks
constexpr int UW_U = 4;                            // frames a lane has in flight
constexpr int64_t UW_WAVES = 4096;                 // chunks = 0 splits the frames until about this many waves exist ...
constexpr int64_t UW_ENOUGH = 2048;                // ... unless the atoms alone give this many, or, read through row_of (the
constexpr int64_t UW_ENOUGH_GATHERED = 1024;       // second pass gathers again), this many (profiles/unwrap.md)
constexpr int64_t UW_MAX_FRAMES = (int64_t)1 << 24;
constexpr int64_t UW_MAX_ATOMS = (int64_t)1 << 28;
constexpr int UW_BAD_STEP = 1, UW_BAD_ROW = 2;

struct UwVec { double x, y, z; };

__device__ __forceinline__ int64_t uw_row(const int64_t *__restrict__ row_of, int64_t f, int64_t N, int64_t i, int &bad)
{
    if (row_of == nullptr) return i;
    const int64_t r = row_of[f * N + i];
    if ((uint64_t)r < (uint64_t)N) return r;
    bad |= UW_BAD_ROW; // (never dereferenced: the atom's own row stands in, the call fails)
    return i;
}

// the 24 bytes of one atom as a 16-byte and an 8-byte request (rows start at any 8-byte address)
__device__ __forceinline__ UwVec uw_load(const double *__restrict__ pos, int64_t f, int64_t N, int64_t r)
{
    const double *p = pos + (f * N + r) * 3;
    const RowPair xy = *reinterpret_cast<const RowPair *>(p);
    return UwVec{xy.x, xy.y, p[2]};
}

__device__ __forceinline__ UwVec uw_frac(const UwVec &p, const double *__restrict__ m)
{
    return UwVec{(p.x * m[0] + p.y * m[3]) + p.z * m[6], (p.x * m[1] + p.y * m[4]) + p.z * m[7], (p.x * m[2] + p.y * m[5]) + p.z * m[8]};
}

__device__ __forceinline__ int64_t uw_step(double before, double now, int &bad)
{
    const double d = before - now;
    if (!(fabs(d) < 2147483648.0)) { bad |= UW_BAD_STEP; return 0; }
    return (int64_t)rint(d);
}

// grid: atom blocks x chunks, the atom block fastest.  WRITE = false is pass A (chunks 0 .. C-2, nothing but carry written),
// WRITE = true pass C.  carry may be NULL in pass C (one chunk, or image mode).
template <bool WRITE, bool IMAGE>
__global__ __launch_bounds__(UW_AB) void k_uw_walk(const double *__restrict__ pos, const int64_t *__restrict__ row_of,
                                                   const int32_t *__restrict__ image, const double *__restrict__ cell,
                                                   const double *__restrict__ inv, int px, int py, int pz, int64_t F, int64_t N,
                                                   int64_t C, int64_t nab, int64_t *__restrict__ carry,
                                                   double *__restrict__ unwrapped, int64_t *__restrict__ shifts, int *__restrict__ flag)
{
    const int64_t ab = blockIdx.x % nab, c = blockIdx.x / nab;
    const int64_t i = ab * UW_AB + threadIdx.x;
    const bool have = i < N;
    const int64_t ii = have ? i : N - 1; // (a lane past the end reads the last atom and stores nothing: no branch per load)
    const int64_t f0 = c * F / C, f1 = (c + 1) * F / C;
    int bad = 0;
    int64_t sx = 0, sy = 0, sz = 0;
    UwVec before{0.0, 0.0, 0.0};
    if (!IMAGE) {
        if (WRITE && carry != nullptr) {
            const int64_t *s = carry + (c * N + ii) * 3;
            sx = s[0]; sy = s[1]; sz = s[2];
        }
        if (f0 > 0) before = uw_frac(uw_load(pos, f0 - 1, N, uw_row(row_of, f0 - 1, N, ii, bad)), inv + (f0 - 1) * 9);
    }
    for (int64_t f = f0; f < f1; f += UW_U) {
        int64_t r[UW_U];
        UwVec p[UW_U];
        int32_t im[UW_U][3];
#pragma unroll
        for (int u = 0; u < UW_U; ++u) { // (a frame past the chunk's end is loaded as its last frame and not used)
            const int64_t g = f + u < f1 ? f + u : f1 - 1;
            r[u] = uw_row(row_of, g, N, ii, bad);
        }
#pragma unroll
        for (int u = 0; u < UW_U; ++u) {
            const int64_t g = f + u < f1 ? f + u : f1 - 1;
            p[u] = uw_load(pos, g, N, r[u]);
            if (IMAGE) {
                const int32_t *s = image + (g * N + r[u]) * 3;
                im[u][0] = s[0]; im[u][1] = s[1]; im[u][2] = s[2];
            }
        }
#pragma unroll
        for (int u = 0; u < UW_U; ++u) {
            const int64_t g = f + u;
            if (g < f1) {
                if (IMAGE) {
                    sx = im[u][0]; sy = im[u][1]; sz = im[u][2];
                } else {
                    const UwVec now = uw_frac(p[u], inv + g * 9);
                    if (g > 0) {
                        if (px) sx += uw_step(before.x, now.x, bad);
                        if (py) sy += uw_step(before.y, now.y, bad);
                        if (pz) sz += uw_step(before.z, now.z, bad);
                    }
                    before = now;
                }
                if (WRITE && have) {
                    const double *h = cell + g * 9;
                    const double ax = (double)sx, ay = (double)sy, az = (double)sz;
                    double *out = unwrapped + (g * N + i) * 3;
                    out[0] = p[u].x + ((ax * h[0] + ay * h[3]) + az * h[6]);
                    out[1] = p[u].y + ((ax * h[1] + ay * h[4]) + az * h[7]);
                    out[2] = p[u].z + ((ax * h[2] + ay * h[5]) + az * h[8]);
                    if (shifts != nullptr) {
                        int64_t *s = shifts + (g * N + i) * 3;
                        s[0] = sx; s[1] = sy; s[2] = sz;
                    }
                }
            }
        }
    }
    if (!WRITE && have) {
        int64_t *s = carry + ((c + 1) * N + i) * 3;
        s[0] = sx; s[1] = sy; s[2] = sz;
    }
    if (bad) atomicOr(flag, bad);
}

// pass B: element e of the N x 3 sums; slot 0 = 0, slot c += slot c - 1
__global__ __launch_bounds__(256) void k_uw_scan(int64_t *__restrict__ carry, int64_t C, int64_t n3)
{
    const int64_t e = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (e >= n3) return;
    int64_t sum = 0;
    carry[e] = 0;
    for (int64_t c = 1; c < C; ++c) {
        sum += carry[c * n3 + e];
        carry[c * n3 + e] = sum;
    }
}

// chunks of the frame axis: asked >= 1 is taken as it is; 0 = one chunk when the atoms alone make enough waves (UW_ENOUGH, or
// UW_ENOUGH_GATHERED with row_of), else enough chunks for UW_WAVES waves, none shorter than about UW_T frames.  Never more than F.
static int64_t uw_chunks(int asked, int64_t F, int64_t nab, bool gathered)
{
    int64_t C = asked;
    if (asked == 0) {
        const int64_t want = (UW_WAVES + nab - 1) / nab, most = (F + UW_T - 1) / UW_T;
        C = nab >= (gathered ? UW_ENOUGH_GATHERED : UW_ENOUGH) ? 1 : (want < most ? want : most);
    }
    return C < 1 ? 1 : (C > F ? F : C);
}

} // namespace mdh

using namespace mdh;

extern "C" {

int mdh_unwrap_trajectory(const double *pos, const int64_t *row_of, const int32_t *image, const double *cell_host,
                          const double *inv_host, const int *pbc3_host, int64_t F, int64_t N, int chunks, double *unwrapped,
                          int64_t *shifts, int space, void *stream)
{
    const std::string me("mdh_unwrap_trajectory");
    if (pos == nullptr) { set_error(me + ": pos is NULL"); return MDH_ERR_ARG; }
    if (cell_host == nullptr) { set_error(me + ": cell_host is NULL"); return MDH_ERR_ARG; }
    if (image == nullptr && inv_host == nullptr) { set_error(me + ": inv_host is NULL in minimum-image mode"); return MDH_ERR_ARG; }
    if (pbc3_host == nullptr) { set_error(me + ": pbc3_host is NULL"); return MDH_ERR_ARG; }
    if (unwrapped == nullptr) { set_error(me + ": unwrapped is NULL"); return MDH_ERR_ARG; }
    if (F < 1) { set_error(me + ": needs at least one frame"); return MDH_ERR_ARG; }
    if (N < 1) { set_error(me + ": needs at least one atom"); return MDH_ERR_ARG; }
    if (chunks < 0) { set_error(me + ": chunks is negative"); return MDH_ERR_ARG; }
    if (F > UW_MAX_FRAMES) { set_error(me + ": more than 16 777 216 frames"); return MDH_ERR_ARG; }
    if (N > UW_MAX_ATOMS) { set_error(me + ": more than 268 435 456 atoms"); return MDH_ERR_ARG; }
    const int64_t nab = (N + UW_AB - 1) / UW_AB, C = uw_chunks(chunks, F, nab, row_of != nullptr);
    if (nab * C > 0x7fffffff) { set_error(me + ": atoms x chunks is too large for one launch"); return MDH_ERR_ARG; }
    const bool by_image = image != nullptr, scan = !by_image && C > 1;
    const int px = pbc3_host[0] != 0, py = pbc3_host[1] != 0, pz = pbc3_host[2] != 0;
    const size_t cells = (size_t)F * (size_t)N * 3;

    Scope sc(stream);
    hipStream_t st = sc.stream();
    const double *dpos = sc.stage_in(pos, cells, space);
    const int64_t *drow = sc.stage_in(row_of, (size_t)F * (size_t)N, space);
    const int32_t *dimage = sc.stage_in(image, cells, space);
    const double *dcell = sc.stage_in(cell_host, (size_t)F * 9, MDH_HOST);
    const double *dinv = by_image ? nullptr : sc.stage_in(inv_host, (size_t)F * 9, MDH_HOST);
    double *dout = sc.stage(unwrapped, cells, space, false, true);
    int64_t *dshifts = sc.stage(shifts, cells, space, false, true);
    int64_t *carry = scan ? sc.alloc_n<int64_t>((size_t)C * (size_t)N * 3) : nullptr;
    int *flag = sc.alloc_n<int>(1);
    if (sc.failed() || !dcell || (!by_image && !dinv) || (scan && !carry) || !flag)
        return sc.error();
    MDH_HIP(hipMemsetAsync(flag, 0, sizeof(int), st));
    {
        ProfRange pr("unwrap_trajectory", st);
        const dim3 all((unsigned)(nab * C)), block(UW_AB);
        if (by_image) {
            hipLaunchKernelGGL((k_uw_walk<true, true>), all, block, 0, st, dpos, drow, dimage, dcell, dinv, px, py, pz, F, N, C, nab,
                               carry, dout, dshifts, flag);
        } else {
            if (scan) {
                hipLaunchKernelGGL((k_uw_walk<false, false>), dim3((unsigned)(nab * (C - 1))), block, 0, st, dpos, drow, dimage, dcell,
                                   dinv, px, py, pz, F, N, C, nab, carry, dout, dshifts, flag);
                hipLaunchKernelGGL(k_uw_scan, dim3((unsigned)grid_for(N * 3, 256)), dim3(256), 0, st, carry, C, N * 3);
            }
            hipLaunchKernelGGL((k_uw_walk<true, false>), all, block, 0, st, dpos, drow, dimage, dcell, dinv, px, py, pz, F, N, C, nab,
                               carry, dout, dshifts, flag);
        }
    }
    MDH_HIP(hipGetLastError());
    int raised = 0;
    MDH_HIP(hipMemcpyAsync(&raised, flag, sizeof(int), hipMemcpyDeviceToHost, st));
    MDH_TRY(sc.finish(space));
    MDH_HIP(hipStreamSynchronize(st));
    if (raised & UW_BAD_ROW) { set_error(me + ": row_of holds an entry outside 0 .. atoms - 1"); return MDH_ERR_ARG; }
    if (raised & UW_BAD_STEP) {
        set_error(me + ": a step in fractional coordinates is not finite or reaches 2^31 (a NaN position or a degenerate cell)");
        return MDH_ERR_ARG;
    }
    return MDH_OK;
}
}

MDH_WARM_UNIT(unwrap)
