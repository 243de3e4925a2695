// chill.hip — CHILL+ water-phase identification (Nguyen & Molinero 2015)                src/chill_plus.cpp:27-179
//
// A row entry jj < neighbor_number[i] is a BOND iff distance_list[i, jj] <= rc and verlet_list[i, jj] >= 0; a rejected entry
// is passed over, the row goes on behind it (:114-116).  Two passes over the rows, two launches on one stream:
//   1  q_i[m] = sum over the bonds of Y_3m(d), m = -3 .. 3, d = pbc(r_j - r_i) in f64 and everything after it in f32  (:27-71, :105-125)
//   2  c_ij = Re(sum_m q_i[m] conj(q_j[m])) / (sqrtf(|q_i|^2) sqrtf(|q_j|^2)) over the bonds; eclipsed -0.35 < c < 0.25,
//      staggered c < -0.8; the code from the three counts                                                      (:129-176)
// Pass 1 leaves one 64-byte record per atom — the 14 floats of q, then sqrtf(|q|^2), then a pad — so that a neighbour in pass 2
// is exactly one cache line and the reference's product of two square roots is formed from the same two floats.
//
// f32 throughout, product then add (the Makefile's -ffp-contract=off), IEEE '/' and sqrtf, the reference's order of operations.
// One thing is not the reference's: e^{i phi} is ((float)dx, (float)dy) / xy instead of expf(i atan2f(dy, dx)) — no device
// libm is bitwise the host's, and the quotient is at least as close to the true value.  Where xy == 0 it is (1, 0), which is
// what atan2f(0, 0) = 0 gives; the amplitudes that multiply it are zero there.  DESIGN.md states the parity contract.
#include "common.hpp"

namespace mdh {

struct __attribute__((aligned(16))) ChillQ { float q[14]; float norm; float pad; }; // q[2k], q[2k+1] = Re, Im of m = k - 3
static_assert(sizeof(ChillQ) == 64, "one cache line per atom");

constexpr int CHILL_FLIGHT = 4; // neighbours whose gathers are in flight together: a whole row of four-coordinated ice
static_assert(ROW_CHUNK % CHILL_FLIGHT == 0, "a chunk is a whole number of flights");

// Y_3m of a bond added to q, m = -3 .. 3 in turn (:27-71, :123)
__device__ __forceinline__ void chill_add_y3m(double dx, double dy, double dz, float (&q)[14])
{
    const float r2 = (float)(dx * dx + dy * dy + dz * dz);
    if (r2 <= 0.0f)
        return; // (the reference adds seven zeros)
    const float r = sqrtf(r2);
    const float ct = (float)dz / r;
    const float xy = sqrtf((float)(dx * dx + dy * dy));
    const float st = xy / r;
    constexpr float PI = 3.14159265358979323846f;
    const float N0 = 0.25f * sqrtf(7.0f / PI);
    const float N1 = 0.125f * sqrtf(21.0f / PI);
    const float N2 = 0.25f * sqrtf(105.0f / (2.0f * PI));
    const float N3 = 0.125f * sqrtf(35.0f / PI);
    const float ct2 = ct * ct;
    const float ct3 = ct2 * ct;
    const float st2 = st * st;
    const float st3 = st2 * st;
    // e1 = e^{i phi}; e2 = e1 e1, e3 = e2 e1 as complex products (ac - bd, ad + bc)
    const bool axial = !(xy > 0.0f);
    const float e1r = axial ? 1.0f : (float)dx / xy, e1i = axial ? 0.0f : (float)dy / xy;
    const float e2r = e1r * e1r - e1i * e1i, e2i = e1r * e1i + e1i * e1r;
    const float e3r = e2r * e1r - e2i * e1i, e3i = e2r * e1i + e2i * e1r;
    const float a1 = N1 * st * (5.0f * ct2 - 1.0f);
    const float a2 = N2 * st2 * ct;
    const float a3 = N3 * st3;
    q[0] += a3 * e3r;  q[1] += a3 * -e3i;  // m = -3:  a3 conj(e3)
    q[2] += a2 * e2r;  q[3] += a2 * -e2i;  // m = -2
    q[4] += a1 * e1r;  q[5] += a1 * -e1i;  // m = -1
    q[6] += N0 * (5.0f * ct3 - 3.0f * ct); q[7] += 0.0f; // m = 0
    q[8] += -a1 * e1r; q[9] += -a1 * e1i;  // m = 1
    q[10] += a2 * e2r; q[11] += a2 * e2i;  // m = 2
    q[12] += -a3 * e3r; q[13] += -a3 * e3i; // m = 3
}

// Both passes walk the rows alike.  One thread per atom, one-wave workgroups; the 64 rows of a workgroup a chunk of ROW_CHUNK
// columns at a time through LDS (stage_row_chunk), then CHILL_FLIGHT entries at a time: the records of that many neighbours —
// positions in pass 1, q vectors in pass 2 — are in flight together and use(record) sees the bonds strictly in row order.  An
// entry that is no bond gathers the atom's own record (a line the lane holds already); an index >= N that is not negative reads
// the atom itself too (safe_id) and counts as the bond the reference would have read out of bounds for.
template <class R, class Use>
__device__ __forceinline__ void chill_bonds(const int *__restrict__ verlet, const double *__restrict__ dist, const int *__restrict__ nn,
                                            int64_t N, int64_t M, double rc, const R *__restrict__ table, Use &&use)
{
    __shared__ int ids[ROW_CHUNK * 64];
    __shared__ double dst[ROW_CHUNK * 64];
    const int64_t row0 = (int64_t)blockIdx.x * 64, i = row0 + threadIdx.x;
    const int n = i < N ? min(max(nn[i], 0), (int)M) : 0;
    const int most = wave_max(n);
    for (int c0 = 0; c0 < most; c0 += ROW_CHUNK) {
        __syncthreads();
        stage_row_chunk<true>(verlet, dist, N, M, row0, c0, ids, dst);
        __syncthreads();
        for (int q0 = 0; q0 < ROW_CHUNK && c0 + q0 < n; q0 += CHILL_FLIGHT) {
            bool bond[CHILL_FLIGHT];
            R rec[CHILL_FLIGHT];
#pragma unroll
            for (int u = 0; u < CHILL_FLIGHT; ++u) {
                // (an entry behind the row's end is never a bond, whatever the LDS holds there)
                const int j = ids[(q0 + u) * 64 + threadIdx.x];
                bond[u] = c0 + q0 + u < n && !(dst[(q0 + u) * 64 + threadIdx.x] > rc) && j >= 0;
                rec[u] = table[bond[u] ? safe_id(j, i, N) : i];
            }
#pragma unroll
            for (int u = 0; u < CHILL_FLIGHT; ++u)
                if (bond[u]) use(rec[u]);
        }
    }
}

template <bool TRI>
__global__ __launch_bounds__(64) void k_chill_q(const int *__restrict__ verlet, const double *__restrict__ dist,
                                                const int *__restrict__ nn, int64_t N, int64_t M, DBox b,
                                                const Pos4 *__restrict__ pos, double rc, ChillQ *__restrict__ out)
{
    const int64_t i = (int64_t)blockIdx.x * 64 + threadIdx.x;
    const Pos4 self = pos[i < N ? i : 0];
    float q[14];
#pragma unroll
    for (int k = 0; k < 14; ++k) q[k] = 0.0f;
    chill_bonds(verlet, dist, nn, N, M, rc, pos, [&](const Pos4 &pj) {
        double dx = pj.x - self.x, dy = pj.y - self.y, dz = pj.z - self.z;
        pbc<TRI>(b, dx, dy, dz);
        chill_add_y3m(dx, dy, dz, q);
    });
    if (i < N) {
        ChillQ mine;
        float norm_sq = 0.0f; // :135-136
#pragma unroll
        for (int k = 0; k < 7; ++k) {
            norm_sq += q[2 * k] * q[2 * k] + q[2 * k + 1] * q[2 * k + 1];
            mine.q[2 * k] = q[2 * k];
            mine.q[2 * k + 1] = q[2 * k + 1];
        }
        mine.norm = sqrtf(norm_sq);
        mine.pad = 0.0f;
        out[i] = mine;
    }
}

__global__ __launch_bounds__(64) void k_chill_classify(const int *__restrict__ verlet, const double *__restrict__ dist,
                                                       const int *__restrict__ nn, int64_t N, int64_t M,
                                                       const ChillQ *__restrict__ rec, double rc, int *__restrict__ pattern)
{
    const int64_t i = (int64_t)blockIdx.x * 64 + threadIdx.x;
    const ChillQ qi = rec[i < N ? i : 0];
    int eclipsed = 0, staggered = 0, coordination = 0;
    chill_bonds(verlet, dist, nn, N, M, rc, rec, [&](const ChillQ &qj) {
        float c1 = 0.0f; // Re(q_i[k] conj(q_j[k])) = ac + bd, k in turn (:149-155)
#pragma unroll
        for (int k = 0; k < 7; ++k) c1 += qi.q[2 * k] * qj.q[2 * k] + qi.q[2 * k + 1] * qj.q[2 * k + 1];
        const float denom = qi.norm * qj.norm;
        const float c = denom > 0.0f ? c1 / denom : 0.0f;
        if (c > -0.35f && c < 0.25f) ++eclipsed;
        if (c < -0.8f) ++staggered;
        ++coordination;
    });
    if (i < N) {
        int code = 0; // :165-175
        if (coordination == 4) {
            if (eclipsed == 4) code = 4;
            else if (eclipsed == 3) code = 5;
            else if (staggered == 4) code = 2;
            else if (staggered == 3 && eclipsed == 1) code = 1;
            else if (staggered == 3 && eclipsed == 0) code = 3;
            else if (staggered == 2) code = 3;
        }
        pattern[i] = code;
    }
}

} // namespace mdh

using namespace mdh;

extern "C" int mdh_chill_plus(const double *x, const double *y, const double *z, int64_t N, const double *box9,
                              const double *origin3, const int *boundary3, const int *verlet, const double *dist, const int *nn,
                              int64_t M, double rc, int *pattern, int space, void *stream)
{
    if (N < 0 || N >= ((int64_t)1 << 31) || M <= 0 || !(rc > 0)) {
        set_error("mdh_chill_plus: need a neighbor list (M > 0) and rc > 0");
        return MDH_ERR_ARG;
    }
    DBox b;
    MDH_TRY(make_box(b, box9, origin3, boundary3));
    if (N == 0)
        return MDH_OK;
    Scope sc(stream);
    const double *dx = sc.stage_in(x, (size_t)N, space), *dy = sc.stage_in(y, (size_t)N, space), *dz = sc.stage_in(z, (size_t)N, space);
    const int *dv = sc.stage_in(verlet, (size_t)(N * M), space);
    const double *dd = sc.stage_in(dist, (size_t)(N * M), space);
    const int *dn = sc.stage_in(nn, (size_t)N, space);
    int *dp = sc.stage(pattern, (size_t)N, space, false, true);
    if (sc.failed())
        return sc.error();
    const Pos4 *pos = pack_positions(sc, dx, dy, dz, N);
    ChillQ *rec = sc.alloc_n<ChillQ>((size_t)N);
    if (!pos || !rec)
        return sc.error();
    const dim3 grid(grid_for(N, 64)), block(64);
    {
        ProfRange pr("k_chill_q", sc.stream());
        if (b.tri)
            hipLaunchKernelGGL(k_chill_q<true>, grid, block, 0, sc.stream(), dv, dd, dn, N, M, b, pos, rc, rec);
        else
            hipLaunchKernelGGL(k_chill_q<false>, grid, block, 0, sc.stream(), dv, dd, dn, N, M, b, pos, rc, rec);
    }
    {
        ProfRange pr("k_chill_classify", sc.stream());
        hipLaunchKernelGGL(k_chill_classify, grid, block, 0, sc.stream(), dv, dd, dn, N, M, rec, rc, dp);
    }
    return sc.finish(space);
}

MDH_WARM_UNIT(chill)
