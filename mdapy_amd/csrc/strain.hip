// strain.hip — atomic strain of a current frame against a reference frame      src/atomic_strain.cpp:110-217
//
// For every atom i, over the entries j of i's row of the REFERENCE frame's cutoff list, in list order:
//   d_ref = pbc_ref(r_ref[j] - r_ref[i]),  d_cur = pbc_cur(r_cur[j] - r_cur[i])
//   V[m][n] += d_ref[n] * d_ref[m],  W[m][n] += d_ref[n] * d_cur[m]                                        (:186-191)
// then F = (W V^-1)^T, s = (F^T F - I) / 2, the von Mises shear invariant of s and a third of its trace (:195-215).
// All of it f64, product then add (the Makefile's -ffp-contract=off), every sum in the reference's order: bit for bit.
#include "common.hpp"

namespace mdh {

struct StrainMap { double m[9]; };

// A frame's positions as one 32-byte record per atom (common.hpp Pos4): a neighbour is then two 16-byte requests per frame
// instead of three 8-byte ones from three arrays (see k_pack_velocity_mass in consumers.hip).  MAP: the current frame through
// the affine map of src/mdapy/atomic_strain.py:199-212 on the way — x' = (x m00 + y m10) + z m20, ... ; the origin is not
// subtracted, as in the reference.
template <bool MAP>
__global__ __launch_bounds__(256) void k_strain_pack(const double *__restrict__ x, const double *__restrict__ y,
                                                     const double *__restrict__ z, int64_t N, StrainMap a, Pos4 *__restrict__ out)
{
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= N)
        return;
    const double px = x[i], py = y[i], pz = z[i];
    if (MAP)
        out[i] = Pos4{px * a.m[0] + py * a.m[3] + pz * a.m[6], px * a.m[1] + py * a.m[4] + pz * a.m[7],
                      px * a.m[2] + py * a.m[5] + pz * a.m[8], 0.0};
    else
        out[i] = Pos4{px, py, pz, 0.0};
}

// shear and volumetric strain from V (symmetric: its six distinct sums) and W (row-major, W[m][n] at 3 m + n)
__device__ __forceinline__ void strain_invariants(const double (&v)[6], const double (&w)[9], double &shear, double &volumetric)
{
    const double V[9] = {v[0], v[1], v[2], v[1], v[3], v[4], v[2], v[4], v[5]};
    // the inverse: adjugate times 1 / det, the identity for a singular V (:53-83)
    const double det = V[0] * (V[4] * V[8] - V[5] * V[7]) - V[1] * (V[3] * V[8] - V[5] * V[6]) + V[2] * (V[3] * V[7] - V[4] * V[6]);
    double Vi[9] = {1.0, 0.0, 0.0, 0.0, 1.0, 0.0, 0.0, 0.0, 1.0};
    if (!(fabs(det) < 1e-12)) {
        const double inv = 1.0 / det;
        Vi[0] = (V[4] * V[8] - V[5] * V[7]) * inv;
        Vi[1] = (V[2] * V[7] - V[1] * V[8]) * inv;
        Vi[2] = (V[1] * V[5] - V[2] * V[4]) * inv;
        Vi[3] = (V[5] * V[6] - V[3] * V[8]) * inv;
        Vi[4] = (V[0] * V[8] - V[2] * V[6]) * inv;
        Vi[5] = (V[2] * V[3] - V[0] * V[5]) * inv;
        Vi[6] = (V[3] * V[7] - V[4] * V[6]) * inv;
        Vi[7] = (V[1] * V[6] - V[0] * V[7]) * inv;
        Vi[8] = (V[0] * V[4] - V[1] * V[3]) * inv;
    }
    // P = W V^-1; F = P^T, so F^T F = P P^T.  Every element is 0.0 + the three products in turn (:38-50: the leading 0.0 turns a
    // -0.0 first product into +0.0, and stays)
    double P[9];
#pragma unroll
    for (int r = 0; r < 3; ++r)
#pragma unroll
        for (int c = 0; c < 3; ++c) {
            double sum = 0.0;
#pragma unroll
            for (int k = 0; k < 3; ++k) sum += w[3 * r + k] * Vi[3 * k + c];
            P[3 * r + c] = sum;
        }
    double s[9];
#pragma unroll
    for (int r = 0; r < 3; ++r)
#pragma unroll
        for (int c = 0; c < 3; ++c) {
            double sum = 0.0;
#pragma unroll
            for (int k = 0; k < 3; ++k) sum += P[3 * r + k] * P[3 * c + k];
            s[3 * r + c] = (sum - (r == c ? 1.0 : 0.0)) / 2.0; // :200
        }
    const double xy = s[0] - s[4], yz = s[4] - s[8], xz = s[0] - s[8];
    shear = sqrt(s[1] * s[1] + s[2] * s[2] + s[5] * s[5] + (xy * xy + xz * xz + yz * yz) / 6.0); // :207-212
    volumetric = (s[0] + s[4] + s[8]) / 3.0;
}

// One thread per atom; the rows of the 64 atoms of a workgroup a chunk of ROW_CHUNK columns at a time through LDS
// (stage_row_chunk), then STRAIN_FLIGHT entries at a time: the reference and current records of that many neighbours are in
// flight together, and their contributions are added strictly in list order, so V and W are the sums of the reference's
// entry-by-entry loop.  V is symmetric bit for bit (a product does not depend on the order of its factors, and both halves add
// the same products in the same order): six accumulators stand for its nine.  A row ends at neighbor_number[i] entries or at the
// first entry outside [0, N), whichever comes first: a pad never indexes memory.
constexpr int STRAIN_FLIGHT = 4;

template <bool TRI_REF, bool TRI_CUR>
__global__ __launch_bounds__(64) void k_atomic_strain(const int *__restrict__ verlet, const int *__restrict__ nn, int64_t N, int64_t M,
                                                      DBox rb, DBox cb, const Pos4 *__restrict__ ref, const Pos4 *__restrict__ cur,
                                                      double *__restrict__ shear, double *__restrict__ volumetric)
{
    static_assert(ROW_CHUNK % STRAIN_FLIGHT == 0, "a chunk is a whole number of flights");
    __shared__ int ids[ROW_CHUNK * 64];
    const int64_t row0 = (int64_t)blockIdx.x * 64, i = row0 + threadIdx.x;
    const bool on = i < N;
    const Pos4 ri = ref[on ? i : 0], ci = cur[on ? i : 0];
    const int n = on ? min(max(nn[i], 0), (int)M) : 0;
    const int most = wave_max(n);
    double v[6] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
    double w[9] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
    bool stop = false;
    for (int c0 = 0; c0 < most; c0 += ROW_CHUNK) {
        __syncthreads();
        stage_row_chunk<false>(verlet, nullptr, N, M, row0, c0, ids, nullptr);
        __syncthreads();
        for (int q0 = 0; q0 < ROW_CHUNK && c0 + q0 < n && !stop; q0 += STRAIN_FLIGHT) {
            int js[STRAIN_FLIGHT];
            Pos4 rj[STRAIN_FLIGHT], cj[STRAIN_FLIGHT];
#pragma unroll
            for (int u = 0; u < STRAIN_FLIGHT; ++u) js[u] = ids[(q0 + u) * 64 + threadIdx.x];
#pragma unroll
            for (int u = 0; u < STRAIN_FLIGHT; ++u) {
                // (an entry behind the row's end, whatever the LDS holds there, and a pad read the atom itself: never used)
                const int64_t j = (c0 + q0 + u < n && (unsigned)js[u] < (unsigned)N) ? js[u] : i;
                rj[u] = ref[j];
                cj[u] = cur[j];
            }
#pragma unroll
            for (int u = 0; u < STRAIN_FLIGHT; ++u) {
                if (stop || c0 + q0 + u >= n)
                    continue;
                if ((unsigned)js[u] >= (unsigned)N) { stop = true; continue; }
                double a[3] = {rj[u].x - ri.x, rj[u].y - ri.y, rj[u].z - ri.z};
                pbc<TRI_REF>(rb, a[0], a[1], a[2]);
                double b[3] = {cj[u].x - ci.x, cj[u].y - ci.y, cj[u].z - ci.z};
                pbc<TRI_CUR>(cb, b[0], b[1], b[2]);
                v[0] += a[0] * a[0]; v[1] += a[1] * a[0]; v[2] += a[2] * a[0];
                v[3] += a[1] * a[1]; v[4] += a[2] * a[1]; v[5] += a[2] * a[2];
#pragma unroll
                for (int m = 0; m < 3; ++m)
#pragma unroll
                    for (int k = 0; k < 3; ++k) w[3 * m + k] += a[k] * b[m];
            }
        }
    }
    if (on) {
        double sh, vo;
        strain_invariants(v, w, sh, vo);
        shear[i] = sh;
        volumetric[i] = vo;
    }
}

static void launch_strain(const int *verlet, const int *nn, int64_t N, int64_t M, const DBox &rb, const DBox &cb, const Pos4 *ref,
                          const Pos4 *cur, double *shear, double *volumetric, hipStream_t st)
{
    const dim3 grid(grid_for(N, 64)), block(64);
    ProfRange pr("k_atomic_strain", st);
    if (rb.tri && cb.tri) hipLaunchKernelGGL((k_atomic_strain<true, true>), grid, block, 0, st, verlet, nn, N, M, rb, cb, ref, cur, shear, volumetric);
    else if (rb.tri) hipLaunchKernelGGL((k_atomic_strain<true, false>), grid, block, 0, st, verlet, nn, N, M, rb, cb, ref, cur, shear, volumetric);
    else if (cb.tri) hipLaunchKernelGGL((k_atomic_strain<false, true>), grid, block, 0, st, verlet, nn, N, M, rb, cb, ref, cur, shear, volumetric);
    else hipLaunchKernelGGL((k_atomic_strain<false, false>), grid, block, 0, st, verlet, nn, N, M, rb, cb, ref, cur, shear, volumetric);
}

static void launch_pack(const double *x, const double *y, const double *z, int64_t N, const double *map9_host, Pos4 *out, hipStream_t st)
{
    StrainMap a{};
    if (map9_host) {
        for (int k = 0; k < 9; ++k) a.m[k] = map9_host[k];
        hipLaunchKernelGGL((k_strain_pack<true>), dim3(grid_for(N, 256)), dim3(256), 0, st, x, y, z, N, a, out);
    } else {
        hipLaunchKernelGGL((k_strain_pack<false>), dim3(grid_for(N, 256)), dim3(256), 0, st, x, y, z, N, a, out);
    }
}

static bool strain_shape_ok(int64_t N, int64_t M, const char *who)
{
    if (N < 0 || M < 0 || N >= ((int64_t)1 << 31) || M >= (1 << 23)) {
        set_error(std::string(who) + ": invalid list shape");
        return false;
    }
    return true;
}

} // namespace mdh

using namespace mdh;

extern "C" {

int mdh_strain_pack(const double *x, const double *y, const double *z, int64_t N, const double *map9_host, double *records,
                    int space, void *stream)
{
    if (N < 0 || N >= ((int64_t)1 << 31)) { set_error("mdh_strain_pack: invalid atom count"); return MDH_ERR_ARG; }
    if (N == 0)
        return MDH_OK;
    Scope sc(stream);
    const double *dx = sc.stage_in(x, (size_t)N, space), *dy = sc.stage_in(y, (size_t)N, space), *dz = sc.stage_in(z, (size_t)N, space);
    double *out = sc.stage(records, (size_t)N * 4, space, false, true);
    if (sc.failed())
        return sc.error();
    launch_pack(dx, dy, dz, N, map9_host, reinterpret_cast<Pos4 *>(out), sc.stream());
    return sc.finish(space);
}

int mdh_atomic_strain_records(const int *verlet, const int *nn, int64_t N, int64_t M, const double *ref_box9, const double *ref_origin3,
                              const double *cur_box9, const double *cur_origin3, const int *boundary3, const double *ref_records,
                              const double *cur_records, double *shear, double *volumetric, int space, void *stream)
{
    if (!strain_shape_ok(N, M, "mdh_atomic_strain_records"))
        return MDH_ERR_ARG;
    DBox rb, cb;
    MDH_TRY(make_box(rb, ref_box9, ref_origin3, boundary3));
    MDH_TRY(make_box(cb, cur_box9, cur_origin3, boundary3));
    if (N == 0)
        return MDH_OK;
    Scope sc(stream);
    const int *dv = M ? sc.stage_in(verlet, (size_t)(N * M), space) : nullptr;
    const int *dn = sc.stage_in(nn, (size_t)N, space);
    const double *dr = sc.stage_in(ref_records, (size_t)N * 4, space), *dc = sc.stage_in(cur_records, (size_t)N * 4, space);
    double *ds = sc.stage(shear, (size_t)N, space, false, true), *dw = sc.stage(volumetric, (size_t)N, space, false, true);
    if (sc.failed())
        return sc.error();
    launch_strain(dv, dn, N, M, rb, cb, reinterpret_cast<const Pos4 *>(dr), reinterpret_cast<const Pos4 *>(dc), ds, dw, sc.stream());
    return sc.finish(space);
}

int mdh_atomic_strain(const int *verlet, const int *nn, int64_t N, int64_t M, const double *ref_box9, const double *ref_origin3,
                      const double *cur_box9, const double *cur_origin3, const int *boundary3, const double *ref_x, const double *ref_y,
                      const double *ref_z, const double *cur_x, const double *cur_y, const double *cur_z, const double *map9_host,
                      double *shear, double *volumetric, int space, void *stream)
{
    if (!strain_shape_ok(N, M, "mdh_atomic_strain"))
        return MDH_ERR_ARG;
    DBox rb, cb;
    MDH_TRY(make_box(rb, ref_box9, ref_origin3, boundary3));
    MDH_TRY(make_box(cb, cur_box9, cur_origin3, boundary3));
    if (N == 0)
        return MDH_OK;
    Scope sc(stream);
    const int *dv = M ? sc.stage_in(verlet, (size_t)(N * M), space) : nullptr;
    const int *dn = sc.stage_in(nn, (size_t)N, space);
    const double *rx = sc.stage_in(ref_x, (size_t)N, space), *ry = sc.stage_in(ref_y, (size_t)N, space), *rz = sc.stage_in(ref_z, (size_t)N, space);
    const double *cx = sc.stage_in(cur_x, (size_t)N, space), *cy = sc.stage_in(cur_y, (size_t)N, space), *cz = sc.stage_in(cur_z, (size_t)N, space);
    double *ds = sc.stage(shear, (size_t)N, space, false, true), *dw = sc.stage(volumetric, (size_t)N, space, false, true);
    if (sc.failed())
        return sc.error();
    Pos4 *ref = sc.alloc_n<Pos4>((size_t)N), *cur = sc.alloc_n<Pos4>((size_t)N);
    if (!ref || !cur)
        return sc.error();
    launch_pack(rx, ry, rz, N, nullptr, ref, sc.stream());
    launch_pack(cx, cy, cz, N, map9_host, cur, sc.stream());
    launch_strain(dv, dn, N, M, rb, cb, ref, cur, ds, dw, sc.stream());
    return sc.finish(space);
}
}

MDH_WARM_UNIT(strain)
