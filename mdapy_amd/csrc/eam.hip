// eam.hip — embedded-atom energies, forces and virials over a cutoff list                      src/eam.cpp:85-182
//
// Pass 1, for every atom i over the entries j of its row, in list order, with r the list's distance:
//   rho_i += rho_{t_j}(r)  where r <= rc                                                                    (:90-104)
//   F_i, dF_i = F_{t_i}.evaluate_and_derivative(rho_i)                                                     (:107-113)
// Pass 2, over the same entries in the same order, d = pbc(r_j - r_i):
//   z2, dz2 = (r phi)_{t_i t_j}(r);  rinv = 1 / r;  phi = z2 rinv;  dphi = (dz2 - phi) rinv
//   pf = ((dphi + dF_i rho'_{t_j}(r)) + dF_j rho'_{t_i}(r)) rinv;  fp = pf d;  f += fp;  v[3a+b] -= d[a] fp[b];  e += 0.5 phi
//   energy = (E0 + F_i) + e,  force = F0 + f,  virial = V0 + v * 0.5                                        (:117-182)
// E0, F0, V0: what the arrays hold when the call accumulates, 0.0 otherwise.  The splines are the reference's
// UniformCubicSpline (src/spline.h:394-500): the coefficients come from the host, one 32-byte knot (a, b, c, d) per
// interval; locate, Horner and the derivative are its expressions.  All of it f64, product then add (-ffp-contract=off).
#include "common.hpp"
#include <algorithm>

namespace mdh {

struct __attribute__((aligned(16))) Knot { double a, b, c, d; };

// spline.h:461-468 — the interval of x and the offset into it; m < 0 clamps to knot 0 with no offset, m > n - 1 takes the last
// slot (a straight line).  The conversion saturates, and a NaN converts to 0: the index is inside [0, n) whatever x is.
__device__ __forceinline__ int locate(double x, double h, int n, double &dx)
{
    int m = (int)(x / h);
    if (m < 0) { dx = 0.0; return 0; }
    if (m > n - 1) m = n - 1;
    dx = x - m * h;
    return m;
}
__device__ __forceinline__ double knot_value(const Knot &k, double dx) { return k.a + (k.b + (k.c + k.d * dx) * dx) * dx; } // :474
__device__ __forceinline__ double knot_slope(const Knot &k, double dx) { return k.b + (2.0 * k.c + 3.0 * k.d * dx) * dx; } // :481

// positions and type as one 32-byte record per atom (common.hpp Pos4, w = the type): pass 2 reads a neighbour's position and its
// type in the same two 16-byte requests
__global__ __launch_bounds__(256) void k_eam_pack(const double *__restrict__ x, const double *__restrict__ y, const double *__restrict__ z,
                                                  const int *__restrict__ type, int64_t N, Pos4 *__restrict__ out)
{
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i < N)
        out[i] = Pos4{x[i], y[i], z[i], (double)type[i]};
}

// One thread per atom, rows through LDS a chunk at a time (stage_row_chunk, ids and distances), EAM_FLIGHT entries at a time: first
// the neighbours' types (pass 2: records and dF) are in flight together, then the knots they select; contributions are added
// strictly in list order.  A row ends at nn[i] entries or at the first entry outside [0, N): a pad never indexes memory.  What the
// LDS holds behind a row's end is never used: locate() clamps whatever distance it is given into the table.
// A type outside [0, nelem) contributes nothing (as j) and receives nothing (as i).
constexpr int EAM_FLIGHT = 4;

__global__ __launch_bounds__(64) void k_eam_density(const int *__restrict__ verlet, const double *__restrict__ dist, const int *__restrict__ nn,
                                                    int64_t N, int64_t M, const int *__restrict__ type, const Knot *__restrict__ rho_tab,
                                                    const Knot *__restrict__ F_tab, int nelem, int nrho, double drho, int nr, double dr,
                                                    double rc, double *__restrict__ dF, double *__restrict__ Femb)
{
    static_assert(ROW_CHUNK % EAM_FLIGHT == 0, "a chunk is a whole number of flights");
    __shared__ int ids[ROW_CHUNK * 64];
    __shared__ double dst[ROW_CHUNK * 64];
    const int64_t row0 = (int64_t)blockIdx.x * 64, i = row0 + threadIdx.x;
    const bool on = i < N;
    const int ti = on ? type[i] : -1;
    const bool mine = (unsigned)ti < (unsigned)nelem;
    const int n = mine ? min(max(nn[i], 0), (int)M) : 0;
    const int most = wave_max(n);
    double rho = 0.0;
    bool stop = false;
    for (int c0 = 0; c0 < most; c0 += ROW_CHUNK) {
        __syncthreads();
        stage_row_chunk<true>(verlet, dist, N, M, row0, c0, ids, dst);
        __syncthreads();
        for (int q0 = 0; q0 < ROW_CHUNK && c0 + q0 < n && !stop; q0 += EAM_FLIGHT) {
            int js[EAM_FLIGHT], tj[EAM_FLIGHT];
            double rs[EAM_FLIGHT], dx[EAM_FLIGHT];
            Knot kn[EAM_FLIGHT];
#pragma unroll
            for (int u = 0; u < EAM_FLIGHT; ++u) {
                js[u] = ids[(q0 + u) * 64 + threadIdx.x];
                rs[u] = dst[(q0 + u) * 64 + threadIdx.x];
            }
#pragma unroll
            for (int u = 0; u < EAM_FLIGHT; ++u)
                tj[u] = type[(c0 + q0 + u < n && (unsigned)js[u] < (unsigned)N) ? js[u] : i];
#pragma unroll
            for (int u = 0; u < EAM_FLIGHT; ++u) {
                const int m = locate(rs[u], dr, nr, dx[u]);
                kn[u] = rho_tab[((unsigned)tj[u] < (unsigned)nelem ? tj[u] : 0) * nr + m];
            }
#pragma unroll
            for (int u = 0; u < EAM_FLIGHT; ++u) {
                if (stop || c0 + q0 + u >= n)
                    continue;
                if ((unsigned)js[u] >= (unsigned)N) { stop = true; continue; }
                if (rs[u] <= rc && (unsigned)tj[u] < (unsigned)nelem)
                    rho += knot_value(kn[u], dx[u]);
            }
        }
    }
    if (on) {
        double dx;
        const int m = locate(rho, drho, nrho, dx);
        const Knot k = F_tab[(mine ? ti : 0) * nrho + m];
        Femb[i] = mine ? knot_value(k, dx) : 0.0;
        dF[i] = mine ? knot_slope(k, dx) : 0.0;
    }
}

template <bool TRI>
__global__ __launch_bounds__(64) void k_eam_pair(const int *__restrict__ verlet, const double *__restrict__ dist, const int *__restrict__ nn,
                                                 int64_t N, int64_t M, DBox b, const Pos4 *__restrict__ rec, const double *__restrict__ dF,
                                                 const double *__restrict__ Femb, const Knot *__restrict__ rho_tab,
                                                 const Knot *__restrict__ rphi_tab, int nelem, int nr, double dr, double rc, int accumulate,
                                                 double *__restrict__ energy, double *__restrict__ force, double *__restrict__ virial)
{
    __shared__ int ids[ROW_CHUNK * 64];
    __shared__ double dst[ROW_CHUNK * 64];
    const int64_t row0 = (int64_t)blockIdx.x * 64, i = row0 + threadIdx.x;
    const bool on = i < N;
    const Pos4 ri = rec[on ? i : 0];
    const int ti = on ? (int)ri.w : -1;
    const bool mine = (unsigned)ti < (unsigned)nelem;
    const double dFi = on ? dF[i] : 0.0;
    const int n = mine ? min(max(nn[i], 0), (int)M) : 0;
    const int most = wave_max(n);
    const int own = (mine ? ti : 0) * nr, pairs = (mine ? ti : 0) * nelem;
    double e = 0.0, f[3] = {0.0, 0.0, 0.0};
    double v[9] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
    bool stop = false;
    for (int c0 = 0; c0 < most; c0 += ROW_CHUNK) {
        __syncthreads();
        stage_row_chunk<true>(verlet, dist, N, M, row0, c0, ids, dst);
        __syncthreads();
        for (int q0 = 0; q0 < ROW_CHUNK && c0 + q0 < n && !stop; q0 += EAM_FLIGHT) {
            int js[EAM_FLIGHT], tj[EAM_FLIGHT];
            double rs[EAM_FLIGHT], dx[EAM_FLIGHT], dFj[EAM_FLIGHT];
            Pos4 rj[EAM_FLIGHT];
            Knot kz[EAM_FLIGHT], kj[EAM_FLIGHT], ki[EAM_FLIGHT];
#pragma unroll
            for (int u = 0; u < EAM_FLIGHT; ++u) {
                js[u] = ids[(q0 + u) * 64 + threadIdx.x];
                rs[u] = dst[(q0 + u) * 64 + threadIdx.x];
            }
#pragma unroll
            for (int u = 0; u < EAM_FLIGHT; ++u) {
                // (an entry behind the row's end and a pad read the atom itself: never used)
                const int64_t j = (c0 + q0 + u < n && (unsigned)js[u] < (unsigned)N) ? js[u] : i;
                rj[u] = rec[j];
                dFj[u] = dF[j];
            }
#pragma unroll
            for (int u = 0; u < EAM_FLIGHT; ++u) {
                tj[u] = (int)rj[u].w;
                const int t = (unsigned)tj[u] < (unsigned)nelem ? tj[u] : 0;
                const int m = locate(rs[u], dr, nr, dx[u]);
                kz[u] = rphi_tab[(pairs + t) * nr + m];
                kj[u] = rho_tab[t * nr + m];
                ki[u] = rho_tab[own + m];
            }
#pragma unroll
            for (int u = 0; u < EAM_FLIGHT; ++u) {
                if (stop || c0 + q0 + u >= n)
                    continue;
                if ((unsigned)js[u] >= (unsigned)N) { stop = true; continue; }
                if (!(rs[u] <= rc) || (unsigned)tj[u] >= (unsigned)nelem)
                    continue;
                double d[3] = {rj[u].x - ri.x, rj[u].y - ri.y, rj[u].z - ri.z};
                pbc<TRI>(b, d[0], d[1], d[2]);
                const double z2 = knot_value(kz[u], dx[u]), dz2 = knot_slope(kz[u], dx[u]);
                const double rinv = 1.0 / rs[u];
                const double phi = z2 * rinv;
                const double dphi = (dz2 - phi) * rinv;
                const double drho_j = knot_slope(kj[u], dx[u]), drho_i = knot_slope(ki[u], dx[u]);
                e += 0.5 * phi;
                double pf = dphi + dFi * drho_j + dFj[u] * drho_i;
                pf *= rinv;
                const double fp[3] = {pf * d[0], pf * d[1], pf * d[2]};
#pragma unroll
                for (int a = 0; a < 3; ++a) f[a] += fp[a];
#pragma unroll
                for (int a = 0; a < 3; ++a)
#pragma unroll
                    for (int c = 0; c < 3; ++c) v[3 * a + c] -= d[a] * fp[c];
            }
        }
    }
    if (!on || (accumulate && !mine))
        return;
    if (accumulate) {
        energy[i] = (energy[i] + Femb[i]) + e;
#pragma unroll
        for (int a = 0; a < 3; ++a) force[3 * i + a] += f[a];
#pragma unroll
        for (int a = 0; a < 9; ++a) virial[9 * i + a] += v[a] * 0.5;
    } else {
        energy[i] = (0.0 + Femb[i]) + e;
#pragma unroll
        for (int a = 0; a < 3; ++a) force[3 * i + a] = 0.0 + f[a];
#pragma unroll
        for (int a = 0; a < 9; ++a) virial[9 * i + a] = 0.0 + v[a] * 0.5;
    }
}

// The nine column sums of an (n x 9) array in a fixed order, without atomics: 252 = 28 x 9 threads of a block walk the flat array
// with a stride that is a multiple of nine, so thread t only ever meets column t % 9; the 28 threads of a column are then added in
// turn.  Applied twice — the virials into one row of nine per block, those rows into the result — it is a two-level tree whose shape
// depends on n alone: two runs give the same bits.
constexpr int VSUM_THREADS = 252, VSUM_BLOCKS = 1024;

__global__ __launch_bounds__(256) void k_column_sums9(const double *__restrict__ v, int64_t total, double *__restrict__ out)
{
    __shared__ double s[VSUM_THREADS];
    const int t = threadIdx.x;
    if (t < VSUM_THREADS) {
        double acc = 0.0;
        const int64_t step = (int64_t)gridDim.x * VSUM_THREADS;
#pragma unroll 4
        for (int64_t k = (int64_t)blockIdx.x * VSUM_THREADS + t; k < total; k += step) acc += v[k];
        s[t] = acc;
    }
    __syncthreads();
    if (t < 9) {
        double sum = 0.0;
        for (int r = 0; r < VSUM_THREADS / 9; ++r) sum += s[9 * r + t];
        out[(int64_t)blockIdx.x * 9 + t] = sum;
    }
}

void launch_virial_sum(Scope &sc, const double *virial, int64_t n_real, double *sum9)
{
    const int blocks = (int)std::min<int64_t>(VSUM_BLOCKS, std::max<int64_t>(1, (n_real * 9 + VSUM_THREADS - 1) / VSUM_THREADS));
    double *partial = sc.alloc_n<double>((size_t)blocks * 9);
    if (!partial)
        return;
    ProfRange pr("k_column_sums9", sc.stream());
    hipLaunchKernelGGL(k_column_sums9, dim3(blocks), dim3(256), 0, sc.stream(), virial, n_real * 9, partial);
    hipLaunchKernelGGL(k_column_sums9, dim3(1), dim3(256), 0, sc.stream(), (const double *)partial, (int64_t)blocks * 9, sum9);
}

} // namespace mdh

using namespace mdh;

extern "C" {

int mdh_eam(const double *x, const double *y, const double *z, const int *type, int64_t N, const double *box9, const double *origin3,
            const int *boundary3, const int *verlet, const double *dist, const int *nn, int64_t M, const double *F_knots,
            const double *rho_knots, const double *rphi_knots, int nelem, int nrho, double drho, int nr, double dr, double rc,
            int accumulate, double *energy, double *force, double *virial, int64_t n_real, double *virial_sum9, int space, void *stream)
{
    if (N < 0 || M < 0 || N >= ((int64_t)1 << 31) || M >= (1 << 23)) { set_error("mdh_eam: invalid list shape"); return MDH_ERR_ARG; }
    if (nelem < 1 || nr < 2 || nrho < 2 || !(dr > 0.0) || !(drho > 0.0) || !(rc > 0.0)) {
        set_error("mdh_eam: nelem >= 1, nr >= 2, nrho >= 2 and positive dr, drho, rc are required");
        return MDH_ERR_ARG;
    }
    if ((int64_t)nelem * nelem * nr >= ((int64_t)1 << 28) || (int64_t)nelem * nrho >= ((int64_t)1 << 28)) {
        set_error("mdh_eam: tables too large");
        return MDH_ERR_ARG;
    }
    if (n_real < 0 || n_real > N) { set_error("mdh_eam: n_real outside [0, N]"); return MDH_ERR_ARG; }
    DBox b;
    MDH_TRY(make_box(b, box9, origin3, boundary3));
    if (N == 0 && !virial_sum9)
        return MDH_OK;
    Scope sc(stream);
    double *dsum = virial_sum9 ? sc.stage(virial_sum9, (size_t)9, space, false, true) : nullptr;
    if (N == 0) {
        if (sc.failed())
            return sc.error();
        launch_virial_sum(sc, nullptr, 0, dsum);
        return sc.failed() ? sc.error() : sc.finish(space);
    }
    const double *dx = sc.stage_in(x, (size_t)N, space), *dy = sc.stage_in(y, (size_t)N, space), *dz = sc.stage_in(z, (size_t)N, space);
    const int *dt = sc.stage_in(type, (size_t)N, space);
    const int *dv = M ? sc.stage_in(verlet, (size_t)(N * M), space) : nullptr;
    const double *dd = M ? sc.stage_in(dist, (size_t)(N * M), space) : nullptr;
    const int *dn = sc.stage_in(nn, (size_t)N, space);
    const double *tF = sc.stage_in(F_knots, (size_t)nelem * nrho * 4, space);
    const double *tr = sc.stage_in(rho_knots, (size_t)nelem * nr * 4, space);
    const double *tz = sc.stage_in(rphi_knots, (size_t)nelem * nelem * nr * 4, space);
    const bool add = accumulate != 0;
    double *de = sc.stage(energy, (size_t)N, space, add, true), *df = sc.stage(force, (size_t)N * 3, space, add, true);
    double *dw = sc.stage(virial, (size_t)N * 9, space, add, true);
    if (sc.failed())
        return sc.error();
    Pos4 *rec = sc.alloc_n<Pos4>((size_t)N);
    double *dF = sc.alloc_n<double>((size_t)N), *Femb = sc.alloc_n<double>((size_t)N);
    if (!rec || !dF || !Femb)
        return sc.error();
    hipStream_t st = sc.stream();
    const dim3 grid(grid_for(N, 64)), block(64);
    hipLaunchKernelGGL(k_eam_pack, dim3(grid_for(N, 256)), dim3(256), 0, st, dx, dy, dz, dt, N, rec);
    {
        ProfRange pr("k_eam_density", st);
        hipLaunchKernelGGL(k_eam_density, grid, block, 0, st, dv, dd, dn, N, M, dt, reinterpret_cast<const Knot *>(tr),
                           reinterpret_cast<const Knot *>(tF), nelem, nrho, drho, nr, dr, rc, dF, Femb);
    }
    {
        ProfRange pr("k_eam_pair", st);
        if (b.tri)
            hipLaunchKernelGGL((k_eam_pair<true>), grid, block, 0, st, dv, dd, dn, N, M, b, rec, dF, Femb, reinterpret_cast<const Knot *>(tr),
                               reinterpret_cast<const Knot *>(tz), nelem, nr, dr, rc, (int)add, de, df, dw);
        else
            hipLaunchKernelGGL((k_eam_pair<false>), grid, block, 0, st, dv, dd, dn, N, M, b, rec, dF, Femb, reinterpret_cast<const Knot *>(tr),
                               reinterpret_cast<const Knot *>(tz), nelem, nr, dr, rc, (int)add, de, df, dw);
    }
    if (dsum) {
        launch_virial_sum(sc, dw, n_real, dsum);
        if (sc.failed())
            return sc.error();
    }
    return sc.finish(space);
}
}

MDH_WARM_UNIT(eam)
