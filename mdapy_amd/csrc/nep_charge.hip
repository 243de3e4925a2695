// nep_charge.hip — the charge-aware NEP models of GPUMD (nep4_charge1/2/3), written from the definition.
//
// The network of atom i has a second output, the charge q_i = sum_n w1q[n] tanh(w0[n] . x - b0[n]); the mean charge of the real
// atoms is removed.  With alpha = pi / rc (rc the model's largest radial cutoff), K = e^2 / (4 pi eps0) and tap = 2 alpha / sqrt(pi)
// the energy gains
//   k-space (modes 1, 2)  K sum_k G_k |S(k)|^2,  S(k) = sum_i q_i e^{-i k.r_i},  G_k = 2 (2 pi / V) / k^2 exp(-k^2 / (4 alpha^2)),
//                         k = n1 b1 + n2 b2 + n3 b3 with 0 < k^2 < (2 pi alpha)^2 in the half space (n1 > 0, or n1 = 0 and n2 > 0,
//                         or n1 = n2 = 0 and n3 > 0), b_i the reciprocal vectors of the REAL cell
//   real space (mode 1)   K (1/2 sum_ij q_i q_j erfc(alpha d) / d - tap / 2 sum_i q_i^2)        over list entries with d < rc
//   real space (mode 3)   K 1/2 sum_ij q_i q_j (erfc(alpha d) / d + A d + B)                    zero with its slope at d = rc
// D_i is the derivative of that energy with respect to q_i; the model's forces are those of nep.hip's pair pass with Fp_E + D_i Fp_q
// and A_E + D_i A_q.  The same pass with (Fp_q, A_q) alone gives g_ij = dq_i / dr_ij and the Born effective charge
//   bec_i = sqrt(eps_inf) (q_i 1 + 1/2 sum_j r_ij (x) (g_ij + g_ji)).
//
// The passes, no atomics, every sum in an order that depends on the list, N and the k-points alone:
//   A   k_nep_descriptor<Q>   nep.hip's pass A with the charge, Fp_q and A_q as further outputs
//       k_nepq_mean/_center   the mean of the first n_real charges (256 strided partial sums, halved) and (x, y, z, q - mean) records
//   K1  k_nepq_sfactor        four k-points per lane; e^{-i k.r} from per-axis phase tables e^{i n b_d.r} of a few atoms at a time in
//                             LDS (three complex products a term), the atoms added in index order; with few k-points the atoms are
//                             cut into segments (their number follows from the two counts), whose partial sums
//                             k_nepq_sfactor_sum adds in segment order
//   K2  k_nepq_atoms          one atom per lane and four waves a block: wave w takes 64 consecutive k-points of every staged tile of
//                             256 (48 B each: k, G, S, and their integer triple); along a run of consecutive n3 the phase advances by
//                             one complex product; the four waves' ten sums are added in wave order through LDS.  With few atoms the
//                             k-points are cut into ranges, whose sums k_nepq_atoms_sum adds in range order.
//                             (The variant with one sincos per term was measured and lost: profiles/qnep.md.)
//                             One term per (atom, k-point): the k-space part is O(N^2), as in the reference
//   R   k_nepq_real           8 lanes per atom over its row, as the gather; adds to what K2 left (mode 1) or starts from zero (mode 3)
//   B1, B2                    nep.hip's pair pass and gather; the gather starts from the electrostatic force and virial
//   Z   pair pass again with (Fp_q, A_q), then k_nepq_bec, a gather of r_ij (x) (g_ij + g_ji)
// All arithmetic is f64, product then add (-ffp-contract=off).
#include "nep_core.hpp"
#include <cmath>

namespace mdh {

constexpr int NEPQ_TILE = 256, NEPQ_WAVES = 4, NEPQ_SUMS = 10;  // the per-atom k-space sums: the energy, the force (3), the symmetric virial (6)
constexpr int64_t NEPQ_MAX_LATTICE = (int64_t)1 << 28;  // integer triples the host is willing to walk for the k-points

struct KPoint { double kx, ky, kz, G, Sr, Si; };
struct KIndex { int n1, n2, n3, pad; };  // k = n1 b1 + n2 b2 + n3 b3
// the reciprocal vectors (rows), and the per-axis phase tables of the structure factor: L1 = t0 + 1 entries for n1 = 0 .. t0,
// L2 = 2 t1 + 1 for n2 = -t1 .. t1, L3 likewise; TA: the atoms whose tables one block holds in LDS at a time
struct Recip { double b[9]; int L1, L2, L3, t1, t2, TA; };
constexpr int NEPQ_KPL = 4;  // k-points per lane of the structure factor
struct ChargeConst { double alpha, tap, A, B, rc, quarter_inv_alpha2; int mode; };

__global__ __launch_bounds__(256) void k_nepq_mean(const double *__restrict__ q, int64_t n_real, double *__restrict__ mean)
{
    __shared__ double part[256];
    double s = 0.0;
    for (int64_t i = threadIdx.x; i < n_real; i += 256) s += q[i];
    part[threadIdx.x] = s;
    __syncthreads();
    for (int h = 128; h >= 1; h >>= 1) {
        if ((int)threadIdx.x < h)
            part[threadIdx.x] += part[threadIdx.x + h];
        __syncthreads();
    }
    if (threadIdx.x == 0)
        mean[0] = n_real > 0 ? part[0] / (double)n_real : 0.0;
}

__global__ __launch_bounds__(256) void k_nepq_center(double *__restrict__ q, int64_t N, const double *__restrict__ mean,
                                                     const Pos4 *__restrict__ rec, Pos4 *__restrict__ xq, double *__restrict__ charge_out)
{
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= N)
        return;
    const double v = q[i] - mean[0];
    q[i] = v;
    const Pos4 r = rec[i];
    xq[i] = Pos4{r.x, r.y, r.z, v};
    if (charge_out)
        charge_out[i] = v;
}

// grid (blocks of 1024 k-points, atom segments); part: (segments, nk, 2).  e^{-i k.r} = conj(P1[n1] P2[n2] P3[n3]) with
// P_d[n] = e^{i n b_d.r}: the tables of TA atoms at a time in LDS, one sincos per entry, three complex products per term; every lane
// takes NEPQ_KPL k-points, so that a table entry serves many terms.  The atoms of a segment are added in index order
__global__ __launch_bounds__(NEPQ_TILE) void k_nepq_sfactor(const Pos4 *__restrict__ xq, int64_t n_real, int64_t seg_len,
                                                                  const KIndex *__restrict__ kn, int64_t nk, Recip rb, double *__restrict__ part)
{
    extern __shared__ double tab[];  // (TA, L, 2)
    const int L = rb.L1 + rb.L2 + rb.L3;
    int o1[NEPQ_KPL], o2[NEPQ_KPL], o3[NEPQ_KPL];
    double sr[NEPQ_KPL], si[NEPQ_KPL];
#pragma unroll
    for (int j = 0; j < NEPQ_KPL; ++j) {
        const int64_t k = ((int64_t)blockIdx.x * NEPQ_KPL + j) * NEPQ_TILE + threadIdx.x;
        const KIndex n = k < nk ? kn[k] : KIndex{0, 0, 0, 0};
        o1[j] = n.n1; o2[j] = rb.L1 + n.n2 + rb.t1; o3[j] = rb.L1 + rb.L2 + n.n3 + rb.t2;
        sr[j] = si[j] = 0.0;
    }
    const int64_t lo = (int64_t)blockIdx.y * seg_len, hi = min(n_real, lo + seg_len);
    for (int64_t base = lo; base < hi; base += rb.TA) {
        const int count = (int)min((int64_t)rb.TA, hi - base);
        for (int e = threadIdx.x; e < count * L; e += NEPQ_TILE) {
            const int a = e / L, m = e - a * L;
            const int axis = m < rb.L1 ? 0 : (m < rb.L1 + rb.L2 ? 1 : 2);
            const int n = axis == 0 ? m : (axis == 1 ? m - rb.L1 - rb.t1 : m - rb.L1 - rb.L2 - rb.t2);
            const Pos4 r = xq[base + a];
            const double th = rb.b[3 * axis] * r.x + rb.b[3 * axis + 1] * r.y + rb.b[3 * axis + 2] * r.z;
            double sn, cs;
            sincos((double)n * th, &sn, &cs);
            tab[2 * e] = cs;
            tab[2 * e + 1] = sn;
        }
        __syncthreads();
        for (int a = 0; a < count; ++a) {
            const double q = xq[base + a].w;
            const double *row = tab + 2 * (a * L);
#pragma unroll
            for (int j = 0; j < NEPQ_KPL; ++j) {
                const double c1 = row[2 * o1[j]], s1 = row[2 * o1[j] + 1], c2 = row[2 * o2[j]], s2 = row[2 * o2[j] + 1];
                const double c3 = row[2 * o3[j]], s3 = row[2 * o3[j] + 1];
                const double c12 = c1 * c2 - s1 * s2, s12 = c1 * s2 + s1 * c2;
                sr[j] += q * (c12 * c3 - s12 * s3);
                si[j] -= q * (c12 * s3 + s12 * c3);
            }
        }
        __syncthreads();
    }
#pragma unroll
    for (int j = 0; j < NEPQ_KPL; ++j) {
        const int64_t k = ((int64_t)blockIdx.x * NEPQ_KPL + j) * NEPQ_TILE + threadIdx.x;
        if (k < nk) {
            part[((int64_t)blockIdx.y * nk + k) * 2] = sr[j];
            part[((int64_t)blockIdx.y * nk + k) * 2 + 1] = si[j];
        }
    }
}

__global__ __launch_bounds__(256) void k_nepq_sfactor_sum(const double *__restrict__ part, int segments, int64_t nk, KPoint *__restrict__ kp)
{
    const int64_t k = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (k >= nk)
        return;
    double sr = 0.0, si = 0.0;
    for (int s = 0; s < segments; ++s) {
        sr += part[((int64_t)s * nk + k) * 2];
        si += part[((int64_t)s * nk + k) * 2 + 1];
    }
    kp[k].Sr = sr;
    kp[k].Si = si;
}

// grid (blocks of 64 atoms, k-point ranges of klen); part: (ranges, NEPQ_SUMS, N).  A block stages its range 256 k-points at a time and
// wave w takes the 64 consecutive ones w * 64 ..  Along a run of consecutive n3 at the same (n1, n2) — the order the k-points are
// made in — e^{i k.r} follows from the last one by one complex product with e^{i b3.r}; a sincos only where a run begins
__global__ __launch_bounds__(64 * NEPQ_WAVES) void k_nepq_atoms(const Pos4 *__restrict__ xq, int64_t N, const KPoint *__restrict__ kp,
                                                                const KIndex *__restrict__ kn, int64_t nk, int64_t klen, ChargeConst cc, Recip rb,
                                                                double *__restrict__ part)
{
    __shared__ KPoint tile[NEPQ_TILE];
    __shared__ KIndex tilen[NEPQ_TILE];
    __shared__ double sums[NEPQ_WAVES][NEPQ_SUMS][64];
    const int lane = threadIdx.x % 64, wave = threadIdx.x / 64;
    const int64_t i = (int64_t)blockIdx.x * 64 + lane;
    const bool on = i < N;
    const Pos4 r = xq[on ? i : 0];
    double th[3], s3, c3;
#pragma unroll
    for (int d = 0; d < 3; ++d) th[d] = rb.b[3 * d] * r.x + rb.b[3 * d + 1] * r.y + rb.b[3 * d + 2] * r.z;
    sincos(th[2], &s3, &c3);
    double e = 0.0, f[3] = {0.0, 0.0, 0.0}, v[6] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
    const int64_t lo = (int64_t)blockIdx.y * klen, hi = min(nk, lo + klen);
    for (int64_t base = lo; base < hi; base += NEPQ_TILE) {
        const int count = (int)min((int64_t)NEPQ_TILE, hi - base);
        if ((int)threadIdx.x < count) {
            tile[threadIdx.x] = kp[base + threadIdx.x];
            tilen[threadIdx.x] = kn[base + threadIdx.x];
        }
        __syncthreads();
        const int first = wave * 64, last = min(count, first + 64);
        double s = 0.0, c = 1.0;
        int p1 = 0, p2 = 0, p3 = 0;
        bool have = false;
        for (int t = first; t < last; ++t) {
            const KPoint p = tile[t];
            const KIndex n = tilen[t];
            if (have && n.n1 == p1 && n.n2 == p2 && n.n3 == p3 + 1) {
                const double cn = c * c3 - s * s3;
                s = s * c3 + c * s3;
                c = cn;
            } else {
                sincos(((double)n.n1 * th[0] + (double)n.n2 * th[1]) + (double)n.n3 * th[2], &s, &c);
            }
            p1 = n.n1; p2 = n.n2; p3 = n.n3;
            have = true;
            const double gse = p.G * (p.Sr * c - p.Si * s), gim = p.G * (p.Sr * s + p.Si * c);
            const double ksq = p.kx * p.kx + p.ky * p.ky + p.kz * p.kz;
            const double factor = 2.0 * cc.quarter_inv_alpha2 + 2.0 / ksq;
            e += gse;
            f[0] += p.kx * gim;
            f[1] += p.ky * gim;
            f[2] += p.kz * gim;
            v[0] += gse * (1.0 - factor * (p.kx * p.kx));
            v[1] += gse * (1.0 - factor * (p.ky * p.ky));
            v[2] += gse * (1.0 - factor * (p.kz * p.kz));
            v[3] -= gse * (factor * (p.kx * p.ky));
            v[4] -= gse * (factor * (p.ky * p.kz));
            v[5] -= gse * (factor * (p.kz * p.kx));
        }
        __syncthreads();
    }
    sums[wave][0][lane] = e;
    sums[wave][1][lane] = f[0]; sums[wave][2][lane] = f[1]; sums[wave][3][lane] = f[2];
#pragma unroll
    for (int a = 0; a < 6; ++a) sums[wave][4 + a][lane] = v[a];
    __syncthreads();
    if (wave != 0 || !on)
        return;
#pragma unroll
    for (int a = 0; a < NEPQ_SUMS; ++a) {
        double t = sums[0][a][lane];
#pragma unroll
        for (int w = 1; w < NEPQ_WAVES; ++w) t += sums[w][a][lane];
        part[((int64_t)blockIdx.y * NEPQ_SUMS + a) * N + i] = t;
    }
}

// the ranges' sums in range order; writes D, fc (N, 3), vc (N, 9) and adds the k-space energy to energy
__global__ __launch_bounds__(256) void k_nepq_atoms_sum(const double *__restrict__ part, int ranges, const Pos4 *__restrict__ xq, int64_t N,
                                                        double *__restrict__ energy, double *__restrict__ D, double *__restrict__ fc,
                                                        double *__restrict__ vc)
{
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= N)
        return;
    double t[NEPQ_SUMS];
#pragma unroll
    for (int a = 0; a < NEPQ_SUMS; ++a) {
        double sum = 0.0;
        for (int y = 0; y < ranges; ++y) sum += part[((int64_t)y * NEPQ_SUMS + a) * N + i];
        t[a] = sum;
    }
    const double kq = NEP_COULOMB * xq[i].w;
    energy[i] += kq * t[0];
    D[i] = 2.0 * NEP_COULOMB * t[0];
#pragma unroll
    for (int a = 0; a < 3; ++a) fc[3 * i + a] = (2.0 * kq) * t[1 + a];
    const double xx = kq * t[4], yy = kq * t[5], zz = kq * t[6], xy = kq * t[7], yz = kq * t[8], zx = kq * t[9];
    double *w = vc + 9 * i;
    w[0] = xx; w[1] = xy; w[2] = zx; w[3] = xy; w[4] = yy; w[5] = yz; w[6] = zx; w[7] = yz; w[8] = zz;
}

// the real-space part over the rows; FIRST: nothing ran before it (mode 3), D, fc and vc are written, else added to
template <bool TRI, bool FIRST>
__global__ __launch_bounds__(64) void k_nepq_real(const int *__restrict__ verlet, const double *__restrict__ dist, const int *__restrict__ nn,
                                                  int64_t N, int64_t M, DBox b, const Pos4 *__restrict__ rec, const double *__restrict__ q,
                                                  ChargeConst cc, double *__restrict__ energy, double *__restrict__ D, double *__restrict__ fc,
                                                  double *__restrict__ vc)
{
    constexpr int W = NEP_GATHER_W, G = 64 / W;
    const int lane = threadIdx.x % W, grp = threadIdx.x / W;
    const int64_t i = (int64_t)blockIdx.x * G + grp;
    const bool on = i < N;
    const Pos4 ri = rec[on ? i : 0];
    const double qi = on ? q[i] : 0.0;
    const int n = (on && ri.w >= 0.0) ? min(max(nn[i], 0), (int)M) : 0;
    double e = 0.0, dsum = 0.0, f[3] = {0.0, 0.0, 0.0};
    double v[9] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
    for (int slot = lane; slot < n; slot += W) {
        const int j = verlet[i * M + slot];
        if ((unsigned)j >= (unsigned)N)
            continue;
        const Pos4 rj = rec[j];
        const double d = dist[i * M + slot];
        if (rj.w < 0.0 || !(d < cc.rc))
            continue;
        double r[3] = {rj.x - ri.x, rj.y - ri.y, rj.z - ri.z};
        nep_image<TRI>(b, r[0], r[1], r[2]);
        const double qj = q[j], qq = qi * qj;
        const double screened = erfc(cc.alpha * d) / d;
        double phi = screened, slope = (screened + cc.tap * exp(-(cc.alpha * cc.alpha) * (d * d))) / (d * d);
        if (cc.mode == 3) {
            phi += cc.A * d + cc.B;
            slope -= cc.A / d;
        }
        const double f2 = (-0.5 * NEP_COULOMB) * qq * slope;
        e += (0.5 * NEP_COULOMB) * qq * phi;
        dsum += NEP_COULOMB * qj * phi;
#pragma unroll
        for (int a = 0; a < 3; ++a) f[a] += (2.0 * f2) * r[a];
#pragma unroll
        for (int a = 0; a < 3; ++a)
#pragma unroll
            for (int c = 0; c < 3; ++c) v[3 * a + c] -= r[a] * (f2 * r[c]);
    }
    e = group_sum<W>(e);
    dsum = group_sum<W>(dsum);
#pragma unroll
    for (int a = 0; a < 3; ++a) f[a] = group_sum<W>(f[a]);
#pragma unroll
    for (int a = 0; a < 9; ++a) v[a] = group_sum<W>(v[a]);
    if (!on || lane != 0)
        return;
    if (cc.mode == 1) {  // the self terms
        e += (-NEP_COULOMB * cc.tap * 0.5) * (qi * qi);
        dsum += (-NEP_COULOMB * cc.tap) * qi;
    }
    energy[i] += e;
    D[i] = FIRST ? dsum : D[i] + dsum;
#pragma unroll
    for (int a = 0; a < 3; ++a) fc[3 * i + a] = FIRST ? f[a] : fc[3 * i + a] + f[a];
#pragma unroll
    for (int a = 0; a < 9; ++a) vc[9 * i + a] = FIRST ? v[a] : vc[9 * i + a] + v[a];
}

// bec_i = sqrt(eps_inf) (q_i 1 + 1/2 sum_j r_ij (x) (g_ij + g_ji)), g the pair table of (Fp_q, A_q); g_ji where row j names i
template <bool TRI>
__global__ __launch_bounds__(64) void k_nepq_bec(const int *__restrict__ verlet, const int *__restrict__ nn, int64_t N, int64_t M, DBox b,
                                                 const Pos4 *__restrict__ rec, const double *__restrict__ table, const double *__restrict__ q,
                                                 const double *__restrict__ sqrt_eps, double *__restrict__ bec)
{
    constexpr int W = NEP_GATHER_W, G = 64 / W;
    const int lane = threadIdx.x % W, grp = threadIdx.x / W;
    const int64_t i = (int64_t)blockIdx.x * G + grp;
    const bool on = i < N;
    const Pos4 ri = rec[on ? i : 0];
    const int n = (on && ri.w >= 0.0) ? min(max(nn[i], 0), (int)M) : 0;
    double z[9] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
    for (int slot = lane; slot < n; slot += W) {
        const int j = verlet[i * M + slot];
        if ((unsigned)j >= (unsigned)N)
            continue;
        const Pos4 rj = rec[j];
        if (rj.w < 0.0)
            continue;
        double d[3] = {rj.x - ri.x, rj.y - ri.y, rj.z - ri.z};
        nep_image<TRI>(b, d[0], d[1], d[2]);
        const int back = nep_back(verlet, nn, M, j, i);
        const double *mine = table + (i * M + slot) * 3;
        double both[3] = {mine[0], mine[1], mine[2]};
        if (back >= 0) {
            const double *theirs = table + ((int64_t)j * M + back) * 3;
            both[0] += theirs[0]; both[1] += theirs[1]; both[2] += theirs[2];
        }
#pragma unroll
        for (int a = 0; a < 3; ++a)
#pragma unroll
            for (int c = 0; c < 3; ++c) z[3 * a + c] += 0.5 * (d[a] * both[c]);
    }
#pragma unroll
    for (int a = 0; a < 9; ++a) z[a] = group_sum<W>(z[a]);
    if (!on || lane != 0)
        return;
    const double qi = q[i], scale = sqrt_eps[0];
#pragma unroll
    for (int a = 0; a < 9; ++a) bec[9 * i + a] = ((a % 4 == 0 ? qi : 0.0) + z[a]) * scale;
}

// the k-points of the cell (rows of cell9 are its vectors) in the order n1, n2, n3 rising -> MDH_OK, or MDH_ERR_ARG with the error set
static int nepq_k_points(const double *cell9, double alpha, int64_t max_kpoints, std::vector<KPoint> &out, std::vector<KIndex> &index, Recip &rb)
{
    const double *a1 = cell9, *a2 = cell9 + 3, *a3 = cell9 + 6;
    auto cross = [](const double *u, const double *v, double *w) {
        w[0] = u[1] * v[2] - u[2] * v[1]; w[1] = u[2] * v[0] - u[0] * v[2]; w[2] = u[0] * v[1] - u[1] * v[0];
    };
    double b[3][3];
    cross(a2, a3, b[0]);
    cross(a3, a1, b[1]);
    cross(a1, a2, b[2]);
    const double det = a1[0] * b[0][0] + a1[1] * b[0][1] + a1[2] * b[0][2];
    if (!(std::fabs(det) > 0.0) || !std::isfinite(det)) { set_error("mdh_nep_charge: the k-space cell has no volume"); return MDH_ERR_ARG; }
    const double two_pi = 2.0 * NEP_PI;
    for (auto &row : b)
        for (double &v : row) v *= two_pi / det;
    double top[3];
    const double *a[3] = {a1, a2, a3};
    for (int i = 0; i < 3; ++i) top[i] = std::floor(alpha * std::sqrt(a[i][0] * a[i][0] + a[i][1] * a[i][1] + a[i][2] * a[i][2]));
    if (!((top[0] + 1.0) * (2.0 * top[1] + 1.0) * (2.0 * top[2] + 1.0) <= (double)NEPQ_MAX_LATTICE)) {
        set_error("mdh_nep_charge: more k-points than the scratch holds");
        return MDH_ERR_ARG;
    }
    const int t0 = (int)top[0], t1 = (int)top[1], t2 = (int)top[2];
    const double ksq_max = (two_pi * alpha) * (two_pi * alpha), G0 = 2.0 * (two_pi / std::fabs(det)), af = 0.25 / (alpha * alpha);
    for (int d = 0; d < 3; ++d)
        for (int c = 0; c < 3; ++c) rb.b[3 * d + c] = b[d][c];
    rb.L1 = t0 + 1; rb.L2 = 2 * t1 + 1; rb.L3 = 2 * t2 + 1; rb.t1 = t1; rb.t2 = t2;
    rb.TA = (int)std::min<int64_t>(16, (48 * 1024) / (16 * ((int64_t)rb.L1 + rb.L2 + rb.L3)));
    if (rb.TA < 1) { set_error("mdh_nep_charge: a cell this long has more phase-table entries than LDS holds"); return MDH_ERR_ARG; }
    out.clear();
    index.clear();
    for (int n1 = 0; n1 <= t0; ++n1)
        for (int n2 = -t1; n2 <= t1; ++n2)
            for (int n3 = -t2; n3 <= t2; ++n3) {
                if ((n1 == 0 && n2 < 0) || (n1 == 0 && n2 == 0 && n3 <= 0))
                    continue;
                const double kx = n1 * b[0][0] + n2 * b[1][0] + n3 * b[2][0], ky = n1 * b[0][1] + n2 * b[1][1] + n3 * b[2][1],
                             kz = n1 * b[0][2] + n2 * b[1][2] + n3 * b[2][2];
                const double ksq = kx * kx + ky * ky + kz * kz;
                if (!(ksq < ksq_max))
                    continue;
                if ((int64_t)out.size() >= max_kpoints) { set_error("mdh_nep_charge: more k-points than the scratch holds"); return MDH_ERR_ARG; }
                out.push_back(KPoint{kx, ky, kz, G0 / ksq * std::exp(-ksq * af), 0.0, 0.0});
                index.push_back(KIndex{n1, n2, n3, 0});
            }
    return MDH_OK;
}

} // namespace mdh

using namespace mdh;

extern "C" {

int mdh_nep_charge(const double *x, const double *y, const double *z, const int *type, int64_t N, const int *type_map_host, int nfile,
                   const double *box9, const double *origin3, const int *boundary3, const int *verlet, const double *dist, const int *nn,
                   int64_t M, const double *model, const int *head12_host, const double *zbl3_host, const double *kcell9_host,
                   double rc_coulomb, int64_t max_kpoints, int64_t n_real, double *energy, double *force, double *virial, double *virial_sum9,
                   double *charge, double *bec, double *descriptor, double *latent, int space, void *stream)
{
    if (N < 0 || M < 0 || N >= ((int64_t)1 << 31) || M >= (1 << 23)) { set_error("mdh_nep_charge: invalid list shape"); return MDH_ERR_ARG; }
    if (!head12_host || !zbl3_host || !type_map_host || !kcell9_host) {
        set_error("mdh_nep_charge: the model's header, ZBL numbers, type map and the k-space cell are required");
        return MDH_ERR_ARG;
    }
    if (n_real < 0 || n_real > N) { set_error("mdh_nep_charge: n_real outside [0, N]"); return MDH_ERR_ARG; }
    if (virial_sum9 && !virial) { set_error("mdh_nep_charge: virial_sum9 needs virial"); return MDH_ERR_ARG; }
    if (!(rc_coulomb > 0.0) || !std::isfinite(rc_coulomb) || max_kpoints < 0) {
        set_error("mdh_nep_charge: the Coulomb cutoff must be positive and max_kpoints not negative");
        return MDH_ERR_ARG;
    }
    NepModel m;
    int64_t len = 0;
    MDH_TRY(nep_model_of("mdh_nep_charge", head12_host, nfile, zbl3_host, type_map_host, true, m, len));
    if (space == MDH_HOST && type)
        for (int64_t i = 0; i < N; ++i)
            if (type[i] < 0 || type[i] >= nfile) { set_error("mdh_nep_charge: an atom's type outside the type map"); return MDH_ERR_ARG; }
    DBox b;
    MDH_TRY(make_box(b, box9, origin3, boundary3));
    ChargeConst cc;
    cc.mode = m.charge;
    cc.rc = rc_coulomb;
    cc.alpha = NEP_PI / rc_coulomb;
    cc.tap = 2.0 * cc.alpha / std::sqrt(NEP_PI);
    cc.A = std::erfc(NEP_PI) / (rc_coulomb * rc_coulomb) + cc.tap * std::exp(-NEP_PI * NEP_PI) / rc_coulomb;
    cc.B = -std::erfc(NEP_PI) / rc_coulomb - cc.A * rc_coulomb;
    cc.quarter_inv_alpha2 = 0.25 / (cc.alpha * cc.alpha);
    std::vector<KPoint> kpoints;
    std::vector<KIndex> kindex;
    Recip rb = {};
    if (cc.mode != 3)
        MDH_TRY(nepq_k_points(kcell9_host, cc.alpha, max_kpoints, kpoints, kindex, rb));
    const int64_t nk = (int64_t)kpoints.size();
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
    NepTypeMap dmap;
    for (int t = 0; t < NEP_MAX_FILE_TYPES; ++t) dmap.local[t] = (signed char)(t < nfile ? type_map_host[t] : -1);
    const int *dv = M ? sc.stage_in(verlet, (size_t)(N * M), space) : nullptr;
    const double *dd = M ? sc.stage_in(dist, (size_t)(N * M), space) : nullptr;
    const int *dn = sc.stage_in(nn, (size_t)N, space);
    m.p = sc.stage_in(model, (size_t)len, space);
    double *de = energy ? sc.stage(energy, (size_t)N, space, false, true) : nullptr;
    double *df = force ? sc.stage(force, (size_t)N * 3, space, false, true) : nullptr;
    double *dw = virial ? sc.stage(virial, (size_t)N * 9, space, false, true) : nullptr;
    double *dc = charge ? sc.stage(charge, (size_t)N, space, false, true) : nullptr;
    double *db = bec ? sc.stage(bec, (size_t)N * 9, space, false, true) : nullptr;
    double *dq = descriptor ? sc.stage(descriptor, (size_t)N * m.dim, space, false, true) : nullptr;
    double *dl = latent ? sc.stage(latent, (size_t)N * m.H, space, false, true) : nullptr;
    // the k-points go up first: they are pageable host memory that ends with this call, so the stream is waited for here,
    // before anything else is queued on it
    KPoint *kp = nk ? sc.stage(kpoints.data(), (size_t)nk, MDH_HOST, true, false) : sc.alloc_n<KPoint>(1);
    KIndex *kn = nk ? sc.stage(kindex.data(), (size_t)nk, MDH_HOST, true, false) : sc.alloc_n<KIndex>(1);
    if (sc.failed() || !kp || !kn)
        return sc.error();
    if (nk && hipStreamSynchronize(sc.stream()) != hipSuccess) { set_error("mdh_nep_charge: the k-points did not reach the device"); return MDH_ERR_HIP; }
    const bool pairs = df || dw;
    const size_t rows3 = (size_t)N * (size_t)std::max<int64_t>(M, 1) * 3;
    Pos4 *rec = sc.alloc_n<Pos4>((size_t)N), *xq = sc.alloc_n<Pos4>((size_t)N);
    double *FpR = sc.alloc_n<double>((size_t)N * m.NR), *FpRq = sc.alloc_n<double>((size_t)N * m.NR);
    double *A = sc.alloc_n<double>((size_t)N * m.NA * 24), *Aq = sc.alloc_n<double>((size_t)N * m.NA * 24);
    double *table = (pairs || db) ? sc.alloc_n<double>(rows3) : nullptr;
    double *q = sc.alloc_n<double>((size_t)N), *mean = sc.alloc_n<double>(1), *D = sc.alloc_n<double>((size_t)N);
    double *fc = sc.alloc_n<double>((size_t)N * 3), *vc = sc.alloc_n<double>((size_t)N * 9);
    if (!de)
        de = sc.alloc_n<double>((size_t)N);
    if (!rec || !xq || !FpR || !FpRq || !A || !Aq || ((pairs || db) && !table) || !q || !mean || !D || !fc || !vc || !de)
        return sc.error();
    hipStream_t st = sc.stream();
    nep_launch_pack(st, dx, dy, dz, dt, dmap, N, m, rec);
    const NepPassArgs pass{dv, dd, dn, N, M, b, rec, m};
    nep_launch_descriptor(st, pass, de, FpR, A, dq, dl, q, FpRq, Aq);
    hipLaunchKernelGGL(k_nepq_mean, dim3(1), dim3(256), 0, st, q, n_real, mean);
    hipLaunchKernelGGL(k_nepq_center, dim3(grid_for(N, 256)), dim3(256), 0, st, q, N, mean, rec, xq, dc);
    if (cc.mode != 3) {
        const int kblocks = std::max(1, grid_for(nk, NEPQ_TILE * NEPQ_KPL));
        // few k-points: the atoms in segments, so that about 1024 blocks run; the number follows from nk and n_real alone
        const int64_t tiles = std::max<int64_t>(1, (n_real + NEPQ_TILE - 1) / NEPQ_TILE);
        const int segments = (int)std::min<int64_t>(tiles, std::max(1, 1024 / kblocks));
        const int64_t seg_len = ((tiles + segments - 1) / segments) * NEPQ_TILE;
        // few atoms: the k-points in ranges (whole tiles), so that about 1024 blocks run; from N and nk alone
        const int ablocks = grid_for(N, 64);
        const int64_t ktiles = std::max<int64_t>(1, (nk + NEPQ_TILE - 1) / NEPQ_TILE);
        const int ranges = (int)std::min<int64_t>(ktiles, std::max(1, 1024 / ablocks));
        const int64_t klen = ((ktiles + ranges - 1) / ranges) * NEPQ_TILE;
        double *part = sc.alloc_n<double>((size_t)segments * (size_t)std::max<int64_t>(nk, 1) * 2);
        double *apart = sc.alloc_n<double>((size_t)ranges * NEPQ_SUMS * (size_t)N);
        if (!part || !apart)
            return sc.error();
        if (nk) {
            ProfRange pr("k_nepq_sfactor", st);
            hipLaunchKernelGGL(k_nepq_sfactor, dim3(kblocks, segments), dim3(NEPQ_TILE), (size_t)rb.TA * (size_t)(rb.L1 + rb.L2 + rb.L3) * 16, st,
                               xq, n_real, seg_len, kn, nk, rb, part);
            hipLaunchKernelGGL(k_nepq_sfactor_sum, dim3(grid_for(nk, 256)), dim3(256), 0, st, part, segments, nk, kp);
        }
        ProfRange pr("k_nepq_atoms", st);
        hipLaunchKernelGGL(k_nepq_atoms, dim3(ablocks, ranges), dim3(64 * NEPQ_WAVES), 0, st, xq, N, kp, kn, nk, klen, cc, rb, apart);
        hipLaunchKernelGGL(k_nepq_atoms_sum, dim3(grid_for(N, 256)), dim3(256), 0, st, apart, ranges, xq, N, de, D, fc, vc);
    }
    if (cc.mode != 2) {
        ProfRange pr("k_nepq_real", st);
        const dim3 grid(grid_for(N, 64 / NEP_GATHER_W));
        auto launch = [&](auto kernel) { hipLaunchKernelGGL(kernel, grid, dim3(64), 0, st, dv, dd, dn, N, M, b, rec, q, cc, de, D, fc, vc); };
        if (cc.mode == 3)
            b.tri ? launch(k_nepq_real<true, true>) : launch(k_nepq_real<false, true>);
        else
            b.tri ? launch(k_nepq_real<true, false>) : launch(k_nepq_real<false, false>);
    }
    if (pairs) {
        nep_launch_pair(st, pass, FpR, A, table, FpRq, Aq, D);
        nep_launch_gather(st, pass, table, df, dw, fc, vc);
        if (dsum) {
            launch_virial_sum(sc, dw, n_real, dsum);
            if (sc.failed())
                return sc.error();
        }
    }
    if (db) {
        NepPassArgs plain = pass;
        plain.m.mode = 0;  // dq / dr has no ZBL part
        nep_launch_pair(st, plain, FpRq, Aq, table, nullptr, nullptr, nullptr);
        ProfRange pr("k_nepq_bec", st);
        const dim3 grid(grid_for(N, 64 / NEP_GATHER_W));
        if (b.tri)
            hipLaunchKernelGGL(k_nepq_bec<true>, grid, dim3(64), 0, st, dv, dn, N, M, b, rec, table, q, m.p + m.o_eps, db);
        else
            hipLaunchKernelGGL(k_nepq_bec<false>, grid, dim3(64), 0, st, dv, dn, N, M, b, rec, table, q, m.p + m.o_eps, db);
    }
    return sc.finish(space);
}
}
