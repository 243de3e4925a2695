// nep.hip — neuroevolution-potential energies, forces and virials over a cutoff list, written from the model's definition
// (Fan et al., Phys. Rev. B 104, 104309; Fan et al., J. Chem. Phys. 157, 114801; Song et al., Nat. Commun. 15, 10208).
//
// Atom i of type t has the descriptor q = (q_n radial, q_n^l angular) and the energy U_t(q * scaler), a one-hidden-layer tanh
// network, plus half of every pair's ZBL energy.  With u = r_ij / d the unit vector to neighbour j and t' its type:
//   g_n(d)  = sum_k c[t][t'][n][k] f_k(d),  f_k = (T_k(x) + 1) / 2 * fc(d),  x = 2 (d / rc - 1)^2 - 1,  fc = (1 + cos(pi d / rc)) / 2,
//             rc the mean of the two types' cutoffs (radial and angular have their own c, rc and numbers of n and k)
//   q_n     = sum_j g_n(d_j)                                     over entries with d < rc_radial
//   s_nk    = sum_j g_n(d_j) b_k(u_j),  k = 0..23                over entries with d < rc_angular
//   b_k     : the real harmonics of l = 1..4 (3 + 5 + 7 + 9): p_lm(z) Re (x + i y)^m and p_lm(z) Im (x + i y)^m, p_lm the m-th
//             derivative of the Legendre polynomial P_l scaled to integer coefficients (harmonics() below)
//   q_n^l   = sum_{k in l} W_k s_nk^2 = (2l+1)/(4 pi) sum_jk g_n(d_j) g_n(d_k) P_l(cos theta_jk)         (addition theorem; NEP_W below)
//   4-body  : a cubic in the five s_nk of l = 2;  5-body: a quartic in the three of l = 1          (tables of the NEP format)
// Forces.  A_nk = dE_i / ds_nk is a per-atom quantity (pass A writes it, 24 numbers per n).  The derivative of E_i with respect
// to r_ij is
//   f_ij = sum_n Fp_n g_n'(d) u  +  sum_n [ g_n'(d) (A_n . b) u + g_n(d) / d (1 - u u^T) (A_n . grad b) ]  +  (ZBL' / 2) u
// with grad b the gradient of b_k as a polynomial in (x, y, z): its radial part drops out under the projector.  The force on i is
// sum_j (f_ij - f_ji), its virial sum_j r_ij (x) f_ji (the reference's convention: virial[j] -= r_ij (x) f_ij).
//
// Three passes, no atomics, every sum in an order that depends on the list alone — two runs give the same bits:
//   A  k_nep_descriptor  W lanes per atom, lane n owns the radial q_n and the 24 sums s_nk of ITS n (24 accumulators a lane: no
//                        scratch); the group's descriptor goes through LDS into the network, whose neurons and then whose
//                        inputs are dealt over the lanes; writes energy, Fp (radial), A, and on request descriptor and latent
//   B1 k_nep_pair        the same groups; lane n adds its n's share of f_ij, the lanes are added as a butterfly, lane 0 writes
//                        the (N, M, 3) table of pair forces
//   B2 k_nep_gather      8 lanes per atom deal the row's entries among them; each entry finds i in row j (the list names a
//                        replica's copies by their own index, so the entry is unique), reads f_ji there, and the lanes' partial
//                        force and virial are added as a butterfly
// All arithmetic is f64, product then add (-ffp-contract=off).
#include "nep_core.hpp"

namespace mdh {

// W_lm = (2l+1)/(4 pi) (2 - delta_m0) (l-m)!/(l+m)! / a_lm^2, p_lm = a_lm d^m P_l / dz^m (addition theorem of the Legendre
// polynomials); the rational factor per (l, m):
//   l = 1: 1, 1 | l = 2: 1/4, 3, 3/4 | l = 3: 1/4, 3/8, 15/4, 5/8 | l = 4: 1/64, 5/8, 5/16, 35/8, 35/64
#define NEP_N1 (3.0 / (4.0 * NEP_PI))
#define NEP_N2 (5.0 / (4.0 * NEP_PI))
#define NEP_N3 (7.0 / (4.0 * NEP_PI))
#define NEP_N4 (9.0 / (4.0 * NEP_PI))
__device__ constexpr double NEP_W[24] = {
    NEP_N1, NEP_N1, NEP_N1,
    NEP_N2 * 0.25, NEP_N2 * 3.0, NEP_N2 * 3.0, NEP_N2 * 0.75, NEP_N2 * 0.75,
    NEP_N3 * 0.25, NEP_N3 * 0.375, NEP_N3 * 0.375, NEP_N3 * 3.75, NEP_N3 * 3.75, NEP_N3 * 0.625, NEP_N3 * 0.625,
    NEP_N4 / 64.0, NEP_N4 * 0.625, NEP_N4 * 0.625, NEP_N4 * 0.3125, NEP_N4 * 0.3125, NEP_N4 * 4.375, NEP_N4 * 4.375, NEP_N4 * 35.0 / 64.0,
    NEP_N4 * 35.0 / 64.0};
// the 4-body (l = 2) and 5-body (l = 1) invariants: coefficient tables of the NEP format (GPUMD; J. Chem. Phys. 157, 114801)
__device__ constexpr double NEP_C4[5] = {-0.007499480826664, -0.134990654879954, 0.067495327439977, 0.404971964639861, -0.809943929279723};
__device__ constexpr double NEP_C5[3] = {0.026596810706114, 0.053193621412227, 0.026596810706114};
// the universal ZBL screening function (Ziegler, Biersack, Littmark), 1 / 0.46850 A, e^2 / (4 pi eps0) in eV A
__device__ constexpr double ZBL_A[4] = {0.18175, 0.50986, 0.28022, 0.02817}, ZBL_B[4] = {3.1998, 0.94229, 0.4029, 0.20162};
constexpr double ZBL_LENGTH_INV = 2.134563;

// g = sum_k c[k] f_k(d) and its derivative, d < rc
__device__ __forceinline__ void radial_function(double d, double rc, const double *__restrict__ c, int K, double &g, double &dg)
{
    const double t = d / rc;
    const double fc = 0.5 * cos(NEP_PI * t) + 0.5, dfc = -0.5 * NEP_PI * sin(NEP_PI * t) / rc;
    const double x = 2.0 * (t - 1.0) * (t - 1.0) - 1.0, dx = 4.0 * (t - 1.0) / rc;
    double T0 = 1.0, T1 = x, D0 = 0.0, D1 = 1.0;
    g = c[0] * fc;
    dg = c[0] * dfc;
    for (int k = 1; k < K; ++k) {
        const double half = (T1 + 1.0) * 0.5;
        g += c[k] * (half * fc);
        dg += c[k] * (0.5 * D1 * dx * fc + half * dfc);
        const double T2 = 2.0 * x * T1 - T0, D2 = 2.0 * T1 + 2.0 * x * D1 - D0;
        T0 = T1; T1 = T2; D0 = D1; D1 = D2;
    }
}

__device__ __forceinline__ void harmonics(double x, double y, double z, double (&b)[24])
{
    const double z2 = z * z;
    const double c2 = x * x - y * y, s2 = 2.0 * x * y, c3 = x * c2 - y * s2, s3 = x * s2 + y * c2, c4 = x * c3 - y * s3, s4 = x * s3 + y * c3;
    const double p31 = 5.0 * z2 - 1.0, p41 = (7.0 * z2 - 3.0) * z, p42 = 7.0 * z2 - 1.0;
    b[0] = z; b[1] = x; b[2] = y;
    b[3] = 3.0 * z2 - 1.0; b[4] = z * x; b[5] = z * y; b[6] = c2; b[7] = s2;
    b[8] = (5.0 * z2 - 3.0) * z; b[9] = p31 * x; b[10] = p31 * y; b[11] = z * c2; b[12] = z * s2; b[13] = c3; b[14] = s3;
    b[15] = (35.0 * z2 - 30.0) * z2 + 3.0; b[16] = p41 * x; b[17] = p41 * y; b[18] = p42 * c2; b[19] = p42 * s2; b[20] = z * c3;
    b[21] = z * s3; b[22] = c4; b[23] = s4;
}

// S = A . b and V = A . grad b.  A term p(z) C with C = Re or Im of (x + i y)^m has the gradient
// (p m Re.., -p m Im.., p' C) of the power m - 1 for the real part and (p m Im.., p m Re.., p' C) for the imaginary one.
__device__ __forceinline__ void contract(const double (&A)[24], double x, double y, double z, double &S, double (&V)[3])
{
    const double z2 = z * z;
    const double c[5] = {1.0, x, x * x - y * y, x * (x * x - y * y) - y * (2.0 * x * y), 0.0};
    const double s[5] = {0.0, y, 2.0 * x * y, x * (2.0 * x * y) + y * (x * x - y * y), 0.0};
    const double c4 = x * c[3] - y * s[3], s4 = x * s[3] + y * c[3];
    S = 0.0;
    V[0] = V[1] = V[2] = 0.0;
    auto axial = [&](double a, double p, double dp) { S += a * p; V[2] += a * dp; };
    auto pair = [&](double ac, double as, double p, double dp, int m, double cm, double sm) {
        const double pm = p * m;
        S += ac * (p * cm) + as * (p * sm);
        V[0] += ac * (pm * c[m - 1]) + as * (pm * s[m - 1]);
        V[1] += as * (pm * c[m - 1]) - ac * (pm * s[m - 1]);
        V[2] += ac * (dp * cm) + as * (dp * sm);
    };
    axial(A[0], z, 1.0);
    pair(A[1], A[2], 1.0, 0.0, 1, c[1], s[1]);
    axial(A[3], 3.0 * z2 - 1.0, 6.0 * z);
    pair(A[4], A[5], z, 1.0, 1, c[1], s[1]);
    pair(A[6], A[7], 1.0, 0.0, 2, c[2], s[2]);
    axial(A[8], (5.0 * z2 - 3.0) * z, 15.0 * z2 - 3.0);
    pair(A[9], A[10], 5.0 * z2 - 1.0, 10.0 * z, 1, c[1], s[1]);
    pair(A[11], A[12], z, 1.0, 2, c[2], s[2]);
    pair(A[13], A[14], 1.0, 0.0, 3, c[3], s[3]);
    axial(A[15], (35.0 * z2 - 30.0) * z2 + 3.0, (140.0 * z2 - 60.0) * z);
    pair(A[16], A[17], (7.0 * z2 - 3.0) * z, 21.0 * z2 - 3.0, 1, c[1], s[1]);
    pair(A[18], A[19], 7.0 * z2 - 1.0, 14.0 * z, 2, c[2], s[2]);
    pair(A[20], A[21], z, 1.0, 3, c[3], s[3]);
    pair(A[22], A[23], 1.0, 0.0, 4, c4, s4);
}

// the pair's ZBL energy e and its derivative de with respect to d; zero from the outer radius on
__device__ __forceinline__ bool zbl_pair(const NepModel &m, int ti, int tj, double d, double &e, double &de)
{
    double lo = m.zbl_inner, hi = m.zbl_outer;
    if (m.mode == 2) {
        lo = 0.0;
        hi = fmin(m.zbl_factor * (m.p[m.o_rcov + ti] + m.p[m.o_rcov + tj]), hi);
    }
    if (!(d < hi))
        return false;
    const double zi = m.p[m.o_z + ti], zj = m.p[m.o_z + tj];
    const double a_inv = (pow(zi, 0.23) + pow(zj, 0.23)) * ZBL_LENGTH_INV, xs = d * a_inv;
    double phi = 0.0, dphi = 0.0;
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        const double term = ZBL_A[k] * exp(-ZBL_B[k] * xs);
        phi += term;
        dphi -= ZBL_B[k] * term;
    }
    dphi *= a_inv;
    const double kq = NEP_COULOMB * zi * zj;
    const double e0 = kq * phi / d, de0 = kq * (dphi / d - phi / (d * d));
    double fc = 1.0, dfc = 0.0;
    if (d >= lo) {
        const double span = NEP_PI / (hi - lo);
        fc = 0.5 * cos(span * (d - lo)) + 0.5;
        dfc = -0.5 * span * sin(span * (d - lo));
    }
    e = e0 * fc;
    de = de0 * fc + e0 * dfc;
    return true;
}

// positions and the model's own type of every atom as one 32-byte record (w = the type, -1: none)
__global__ __launch_bounds__(256) void k_nep_pack(const double *__restrict__ x, const double *__restrict__ y, const double *__restrict__ z,
                                                  const int *__restrict__ type, NepTypeMap map, int nfile, int T, int64_t N,
                                                  Pos4 *__restrict__ out)
{
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= N)
        return;
    const int t = type[i];
    int local = (unsigned)t < (unsigned)nfile ? map.local[t] : -1;
    if ((unsigned)local >= (unsigned)T)
        local = -1;
    out[i] = Pos4{x[i], y[i], z[i], (double)local};
}

// A_nk = dU / ds_nk of one lane's n from the group's Fp row (in LDS) and the lane's sums s; 24 numbers to out
__device__ __forceinline__ void nep_write_A(const double (&s)[24], const double *__restrict__ fp_row, const NepModel &m, int lane, bool mine,
                                            double *__restrict__ out)
{
    double A[24];
    int first = 0;
#pragma unroll
    for (int k = 0; k < 24; ++k) A[k] = 0.0;
    for (int l = 1; l <= m.L3; ++l) {
        const double fp = 2.0 * fp_row[m.NR + (l - 1) * m.NA + lane];
#pragma unroll
        for (int k = 0; k < 24; ++k)
            if (k >= first && k < first + 2 * l + 1) A[k] = fp * (NEP_W[k] * s[k]);
        first += 2 * l + 1;
    }
    int order = m.L3;
    if (m.L4 == 2) {
        const double F = fp_row[m.NR + order * m.NA + lane];
        A[3] += F * (3.0 * NEP_C4[0] * s[3] * s[3] + NEP_C4[1] * (s[4] * s[4] + s[5] * s[5]) + NEP_C4[2] * (s[6] * s[6] + s[7] * s[7]));
        A[4] += F * (2.0 * NEP_C4[1] * s[3] * s[4] - 2.0 * NEP_C4[3] * s[6] * s[4] + NEP_C4[4] * s[5] * s[7]);
        A[5] += F * (2.0 * NEP_C4[1] * s[3] * s[5] + 2.0 * NEP_C4[3] * s[6] * s[5] + NEP_C4[4] * s[4] * s[7]);
        A[6] += F * (2.0 * NEP_C4[2] * s[3] * s[6] + NEP_C4[3] * (s[5] * s[5] - s[4] * s[4]));
        A[7] += F * (2.0 * NEP_C4[2] * s[3] * s[7] + NEP_C4[4] * s[4] * s[5]);
        ++order;
    }
    if (m.L5 == 1) {
        const double F = fp_row[m.NR + order * m.NA + lane];
        const double pp = s[1] * s[1] + s[2] * s[2], s0 = s[0] * s[0];
        A[0] += F * (4.0 * NEP_C5[0] * s0 * s[0] + 2.0 * NEP_C5[1] * s[0] * pp);
        A[1] += F * (2.0 * NEP_C5[1] * s0 * s[1] + 4.0 * NEP_C5[2] * pp * s[1]);
        A[2] += F * (2.0 * NEP_C5[1] * s0 * s[2] + 4.0 * NEP_C5[2] * pp * s[2]);
    }
#pragma unroll
    for (int k = 0; k < 24; ++k) out[k] = mine ? A[k] : 0.0;
}

// Q: a charge model — the network's second output (charge, before the frame's mean is removed) and its derivatives FpRq, Aq, the
// twins of FpR and Aout.  A is linear in Fp, so the two sets are written one after the other from the same 24 sums.
template <int W, bool TRI, bool Q>
__global__ __launch_bounds__(64) void k_nep_descriptor(const int *__restrict__ verlet, const double *__restrict__ dist, const int *__restrict__ nn,
                                                       int64_t N, int64_t M, DBox b, const Pos4 *__restrict__ rec, NepModel m,
                                                       double *__restrict__ energy, double *__restrict__ FpR, double *__restrict__ Aout,
                                                       double *__restrict__ descriptor, double *__restrict__ latent,
                                                       double *__restrict__ charge, double *__restrict__ FpRq, double *__restrict__ Aq)
{
    constexpr int G = 64 / W;
    __shared__ double sq[G][NEP_MAX_DIM];
    __shared__ double lat[G][NEP_MAX_NEURON];
    __shared__ double slope[G][NEP_MAX_NEURON];
    __shared__ double hidden[Q ? G : 1][Q ? NEP_MAX_NEURON : 1];  // tanh(..): the charge's output and slope follow from it
    double(*sqq)[NEP_MAX_NEURON] = lat;  // Fp_q takes the latent space's place once that is written out (dim <= 112 < 128)
    const int lane = threadIdx.x % W, grp = threadIdx.x / W;
    const int64_t i = (int64_t)blockIdx.x * G + grp;
    const bool on = i < N;
    const Pos4 ri = rec[on ? i : 0];
    const int ti = on ? (int)ri.w : -1;
    const bool mine = ti >= 0;
    const int n = mine ? min(max(nn[i], 0), (int)M) : 0;
    const bool radial = lane < m.NR, angular = lane < m.NA;
    double qr = 0.0, ez = 0.0;
    double s[24];
#pragma unroll
    for (int k = 0; k < 24; ++k) s[k] = 0.0;
    for (int slot = 0; slot < n; ++slot) {
        const int j = verlet[i * M + slot];
        if ((unsigned)j >= (unsigned)N)
            continue;
        const Pos4 rj = rec[j];
        const int tj = (int)rj.w;
        if (tj < 0)
            continue;
        const double d = dist[i * M + slot];
        const double rc_r = 0.5 * (m.p[m.o_rc_r + ti] + m.p[m.o_rc_r + tj]), rc_a = 0.5 * (m.p[m.o_rc_a + ti] + m.p[m.o_rc_a + tj]);
        const int pair = ti * m.T + tj;
        if (radial && d < rc_r) {
            double g, dg;
            radial_function(d, rc_r, m.p + m.o_cr + ((int64_t)pair * m.NR + lane) * m.KR, m.KR, g, dg);
            qr += g;
        }
        if (!(d < rc_a))
            continue;
        if (angular) {
            double dx = rj.x - ri.x, dy = rj.y - ri.y, dz = rj.z - ri.z;
            nep_image<TRI>(b, dx, dy, dz);
            double g, dg, h[24];
            radial_function(d, rc_a, m.p + m.o_ca + ((int64_t)pair * m.NA + lane) * m.KA, m.KA, g, dg);
            harmonics(dx / d, dy / d, dz / d, h);
#pragma unroll
            for (int k = 0; k < 24; ++k) s[k] += g * h[k];
        }
        if (m.mode && lane == 0) {
            double e, de;
            if (zbl_pair(m, ti, tj, d, e, de))
                ez += 0.5 * e;
        }
    }
    // the invariants of this lane's n, scaled, into the group's descriptor
    const double *scaler = m.p + m.o_scaler;
    if (radial)
        sq[grp][lane] = qr * scaler[lane];
    if (angular) {
        int first = 0;
        for (int l = 1; l <= m.L3; ++l) {
            double q = 0.0;
#pragma unroll
            for (int k = 0; k < 24; ++k)
                if (k >= first && k < first + 2 * l + 1) q += NEP_W[k] * (s[k] * s[k]);
            first += 2 * l + 1;
            const int at = m.NR + (l - 1) * m.NA + lane;
            sq[grp][at] = q * scaler[at];
        }
        int order = m.L3;
        if (m.L4 == 2) {
            const double q = NEP_C4[0] * s[3] * s[3] * s[3] + NEP_C4[1] * s[3] * (s[4] * s[4] + s[5] * s[5]) + NEP_C4[2] * s[3] * (s[6] * s[6] + s[7] * s[7])
                             + NEP_C4[3] * s[6] * (s[5] * s[5] - s[4] * s[4]) + NEP_C4[4] * s[4] * s[5] * s[7];
            const int at = m.NR + order * m.NA + lane;
            sq[grp][at] = q * scaler[at];
            ++order;
        }
        if (m.L5 == 1) {
            const double pp = s[1] * s[1] + s[2] * s[2], s0 = s[0] * s[0];
            const double q = NEP_C5[0] * s0 * s0 + NEP_C5[1] * s0 * pp + NEP_C5[2] * pp * pp;
            const int at = m.NR + order * m.NA + lane;
            sq[grp][at] = q * scaler[at];
        }
    }
    __syncthreads();
    if (descriptor && on)
        for (int d = lane; d < m.dim; d += W) descriptor[i * m.dim + d] = mine ? sq[grp][d] : 0.0;
    // the network of the atom's type: the neurons dealt over the lanes
    const double *net = m.p + m.o_net + (int64_t)(mine ? ti : 0) * m.net_stride;
    const double *w0 = net, *b0 = net + (int64_t)m.H * m.dim, *w1 = b0 + m.H, *w1q = w1 + m.H, *bias = w1 + (Q ? 2 : 1) * m.H;
    for (int h = lane; h < m.H; h += W) {
        double dot = 0.0;
        for (int d = 0; d < m.dim; ++d) dot += w0[h * m.dim + d] * sq[grp][d];
        const double x = tanh(dot - b0[h]);
        lat[grp][h] = w1[h] * x;
        slope[grp][h] = w1[h] * (1.0 - x * x);
        if (Q)
            hidden[grp][h] = x;
    }
    __syncthreads();
    if (latent && on)
        for (int h = lane; h < m.H; h += W) latent[i * m.H + h] = mine ? lat[grp][h] : 0.0;
    if (energy && on && lane == 0) {
        double e = 0.0;
        for (int h = 0; h < m.H; ++h) e += lat[grp][h];
        energy[i] = mine ? ((e - m.p[m.o_b1]) - bias[0]) + ez : 0.0;
    }
    if (Q && charge && on && lane == 0) {
        double q = 0.0;
        for (int h = 0; h < m.H; ++h) q += w1q[h] * hidden[grp][h];
        charge[i] = mine ? q : 0.0;
    }
    if (Q)
        __syncthreads();
    // Fp_d = dU / dq_d * scaler_d, the inputs dealt over the lanes; they take the descriptor's place in LDS
    for (int d = lane; d < m.dim; d += W) {
        double fp = 0.0;
        for (int h = 0; h < m.H; ++h) fp += slope[grp][h] * w0[h * m.dim + d];
        sq[grp][d] = fp * scaler[d];
        if (Q) {
            double fq = 0.0;
            for (int h = 0; h < m.H; ++h) fq += (w1q[h] * (1.0 - hidden[grp][h] * hidden[grp][h])) * w0[h * m.dim + d];
            sqq[grp][d] = fq * scaler[d];
        }
    }
    __syncthreads();
    if (!on || !Aout)
        return;
    if (radial) {
        FpR[i * m.NR + lane] = mine ? sq[grp][lane] : 0.0;
        if (Q)
            FpRq[i * m.NR + lane] = mine ? sqq[grp][lane] : 0.0;
    }
    if (angular) {
        nep_write_A(s, sq[grp], m, lane, mine, Aout + (i * m.NA + lane) * 24);
        if (Q)
            nep_write_A(s, sqq[grp], m, lane, mine, Aq + (i * m.NA + lane) * 24);
    }
}

// Q: a charge model's forces — Fp_E + D_i Fp_q and A_E + D_i A_q take the place of Fp and A (D_i: the derivative of the
// electrostatic energy with respect to the charge of atom i)
template <int W, bool TRI, bool Q>
__global__ __launch_bounds__(64) void k_nep_pair(const int *__restrict__ verlet, const double *__restrict__ dist, const int *__restrict__ nn,
                                                 int64_t N, int64_t M, DBox b, const Pos4 *__restrict__ rec, NepModel m,
                                                 const double *__restrict__ FpR, const double *__restrict__ Ain, double *__restrict__ table,
                                                 const double *__restrict__ FpRq, const double *__restrict__ Aq, const double *__restrict__ D)
{
    constexpr int G = 64 / W;
    const int lane = threadIdx.x % W, grp = threadIdx.x / W;
    const int64_t i = (int64_t)blockIdx.x * G + grp;
    const bool on = i < N;  // (a group's lanes agree on everything that decides a branch around a shuffle)
    const Pos4 ri = rec[on ? i : 0];
    const int ti = on ? (int)ri.w : -1;
    const int n = on ? min(max(nn[i], 0), (int)M) : 0;
    const bool radial = lane < m.NR, angular = lane < m.NA;
    double fpr = (on && radial) ? FpR[i * m.NR + lane] : 0.0;
    double A[24];
#pragma unroll
    for (int k = 0; k < 24; ++k) A[k] = (on && angular) ? Ain[(i * m.NA + lane) * 24 + k] : 0.0;
    if (Q) {
        const double Di = on ? D[i] : 0.0;
        if (on && radial)
            fpr += Di * FpRq[i * m.NR + lane];
        if (on && angular) {
#pragma unroll
            for (int k = 0; k < 24; ++k) A[k] += Di * Aq[(i * m.NA + lane) * 24 + k];
        }
    }
    // every group of the wave takes the same number of turns, so that the shuffles meet whole waves
    int turns = n;
#pragma unroll
    for (int step = W; step < 64; step <<= 1) turns = max(turns, __shfl_xor(turns, step, 64));
    for (int slot = 0; slot < turns; ++slot) {
        double f[3] = {0.0, 0.0, 0.0};
        const bool live = slot < n;
        const int j = live ? verlet[i * M + slot] : -1;
        if (ti >= 0 && (unsigned)j < (unsigned)N) {
            const Pos4 rj = rec[j];
            const int tj = (int)rj.w;
            const double d = dist[i * M + slot];
            if (tj >= 0) {
                const double rc_r = 0.5 * (m.p[m.o_rc_r + ti] + m.p[m.o_rc_r + tj]), rc_a = 0.5 * (m.p[m.o_rc_a + ti] + m.p[m.o_rc_a + tj]);
                if (d < rc_r || d < rc_a) {
                    double dx = rj.x - ri.x, dy = rj.y - ri.y, dz = rj.z - ri.z;
                    nep_image<TRI>(b, dx, dy, dz);
                    const double u[3] = {dx / d, dy / d, dz / d};
                    const int pair = ti * m.T + tj;
                    if (radial && d < rc_r) {
                        double g, dg;
                        radial_function(d, rc_r, m.p + m.o_cr + ((int64_t)pair * m.NR + lane) * m.KR, m.KR, g, dg);
                        const double along = fpr * dg;
#pragma unroll
                        for (int a = 0; a < 3; ++a) f[a] += along * u[a];
                    }
                    if (d < rc_a) {
                        if (angular) {
                            double g, dg, S, V[3];
                            radial_function(d, rc_a, m.p + m.o_ca + ((int64_t)pair * m.NA + lane) * m.KA, m.KA, g, dg);
                            contract(A, u[0], u[1], u[2], S, V);
                            const double uv = (u[0] * V[0] + u[1] * V[1]) + u[2] * V[2];
                            const double along = dg * S, across = g / d;
#pragma unroll
                            for (int a = 0; a < 3; ++a) f[a] += along * u[a] + across * (V[a] - u[a] * uv);
                        }
                        if (m.mode && lane == 0) {
                            double e, de;
                            if (zbl_pair(m, ti, tj, d, e, de)) {
#pragma unroll
                                for (int a = 0; a < 3; ++a) f[a] += (0.5 * de) * u[a];
                            }
                        }
                    }
                }
            }
        }
#pragma unroll
        for (int a = 0; a < 3; ++a) f[a] = group_sum<W>(f[a]);
        if (live && lane < 3)
            table[(i * M + slot) * 3 + lane] = lane == 0 ? f[0] : (lane == 1 ? f[1] : f[2]);
    }
}

// ADD: the force and the virial start from addf, addv (a charge model's electrostatic part) instead of zero
template <bool TRI, bool ADD>
__global__ __launch_bounds__(64) void k_nep_gather(const int *__restrict__ verlet, const int *__restrict__ nn, int64_t N, int64_t M, DBox b,
                                                   const Pos4 *__restrict__ rec, const double *__restrict__ table, double *__restrict__ force,
                                                   double *__restrict__ virial, const double *__restrict__ addf, const double *__restrict__ addv)
{
    constexpr int W = NEP_GATHER_W, G = 64 / W;
    const int lane = threadIdx.x % W, grp = threadIdx.x / W;
    const int64_t i = (int64_t)blockIdx.x * G + grp;
    const bool on = i < N;
    const Pos4 ri = rec[on ? i : 0];
    const int n = (on && ri.w >= 0.0) ? min(max(nn[i], 0), (int)M) : 0;
    double f[3] = {0.0, 0.0, 0.0};
    double v[9] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
    for (int slot = lane; slot < n; slot += W) {
        const int j = verlet[i * M + slot];
        if ((unsigned)j >= (unsigned)N)
            continue;
        const Pos4 rj = rec[j];
        if (rj.w < 0.0)
            continue;
        double d[3] = {rj.x - ri.x, rj.y - ri.y, rj.z - ri.z};
        nep_image<TRI>(b, d[0], d[1], d[2]);
        // where row j names i: its pair force on the way back
        const int back = nep_back(verlet, nn, M, j, i);
        const double *mine = table + (i * M + slot) * 3;
        double other[3] = {0.0, 0.0, 0.0};
        if (back >= 0) {
            const double *theirs = table + ((int64_t)j * M + back) * 3;
            other[0] = theirs[0]; other[1] = theirs[1]; other[2] = theirs[2];
        }
#pragma unroll
        for (int a = 0; a < 3; ++a) f[a] += mine[a] - other[a];
#pragma unroll
        for (int a = 0; a < 3; ++a)
#pragma unroll
            for (int c = 0; c < 3; ++c) v[3 * a + c] += d[a] * other[c];
    }
#pragma unroll
    for (int a = 0; a < 3; ++a) f[a] = group_sum<W>(f[a]);
#pragma unroll
    for (int a = 0; a < 9; ++a) v[a] = group_sum<W>(v[a]);
    if (!on || lane != 0)
        return;
    if (force) {
#pragma unroll
        for (int a = 0; a < 3; ++a) force[3 * i + a] = ADD ? addf[3 * i + a] + f[a] : f[a];
    }
    if (virial) {
#pragma unroll
        for (int a = 0; a < 9; ++a) virial[9 * i + a] = ADD ? addv[9 * i + a] + v[a] : v[a];
    }
}

// ---------------------------------------------------------------------------------------------- host side, shared by the two entries (nep_core.hpp declares it)
// the header words -> the model's shape and the offsets into its block (m.p is left alone); len: the block's length.
// charge: the entry reads a charge model (w1 of 2 x neurons per type, sqrt(epsilon_inf) before the common bias).
// -> MDH_OK, or MDH_ERR_ARG with the error set
int nep_model_of(const std::string &who, const int *h, int nfile, const double *zbl3_host, const int *type_map_host, bool charge,
                        NepModel &m, int64_t &len)
{
    m.T = h[0]; m.NR = h[1]; m.KR = h[2]; m.NA = h[3]; m.KA = h[4]; m.L3 = h[5]; m.L4 = h[6]; m.L5 = h[7]; m.H = h[8]; m.mode = h[9];
    m.nfile = nfile;
    m.charge = charge ? h[11] : 0;
    if (m.L3 < 1 || m.L3 > 4 || (m.L4 != 0 && m.L4 != 2) || (m.L5 != 0 && m.L5 != 1) || (m.L4 == 2 && m.L3 < 2)) {
        set_error(who + ": l_max out of scope (3-body 1..4, 4-body 0 or 2, 5-body 0 or 1)");
        return MDH_ERR_ARG;
    }
    if (m.T < 1 || m.T > NEP_MAX_FILE_TYPES || nfile < 1 || nfile > NEP_MAX_FILE_TYPES || m.NR < 1 || m.NR > NEP_MAX_N || m.NA < 1 ||
        m.NA > NEP_MAX_N || m.KR < 1 || m.KR > NEP_MAX_K || m.KA < 1 || m.KA > NEP_MAX_K || m.H < 1 || m.H > NEP_MAX_NEURON || m.mode < 0 ||
        m.mode > 2) {
        set_error(who + ": the model is larger than the compiled maxima (96 types, n_max 15, basis_size 16, 128 neurons, descriptor dimension 112)");
        return MDH_ERR_ARG;
    }
    if (charge && (m.charge < 1 || m.charge > 3)) {
        set_error(who + ": charge mode outside 1..3");
        return MDH_ERR_ARG;
    }
    m.dim = m.NR + m.NA * (m.L3 + (m.L4 == 2) + (m.L5 == 1));
    int64_t at = 0;
    m.o_rc_r = (int)at; at += m.T;
    m.o_rc_a = (int)at; at += m.T;
    m.o_z = (int)at; at += m.T;
    m.o_rcov = (int)at; at += m.T;
    m.o_scaler = (int)at; at += m.dim;
    m.o_cr = (int)at; at += (int64_t)m.T * m.T * m.NR * m.KR;
    m.o_ca = (int)at; at += (int64_t)m.T * m.T * m.NA * m.KA;
    m.o_net = (int)at;
    m.net_stride = m.H * (m.dim + (charge ? 3 : 2)) + 1;
    at += (int64_t)m.T * m.net_stride;
    m.o_eps = (int)at; at += charge ? 1 : 0;
    m.o_b1 = (int)at; at += 1;
    len = at;
    if (at != (int64_t)h[10]) { set_error(who + ": the model block's length does not belong to its header"); return MDH_ERR_ARG; }
    m.zbl_inner = zbl3_host[0]; m.zbl_outer = zbl3_host[1]; m.zbl_factor = zbl3_host[2];
    if (m.mode && !(m.zbl_outer > 0.0 && m.zbl_inner >= 0.0 && m.zbl_inner < m.zbl_outer)) {
        set_error(who + ": ZBL needs 0 <= inner < outer");
        return MDH_ERR_ARG;
    }
    for (int t = 0; t < nfile; ++t)
        if (type_map_host[t] < -1 || type_map_host[t] >= m.T) { set_error(who + ": a type map entry outside [-1, T)"); return MDH_ERR_ARG; }
    return MDH_OK;
}

void nep_launch_pack(hipStream_t st, const double *x, const double *y, const double *z, const int *type, const NepTypeMap &map, int64_t N,
                     const NepModel &m, Pos4 *rec)
{
    hipLaunchKernelGGL(k_nep_pack, dim3(grid_for(N, 256)), dim3(256), 0, st, x, y, z, type, map, m.nfile, m.T, N, rec);
}

template <bool Q>
static void launch_descriptor(hipStream_t st, const NepPassArgs &a, double *energy, double *FpR, double *A, double *descriptor, double *latent,
                              double *charge, double *FpRq, double *Aq)
{
    auto launch = [&](auto kernel, int atoms) {
        hipLaunchKernelGGL(kernel, dim3(grid_for(a.N, atoms)), dim3(64), 0, st, a.verlet, a.dist, a.nn, a.N, a.M, a.b, a.rec, a.m, energy, FpR, A,
                           descriptor, latent, charge, FpRq, Aq);
    };
    if (a.wide())
        a.b.tri ? launch(k_nep_descriptor<16, true, Q>, 4) : launch(k_nep_descriptor<16, false, Q>, 4);
    else
        a.b.tri ? launch(k_nep_descriptor<8, true, Q>, 8) : launch(k_nep_descriptor<8, false, Q>, 8);
}

void nep_launch_descriptor(hipStream_t st, const NepPassArgs &a, double *energy, double *FpR, double *A, double *descriptor, double *latent,
                           double *charge, double *FpRq, double *Aq)
{
    ProfRange pr("k_nep_descriptor", st);
    if (charge)
        launch_descriptor<true>(st, a, energy, FpR, A, descriptor, latent, charge, FpRq, Aq);
    else
        launch_descriptor<false>(st, a, energy, FpR, A, descriptor, latent, nullptr, nullptr, nullptr);
}

template <bool Q>
static void launch_pair(hipStream_t st, const NepPassArgs &a, const double *FpR, const double *A, double *table, const double *FpRq,
                        const double *Aq, const double *D)
{
    auto launch = [&](auto kernel, int atoms) {
        hipLaunchKernelGGL(kernel, dim3(grid_for(a.N, atoms)), dim3(64), 0, st, a.verlet, a.dist, a.nn, a.N, a.M, a.b, a.rec, a.m, FpR, A, table,
                           FpRq, Aq, D);
    };
    if (a.wide())
        a.b.tri ? launch(k_nep_pair<16, true, Q>, 4) : launch(k_nep_pair<16, false, Q>, 4);
    else
        a.b.tri ? launch(k_nep_pair<8, true, Q>, 8) : launch(k_nep_pair<8, false, Q>, 8);
}

void nep_launch_pair(hipStream_t st, const NepPassArgs &a, const double *FpR, const double *A, double *table, const double *FpRq, const double *Aq,
                     const double *D)
{
    ProfRange pr("k_nep_pair", st);
    if (D)
        launch_pair<true>(st, a, FpR, A, table, FpRq, Aq, D);
    else
        launch_pair<false>(st, a, FpR, A, table, nullptr, nullptr, nullptr);
}

template <bool ADD>
static void launch_gather(hipStream_t st, const NepPassArgs &a, const double *table, double *force, double *virial, const double *addf,
                          const double *addv)
{
    const dim3 grid(grid_for(a.N, 64 / NEP_GATHER_W));
    if (a.b.tri)
        hipLaunchKernelGGL((k_nep_gather<true, ADD>), grid, dim3(64), 0, st, a.verlet, a.nn, a.N, a.M, a.b, a.rec, table, force, virial, addf, addv);
    else
        hipLaunchKernelGGL((k_nep_gather<false, ADD>), grid, dim3(64), 0, st, a.verlet, a.nn, a.N, a.M, a.b, a.rec, table, force, virial, addf, addv);
}

void nep_launch_gather(hipStream_t st, const NepPassArgs &a, const double *table, double *force, double *virial, const double *addf,
                       const double *addv)
{
    ProfRange pr("k_nep_gather", st);
    if (addf)
        launch_gather<true>(st, a, table, force, virial, addf, addv);
    else
        launch_gather<false>(st, a, table, force, virial, nullptr, nullptr);
}

} // namespace mdh

using namespace mdh;

extern "C" {

int mdh_nep(const double *x, const double *y, const double *z, const int *type, int64_t N, const int *type_map_host, int nfile,
            const double *box9, const double *origin3, const int *boundary3, const int *verlet, const double *dist, const int *nn, int64_t M,
            const double *model, const int *head12_host, const double *zbl3_host, int64_t n_real, double *energy, double *force, double *virial,
            double *virial_sum9, double *descriptor, double *latent, int space, void *stream)
{
    if (N < 0 || M < 0 || N >= ((int64_t)1 << 31) || M >= (1 << 23)) { set_error("mdh_nep: invalid list shape"); return MDH_ERR_ARG; }
    if (!head12_host || !zbl3_host || !type_map_host) { set_error("mdh_nep: the model's header, ZBL numbers and type map are required"); return MDH_ERR_ARG; }
    if (n_real < 0 || n_real > N) { set_error("mdh_nep: n_real outside [0, N]"); return MDH_ERR_ARG; }
    if (virial_sum9 && !virial) { set_error("mdh_nep: virial_sum9 needs virial"); return MDH_ERR_ARG; }
    NepModel m;
    int64_t at = 0;
    MDH_TRY(nep_model_of("mdh_nep", head12_host, nfile, zbl3_host, type_map_host, false, m, at));
    if (space == MDH_HOST && type)
        for (int64_t i = 0; i < N; ++i)
            if (type[i] < 0 || type[i] >= nfile) { set_error("mdh_nep: an atom's type outside the type map"); return MDH_ERR_ARG; }
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
    NepTypeMap dmap;
    for (int t = 0; t < NEP_MAX_FILE_TYPES; ++t) dmap.local[t] = (signed char)(t < nfile ? type_map_host[t] : -1);
    const int *dv = M ? sc.stage_in(verlet, (size_t)(N * M), space) : nullptr;
    const double *dd = M ? sc.stage_in(dist, (size_t)(N * M), space) : nullptr;
    const int *dn = sc.stage_in(nn, (size_t)N, space);
    m.p = sc.stage_in(model, (size_t)at, space);
    double *de = energy ? sc.stage(energy, (size_t)N, space, false, true) : nullptr;
    double *df = force ? sc.stage(force, (size_t)N * 3, space, false, true) : nullptr;
    double *dw = virial ? sc.stage(virial, (size_t)N * 9, space, false, true) : nullptr;
    double *dq = descriptor ? sc.stage(descriptor, (size_t)N * m.dim, space, false, true) : nullptr;
    double *dl = latent ? sc.stage(latent, (size_t)N * m.H, space, false, true) : nullptr;
    if (sc.failed())
        return sc.error();
    const bool pairs = df || dw;
    Pos4 *rec = sc.alloc_n<Pos4>((size_t)N);
    double *FpR = pairs ? sc.alloc_n<double>((size_t)N * m.NR) : nullptr;
    double *A = pairs ? sc.alloc_n<double>((size_t)N * m.NA * 24) : nullptr;
    double *table = pairs ? sc.alloc_n<double>((size_t)N * (size_t)std::max<int64_t>(M, 1) * 3) : nullptr;
    if (!rec || (pairs && (!FpR || !A || !table)))
        return sc.error();
    hipStream_t st = sc.stream();
    nep_launch_pack(st, dx, dy, dz, dt, dmap, N, m, rec);
    const NepPassArgs pass{dv, dd, dn, N, M, b, rec, m};
    nep_launch_descriptor(st, pass, de, FpR, A, dq, dl, nullptr, nullptr, nullptr);
    if (pairs) {
        nep_launch_pair(st, pass, FpR, A, table, nullptr, nullptr, nullptr);
        nep_launch_gather(st, pass, table, df, dw, nullptr, nullptr);
        if (dsum) {
            launch_virial_sum(sc, dw, n_real, dsum);
            if (sc.failed())
                return sc.error();
        }
    }
    return sc.finish(space);
}
}
