// bond.hip — bond-length / bond-angle histograms and the angular distribution function on gfx950.
//
// Replaces src/bond_analysis.cpp: compute_bond :8-137 and compute_adf :139-279.
//
// One kernel family serves both.  A workgroup takes a tile of centres, stages every neighbour slot of the tile in LDS once —
// its minimum-image vector x[j] - x[i] (pbc<TRI>, the very bits the reference recomputes per triplet, :90-100), its list
// distance and, for the ADF, the patterns the slot can serve as j or as k — and then spreads the (centre, p < q) slot pairs
// of the whole tile over its 256 lanes.  Counts are u32 in LDS per workgroup and u64 in HBM, so nothing wraps where the
// reference's int32 would.
//
// Angle bins are exact without a device acos: the bin of the reference, min(floor(acos(c) * 180 / PI * (1 / dtheta)), nbin-1),
// is a non-increasing step function of c, and its nbin-1 step points are found once on the host by bisection with the C
// library's acos (angle_edges below).  A triplet's bin is then the number of step points above its exact f64 cosine: a
// single-precision acosf gives a guess, and one or two exact compares against the table (in LDS) confirm or move it.  The
// guess only decides how many compares are made, never the answer.
#include "common.hpp"
#include <algorithm>
#include <cmath>
#include <cstring>
#include <map>
#include <mutex>
#include <tuple>
#include <vector>

namespace mdh {

static int g_bond_variant = 0; // test hook: 1 = every row through the wide-row path (rows of more than BA_SLOTS slots)

constexpr int BA_BLOCK = 256;
constexpr int BA_TILE = 32;         // centres per tile
constexpr int BA_SLOTS = 512;       // neighbour slots staged in LDS per workgroup (16 KiB of vectors and distances)
constexpr int BA_PAT = 32;          // ADF patterns per launch: one bit each in a u32 role mask
constexpr int BA_EDGES_LDS = 2048;  // angle step points kept in LDS (16 KiB); a finer histogram reads them from L2
constexpr int BA_HIST_LDS = 8192;   // u32 bins kept in LDS (32 KiB); larger histograms go straight to HBM

// ---- host: the step points of the reference's angle bin
static int angle_bin_host(double c, double inv_dtheta, int nbin)
{
    const double PI = 3.14159265358979323846;                 // bond_analysis.cpp:27
    const double theta = std::acos(c) * 180.0 / PI;           // :111, left to right
    const double v = std::floor(theta * inv_dtheta);          // :113
    return v < (double)(nbin - 1) ? (int)v : nbin - 1;        // :114-115
}

static int64_t order_key(double d)
{
    int64_t b;
    std::memcpy(&b, &d, 8);
    return b >= 0 ? b : -(b & INT64_MAX);
}

static double from_key(int64_t k)
{
    const int64_t b = k >= 0 ? k : ((-k) | INT64_MIN);
    double d;
    std::memcpy(&d, &b, 8);
    return d;
}

// e[k] (k = 0 .. nbin-2, ascending) = t_m for m = nbin-1-k: the smallest double c in [-1, 1] whose bin is below m.  Then
// bin(c) >= m  <=>  c < t_m, and bin(c) = #{m : c < t_m}.
static void angle_edges(int nbin, double dtheta, double *e)
{
    const double inv = 1.0 / dtheta; // :43
    for (int m = 1; m < nbin; ++m) {
        int64_t lo = order_key(-1.0), hi = order_key(1.0); // bin(1) = 0 < m
        double t;
        if (angle_bin_host(-1.0, inv, nbin) < m) {
            t = -1.0;
        } else { // bin(lo) >= m, bin(hi) < m
            while (hi - lo > 1) {
                const int64_t mid = lo + (hi - lo) / 2;
                if (angle_bin_host(from_key(mid), inv, nbin) < m) hi = mid;
                else lo = mid;
            }
            t = from_key(hi);
        }
        e[nbin - 1 - m] = t;
    }
}

// the table of (nbin, dtheta) in HBM of the current device, made once per process
static const double *device_edges(int nbin, double dtheta)
{
    static std::mutex mu;
    static std::map<std::tuple<int, int, uint64_t>, double *> cache;
    int dev = 0;
    if (hipGetDevice(&dev) != hipSuccess) return nullptr;
    uint64_t bits;
    std::memcpy(&bits, &dtheta, 8);
    const auto key = std::make_tuple(dev, nbin, bits);
    std::lock_guard<std::mutex> lk(mu);
    auto it = cache.find(key);
    if (it != cache.end()) return it->second;
    std::vector<double> e((size_t)std::max(1, nbin - 1), 2.0);
    angle_edges(nbin, dtheta, e.data());
    double *d = nullptr;
    if (hipMalloc(&d, e.size() * sizeof(double)) != hipSuccess) return nullptr;
    if (hipMemcpy(d, e.data(), e.size() * sizeof(double), hipMemcpyHostToDevice) != hipSuccess) { (void)hipFree(d); return nullptr; }
    cache[key] = d;
    return d;
}

// ---- device
struct AdfPatterns { // one launch's patterns (kernel arguments: uniform reads)
    int a[BA_PAT], b[BA_PAT], c[BA_PAT];
    double lo1[BA_PAT], hi1[BA_PAT], lo2[BA_PAT], hi2[BA_PAT];
    int n;
    unsigned both; // bit m: B != C, the pair counts in either orientation (:203-210)
};

struct BondJob {
    const double *x, *y, *z;
    const int *verlet;
    const double *dist;
    const int *nn;
    const int *type;
    int64_t N, M;
    double rc, inv_dr;         // bond: list cutoff (:61, :81, :88) and 1 / delta_r (:42)
    const double *edges;       // nbin-1 ascending angle step points (HBM)
    float guess;               // 180 / PI / delta_theta: a single-precision first guess of the bin
    int nbin, slots_cap;       // slots_cap: rows wider than this take the wide-row path
    int hsize, hist_lds, edges_lds;
    unsigned long long *out_a; // angles: nbin (bond) or npattern x nbin (ADF)
    unsigned long long *out_l; // bond lengths (bond only)
};

// (p, q), p < q, of pair l of a row of n slots: pair l sits at offset d of slot a on a circle of n slots — offsets 1 .. (n-1)/2
// for every a, and for even n the offset n/2 once (a < n/2)
template <class I>
__device__ __forceinline__ void pair_of(I l, I n, int &p, int &q)
{
    const I h = (n - 1) / 2;
    I a, d;
    if (l < n * h) { a = l / h; d = l - a * h + 1; }
    else { a = l - n * h; d = n / 2; }
    I b = a + d;
    if (b >= n) b -= n;
    p = (int)(a < b ? a : b);
    q = (int)(a < b ? b : a);
}

// bin = #{m : c < t_m} with t_m = e[nbin-1-m]; c is not NaN
__device__ __forceinline__ int angle_bin(double c, const double *e, int nbin, float guess)
{
    if (c > 1.0) c = 1.0;   // :105-108
    if (c < -1.0) c = -1.0;
    int g = (int)(acosf((float)c) * guess);
    g = g < 0 ? 0 : (g > nbin - 1 ? nbin - 1 : g);
    while (g < nbin - 1 && c < e[nbin - 2 - g]) ++g; // bin >= g + 1
    while (g > 0 && c >= e[nbin - 1 - g]) --g;       // bin < g
    return g;
}

__device__ __forceinline__ void hist_add(unsigned *lds, unsigned long long *glob, bool use_lds, int bin)
{
    if (use_lds) atomicAdd(&lds[bin], 1u);
    else atomicAdd(&glob[bin], 1ull);
}

// the neighbour in slot q of row i: its vector from i (raw positions through the minimum image, :90-100), its list distance,
// its id as the list has it, and the id that is safe to read through
template <bool TRI>
__device__ __forceinline__ void slot_vec(const BondJob &J, const DBox &b, int64_t i, int q, double &vx, double &vy, double &vz,
                                         double &r, int &j, int &js)
{
    const int64_t e = i * J.M + q;
    j = J.verlet[e];
    r = J.dist[e];
    js = safe_id(j, i, J.N);
    vx = J.x[js] - J.x[i];
    vy = J.y[js] - J.y[i];
    vz = J.z[js] - J.z[i];
    pbc<TRI>(b, vx, vy, vz);
}

// the pattern bits a slot can take as j (type B within range 1) and as k (type C within range 2) around a centre of type ti
template <bool ADF>
__device__ __forceinline__ void slot_roles(const BondJob &J, const AdfPatterns &P, int ti, int js, double r, unsigned &jm, unsigned &km)
{
    jm = km = 0u;
    if (!ADF) return;
    const int tj = J.type[js];
    for (int m = 0; m < P.n; ++m) {
        if (P.a[m] != ti) continue;                                                // :189
        if (tj == P.b[m] && r <= P.hi1[m] && r >= P.lo1[m]) jm |= 1u << m;          // :198-202
        if (tj == P.c[m] && r <= P.hi2[m] && r >= P.lo2[m]) km |= 1u << m;          // :215-219
    }
}

// one triplet: the cosine from the two vectors and the list distances (:103-104), its bin, and its counts
template <bool ADF>
__device__ __forceinline__ void count_triplet(const BondJob &J, const double *edges, unsigned *lds, bool use_lds, double px, double py,
                                              double pz, double rp, double qx, double qy, double qz, double rq, unsigned hits)
{
    const double dot = px * qx + py * qy + pz * qz;
    const double c = dot / (rp * rq);
    if (!(c == c)) return; // 0/0 of a duplicate atom: not counted
    const int bin = angle_bin(c, edges, J.nbin, J.guess);
    if (!ADF) {
        hist_add(lds, J.out_a, use_lds, bin);
        return;
    }
    while (hits) {
        const int m = __builtin_ctz(hits);
        hits &= hits - 1;
        hist_add(lds, J.out_a, use_lds, m * J.nbin + bin);
    }
}

__device__ __forceinline__ void length_count(const BondJob &J, unsigned *lds, bool use_lds, int64_t i, int j, double r)
{
    if (j > i && r <= J.rc) { // :58-63
        const double v = floor(r * J.inv_dr);
        const int bin = v < (double)(J.nbin - 1) ? (v > 0.0 ? (int)v : 0) : J.nbin - 1; // :64-66
        if (use_lds) atomicAdd(&lds[J.nbin + bin], 1u);
        else atomicAdd(&J.out_l[bin], 1ull);
    }
}

template <bool TRI, bool ADF>
__global__ __launch_bounds__(BA_BLOCK) void k_bond(BondJob J, DBox b, AdfPatterns P)
{
    __shared__ double sx[BA_SLOTS], sy[BA_SLOTS], sz[BA_SLOTS], sr[BA_SLOTS];
    __shared__ unsigned sjm[ADF ? BA_SLOTS : 1], skm[ADF ? BA_SLOTS : 1];
    __shared__ int s_n[BA_TILE], s_slot[BA_TILE + 1];
    __shared__ unsigned s_pair[BA_TILE + 1];
    extern __shared__ __attribute__((aligned(16))) unsigned char ba_dyn[]; // [edges (f64)] [histogram (u32)]
    const int t = threadIdx.x;
    double *e_lds = reinterpret_cast<double *>(ba_dyn);
    unsigned *hist = reinterpret_cast<unsigned *>(ba_dyn + (J.edges_lds ? (size_t)(J.nbin - 1) * 8 : 0));
    const bool use_lds = J.hist_lds != 0;
    if (J.edges_lds)
        for (int q = t; q < J.nbin - 1; q += BA_BLOCK) e_lds[q] = J.edges[q];
    if (use_lds)
        for (int q = t; q < J.hsize; q += BA_BLOCK) hist[q] = 0u;
    const double *edges = J.edges_lds ? e_lds : J.edges;
    const int64_t ntiles = (J.N + BA_TILE - 1) / BA_TILE;
    for (int64_t tile = blockIdx.x; tile < ntiles; tile += gridDim.x) {
        const int64_t i0 = tile * BA_TILE;
        const int nt = (int)min((int64_t)BA_TILE, J.N - i0);
        __syncthreads(); // (the previous tile is done with s_n)
        if (t < BA_TILE) {
            int n = 0;
            if (t < nt) {
                n = J.nn[i0 + t];
                n = n < 0 ? 0 : (n > J.M ? (int)J.M : n);
            }
            s_n[t] = n;
        }
        __syncthreads();
        int c0 = 0;
        while (c0 < nt) {
            // the centres c0 .. c1-1 whose slots fit in LDS together (every thread walks the same counts)
            int c1 = c0, acc = 0;
            while (c1 < nt && acc + s_n[c1] <= J.slots_cap) acc += s_n[c1++];
            if (c1 == c0) {
                // ---- a row wider than the LDS: its slots straight from HBM, every pair reading both of its slots
                const int64_t i = i0 + c0;
                const int n = s_n[c0];
                const int ti = ADF ? J.type[i] : 0;
                if (!ADF)
                    for (int q = t; q < n; q += BA_BLOCK) {
                        const int64_t e = i * J.M + q;
                        length_count(J, hist, use_lds, i, J.verlet[e], J.dist[e]);
                    }
                const int64_t npair = (int64_t)n * (n - 1) / 2;
                for (int64_t l = t; l < npair; l += BA_BLOCK) {
                    int p, q, jp, jq, jps, jqs;
                    pair_of<int64_t>(l, n, p, q);
                    double px, py, pz, rp, qx, qy, qz, rq;
                    slot_vec<TRI>(J, b, i, p, px, py, pz, rp, jp, jps);
                    slot_vec<TRI>(J, b, i, q, qx, qy, qz, rq, jq, jqs);
                    unsigned hits;
                    if (ADF) {
                        unsigned jmp, kmp, jmq, kmq;
                        slot_roles<ADF>(J, P, ti, jps, rp, jmp, kmp);
                        slot_roles<ADF>(J, P, ti, jqs, rq, jmq, kmq);
                        hits = (jmp & kmq) | (jmq & kmp & P.both);
                    } else {
                        hits = (rp <= J.rc && rq <= J.rc) ? 1u : 0u; // :81, :88
                    }
                    if (hits) count_triplet<ADF>(J, edges, hist, use_lds, px, py, pz, rp, qx, qy, qz, rq, hits);
                }
                ++c0;
                continue;
            }
            if (t == 0) { // slot and pair offsets of the centres of this round
                int s = 0;
                unsigned pr = 0;
                for (int c = c0; c < c1; ++c) {
                    s_slot[c - c0] = s;
                    s_pair[c - c0] = pr;
                    s += s_n[c];
                    pr += (unsigned)(s_n[c] * (s_n[c] - 1) / 2);
                }
                s_slot[c1 - c0] = s;
                s_pair[c1 - c0] = pr;
            }
            __syncthreads();
            const int nc = c1 - c0;
            // ---- stage the slots: vector, distance, roles; bond lengths on the way
            for (int s = t; s < acc; s += BA_BLOCK) {
                int lo = 0, hi = nc; // the centre of slot s: s_slot[lo] <= s < s_slot[lo + 1]
                while (hi - lo > 1) {
                    const int mid = (lo + hi) >> 1;
                    if (s_slot[mid] <= s) lo = mid;
                    else hi = mid;
                }
                const int64_t i = i0 + c0 + lo;
                double vx, vy, vz, r;
                int j, js;
                slot_vec<TRI>(J, b, i, s - s_slot[lo], vx, vy, vz, r, j, js);
                sx[s] = vx; sy[s] = vy; sz[s] = vz; sr[s] = r;
                if (ADF) {
                    unsigned jm, km;
                    slot_roles<ADF>(J, P, J.type[i], js, r, jm, km);
                    sjm[s] = jm; skm[s] = km;
                } else {
                    length_count(J, hist, use_lds, i, j, r);
                }
            }
            __syncthreads();
            // ---- the pairs of every centre of the round, spread over the lanes
            const unsigned npair = s_pair[nc];
            for (unsigned l = t; l < npair; l += BA_BLOCK) {
                int lo = 0, hi = nc;
                while (hi - lo > 1) {
                    const int mid = (lo + hi) >> 1;
                    if (s_pair[mid] <= l) lo = mid;
                    else hi = mid;
                }
                int p, q;
                pair_of<unsigned>(l - s_pair[lo], (unsigned)(s_slot[lo + 1] - s_slot[lo]), p, q);
                p += s_slot[lo];
                q += s_slot[lo];
                unsigned hits;
                if (ADF) hits = (sjm[p] & skm[q]) | (sjm[q] & skm[p] & P.both);
                else hits = (sr[p] <= J.rc && sr[q] <= J.rc) ? 1u : 0u;
                if (hits) count_triplet<ADF>(J, edges, hist, use_lds, sx[p], sy[p], sz[p], sr[p], sx[q], sy[q], sz[q], sr[q], hits);
            }
            __syncthreads(); // (the next round restages the slots)
            c0 = c1;
        }
    }
    if (!use_lds)
        return;
    __syncthreads();
    for (int q = t; q < J.hsize; q += BA_BLOCK) {
        const unsigned v = hist[q];
        if (!v) continue;
        if (ADF || q < J.nbin) atomicAdd(&J.out_a[q], (unsigned long long)v);
        else atomicAdd(&J.out_l[q - J.nbin], (unsigned long long)v);
    }
}

template <bool ADF>
static void launch_bond(const BondJob &J, const DBox &b, const AdfPatterns &P, hipStream_t st)
{
    const int64_t ntiles = (J.N + BA_TILE - 1) / BA_TILE;
    const unsigned blocks = (unsigned)std::min<int64_t>(ntiles, 256 * 8);
    const size_t dyn = (J.edges_lds ? (size_t)(J.nbin - 1) * 8 : 0) + (J.hist_lds ? (size_t)J.hsize * 4 : 0);
    ProfRange pr(ADF ? "k_bond<adf>" : "k_bond", st);
    if (b.tri) hipLaunchKernelGGL((k_bond<true, ADF>), dim3(blocks), dim3(BA_BLOCK), dyn, st, J, b, P);
    else hipLaunchKernelGGL((k_bond<false, ADF>), dim3(blocks), dim3(BA_BLOCK), dyn, st, J, b, P);
}

static bool finite_positive(double v) { return v > 0.0 && v < HUGE_VAL; }

} // namespace mdh

using namespace mdh;

extern "C" {

int mdh_debug_set_bond_variant(int v)
{
    if (v != 0 && v != 1) { set_error("mdh_debug_set_bond_variant: 0 or 1"); return MDH_ERR_ARG; }
    g_bond_variant = v;
    return MDH_OK;
}

int mdh_debug_angle_edges(int nbin, double delta_theta, double *out)
{
    if (nbin < 1 || !finite_positive(delta_theta) || !out) { set_error("mdh_debug_angle_edges: invalid argument"); return MDH_ERR_ARG; }
    angle_edges(nbin, delta_theta, out);
    return MDH_OK;
}

int mdh_bond_analysis(const double *x, const double *y, const double *z, int64_t N, const double *box9, const double *origin3,
                      const int *boundary3, const int *verlet, const double *dist, const int *nn, int64_t M, double delta_r,
                      double delta_theta, double rc, int nbin, unsigned long long *length_hist, unsigned long long *angle_hist,
                      int space, void *stream)
{
    if (N < 0 || M < 0 || M >= (1 << 23) || nbin < 1 || nbin > (1 << 24) || !finite_positive(delta_r) || !finite_positive(delta_theta)
        || !(rc == rc)) {
        set_error("mdh_bond_analysis: invalid argument");
        return MDH_ERR_ARG;
    }
    DBox b;
    MDH_TRY(make_box(b, box9, origin3, boundary3));
    if (N == 0 || M == 0)
        return MDH_OK;
    Scope sc(stream);
    hipStream_t st = sc.stream();
    BondJob J{};
    J.x = sc.stage_in(x, (size_t)N, space); J.y = sc.stage_in(y, (size_t)N, space); J.z = sc.stage_in(z, (size_t)N, space);
    J.verlet = sc.stage_in(verlet, (size_t)(N * M), space);
    J.dist = sc.stage_in(dist, (size_t)(N * M), space);
    J.nn = sc.stage_in(nn, (size_t)N, space);
    J.out_l = sc.stage(length_hist, (size_t)nbin, space, true, true);
    J.out_a = sc.stage(angle_hist, (size_t)nbin, space, true, true);
    if (sc.failed())
        return sc.error();
    J.edges = device_edges(nbin, delta_theta);
    if (!J.edges) { set_error("mdh_bond_analysis: angle table"); return MDH_ERR_NOMEM; }
    J.N = N; J.M = M; J.rc = rc; J.inv_dr = 1.0 / delta_r; // :42
    J.nbin = nbin;
    J.guess = (float)(180.0 / 3.14159265358979323846 / delta_theta);
    J.slots_cap = g_bond_variant == 1 ? 0 : BA_SLOTS;
    J.hsize = 2 * nbin;
    J.hist_lds = J.hsize <= BA_HIST_LDS;
    J.edges_lds = nbin - 1 <= BA_EDGES_LDS;
    AdfPatterns P{};
    launch_bond<false>(J, b, P, st);
    return sc.finish(space);
}

int mdh_angular_distribution(const double *x, const double *y, const double *z, int64_t N, const double *box9,
                             const double *origin3, const int *boundary3, const int *verlet, const double *dist, const int *nn,
                             const int *type, int64_t M, double delta_theta, const int *patterns_host, const double *ranges_host,
                             int npattern, int nbin, unsigned long long *hist, int space, void *stream)
{
    if (N < 0 || M < 0 || M >= (1 << 23) || nbin < 1 || nbin > (1 << 24) || npattern < 0 || !finite_positive(delta_theta)
        || (npattern > 0 && (!patterns_host || !ranges_host))) {
        set_error("mdh_angular_distribution: invalid argument");
        return MDH_ERR_ARG;
    }
    if ((int64_t)npattern * nbin >= ((int64_t)1 << 31)) { set_error("mdh_angular_distribution: npattern x nbin too large"); return MDH_ERR_ARG; }
    DBox b;
    MDH_TRY(make_box(b, box9, origin3, boundary3));
    if (N == 0 || M == 0 || npattern == 0)
        return MDH_OK;
    Scope sc(stream);
    hipStream_t st = sc.stream();
    BondJob J{};
    J.x = sc.stage_in(x, (size_t)N, space); J.y = sc.stage_in(y, (size_t)N, space); J.z = sc.stage_in(z, (size_t)N, space);
    J.verlet = sc.stage_in(verlet, (size_t)(N * M), space);
    J.dist = sc.stage_in(dist, (size_t)(N * M), space);
    J.nn = sc.stage_in(nn, (size_t)N, space);
    J.type = sc.stage_in(type, (size_t)N, space);
    unsigned long long *out = sc.stage(hist, (size_t)npattern * nbin, space, true, true);
    if (sc.failed())
        return sc.error();
    J.edges = device_edges(nbin, delta_theta);
    if (!J.edges) { set_error("mdh_angular_distribution: angle table"); return MDH_ERR_NOMEM; }
    J.N = N; J.M = M;
    J.nbin = nbin;
    J.guess = (float)(180.0 / 3.14159265358979323846 / delta_theta);
    J.slots_cap = g_bond_variant == 1 ? 0 : BA_SLOTS;
    J.edges_lds = nbin - 1 <= BA_EDGES_LDS;
    // patterns BA_PAT at a time: a launch per group, each with its own role masks
    for (int m0 = 0; m0 < npattern; m0 += BA_PAT) {
        AdfPatterns P{};
        P.n = std::min(BA_PAT, npattern - m0);
        for (int m = 0; m < P.n; ++m) {
            const int *pt = patterns_host + 3 * (m0 + m);
            const double *rg = ranges_host + 4 * (m0 + m);
            P.a[m] = pt[0]; P.b[m] = pt[1]; P.c[m] = pt[2];
            P.lo1[m] = rg[0]; P.hi1[m] = rg[1]; P.lo2[m] = rg[2]; P.hi2[m] = rg[3];
            if (pt[1] != pt[2]) P.both |= 1u << m;
        }
        J.hsize = P.n * nbin;
        J.hist_lds = J.hsize <= BA_HIST_LDS;
        J.out_a = out + (size_t)m0 * nbin;
        launch_bond<true>(J, b, P, st);
    }
    return sc.finish(space);
}
}

MDH_WARM_UNIT(bond)
