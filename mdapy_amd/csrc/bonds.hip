// bonds.hip — bond pairs and molecule compositions (src/build_bond.cpp, System.create_bonds src/mdapy/system.py:1333-1412,
// System.cal_chemical_species :2575-2740).  DESIGN.md 5k.
//
// mdh_build_bond turns a cutoff list into the ordered (Nbond, 2) list of bonded pairs: a count pass, exclusive_scan_u32 over the
// per-row counts, a write pass.  A pair's slot is its row's prefix sum plus its rank inside the row, never a counter that hands
// out slots as threads arrive; the compositions are integer sums.  The same input gives the same bits on every run.
#include "grid.hpp"
#include <cmath>

namespace mdh {

struct BondList {
    const int *verlet;
    const double *dist;
    const int *nn;
    const int *type;      // (N) compact, or nullptr: every atom is type 0
    const double *cutoff; // (ntype, ntype), device memory
    int64_t N, M, n_real;
    int ntype;
};

// THE predicate, used by the count pass and by the write pass: does slot q of row i, which holds (j, d), list a bond, and under
// which key.  build_bond.cpp:43-56 — j > i, both types inside the matrix, dist <= cutoff (a tie is a bond); an index outside the
// list (the reference would read types[j] out of bounds) is no bond.  n_real > 0: the key is the atom that replica atom j copies,
// j % n_real, and it is the key that has to exceed i; the type is that of the replica atom itself.  Written without branches —
// the two dependent loads (the neighbour's type, its pair's cutoff) go to index 0 where the slot is out — so that the loads of
// several rows can be in flight together.
__device__ __forceinline__ bool bond_test(const BondList &a, int64_t i, int n, int ti, int64_t q, int j, double d, int &key)
{
    const bool inside = q < n && (unsigned)j < (unsigned)a.N;
    const int js = inside ? j : 0;
    const int tj = a.type ? a.type[js] : 0;
    const int k = a.n_real ? js % (int)a.n_real : js; // (n_real <= N < 2^31)
    const bool typed = (unsigned)ti < (unsigned)a.ntype && (unsigned)tj < (unsigned)a.ntype;
    const double limit = a.cutoff[typed ? (int64_t)ti * a.ntype + tj : 0];
    const bool pair = inside && typed && k > i;
    key = pair ? k : 0x7fffffff;
    return pair && d <= limit;
}

// Two things are settled across the lanes that hold a row, both by walking the set bits of a ballot and broadcasting that lane's
// key (__shfl), so their cost follows the bonds of a row and not its width:
//   first   a qualifying slot counts once: it is dropped when an earlier slot of the row holds the same key (two images of one
//           atom in a replica list);
//   rank    of a slot that counts = how many slots that count hold a smaller key: where the row's pairs go, ascending.
// The walks are wave-uniform (`while (__ballot(m != 0))`): every lane executes every __shfl, groups whose mask has run out idle.
//
// k_bond_rows, M <= 64: a row belongs to a group of G lanes (a power of two >= M), lane l holds slot l, and a group takes R
// consecutive rows: the counts, types, entries and distances of all R are loaded before anything is decided (a row is 12 M
// bytes — one row per group in flight left the pass waiting on four dependent memory latencies per wave, profiles/create_bonds.md).
// Entries behind a row's count are loaded too (they are inside the (N, M) arrays) and discarded by the predicate.
// WRITE = false: count[i] = slots that count.  WRITE = true: bond[offset[i] + rank] = (i, key).
template <int G, int R, bool WRITE>
__global__ __launch_bounds__(256) void k_bond_rows(BondList a, int64_t rows, unsigned *__restrict__ count, const int *__restrict__ offset,
                                                   int *__restrict__ bond, int64_t cap)
{
    const int t = threadIdx.x, l = t & (G - 1), gbase = (t & 63) & ~(G - 1);
    const int64_t row0 = (((int64_t)blockIdx.x * 256 + t) / G) * R;
    const unsigned long long gmask = G == 64 ? ~0ull : ((1ull << G) - 1ull);
    int n[R], ti[R], j[R], base[R];
    double d[R];
#pragma unroll
    for (int r = 0; r < R; ++r) {
        const int64_t row = row0 + r;
        const bool live = row < rows, has = live && l < a.M;
        n[r] = live ? a.nn[row] : 0;
        ti[r] = (live && a.type) ? a.type[row] : 0;
        j[r] = has ? a.verlet[row * a.M + l] : -1;
        d[r] = has ? a.dist[row * a.M + l] : 0.0;
        base[r] = (WRITE && live) ? offset[row] : 0;
    }
    int key[R];
    bool ok[R];
#pragma unroll
    for (int r = 0; r < R; ++r) ok[r] = bond_test(a, row0 + r, min(max(n[r], 0), (int)a.M), ti[r], l, j[r], d[r], key[r]);
#pragma unroll
    for (int r = 0; r < R; ++r) {
        bool dup = false;
        unsigned long long m = (__ballot(ok[r]) >> gbase) & gmask;
        while (__ballot(m != 0)) {
            const int s = m ? __builtin_ctzll(m) : 0;
            const int ks = __shfl(key[r], gbase + s, 64);
            if (m && ks == key[r] && s < l) dup = true;
            m &= m - 1;
        }
        const bool counts = ok[r] && !dup;
        const unsigned long long mine = (__ballot(counts) >> gbase) & gmask;
        if (!WRITE) {
            if (l == 0 && row0 + r < rows) count[row0 + r] = (unsigned)__builtin_popcountll(mine);
            continue;
        }
        int rank = 0;
        m = mine;
        while (__ballot(m != 0)) {
            const int s = m ? __builtin_ctzll(m) : 0;
            const int ks = __shfl(key[r], gbase + s, 64);
            if (m && ks < key[r]) ++rank;
            m &= m - 1;
        }
        const int64_t k = (int64_t)base[r] + rank;
        if (counts && k >= 0 && k < cap) reinterpret_cast<int2 *>(bond)[k] = make_int2((int)(row0 + r), key[r]);
    }
}

// k_bond_rows_wide, M > 64 (rc 6 A gives rows of 65-128): a wave per row, over chunks of 64 slots; lane l holds the slots
// 64 c + l.  One bit per chunk and lane ("first": my slot of chunk c counts) is kept between the two steps: 64 chunks,
// M <= 4096 (the entry refuses more).  Chunks in front of a lane's own are read again (they are in cache) instead of kept.
template <bool WRITE>
__global__ __launch_bounds__(256) void k_bond_rows_wide(BondList a, int64_t rows, unsigned *__restrict__ count, const int *__restrict__ offset,
                                                        int *__restrict__ bond, int64_t cap)
{
    const int l = threadIdx.x & 63;
    const int64_t i = ((int64_t)blockIdx.x * 256 + threadIdx.x) >> 6;
    if (i >= rows)
        return; // (wave-uniform: a wave has one row)
    const int n = min(max(a.nn[i], 0), (int)a.M);
    const int ti = a.type ? a.type[i] : 0;
    const int chunks = (int)((a.M + 63) / 64);
    auto slot = [&](int c, int &key) { // the predicate on my slot of chunk c
        const int64_t q = (int64_t)c * 64 + l;
        const bool has = q < a.M;
        return bond_test(a, i, n, ti, q, has ? a.verlet[i * a.M + q] : -1, has ? a.dist[i * a.M + q] : 0.0, key);
    };
    unsigned long long first = 0;
    unsigned total = 0;
    for (int c = 0; c < chunks; ++c) {
        int key;
        const bool ok = slot(c, key);
        bool dup = false;
        for (int e = 0; e <= c; ++e) { // the slots in front of mine: chunks 0 .. c - 1 whole, chunk c up to my lane
            int ekey = key;
            bool eok = ok;
            if (e < c) eok = slot(e, ekey);
            unsigned long long m = __ballot(eok);
            while (m) { // (the same word in every lane)
                const int s = __builtin_ctzll(m);
                const int ks = __shfl(ekey, s, 64);
                if (ks == key && (e < c || s < l)) dup = true;
                m &= m - 1;
            }
        }
        const bool counts = ok && !dup;
        if (counts) first |= 1ull << c;
        total += (unsigned)__builtin_popcountll(__ballot(counts));
    }
    if (!WRITE) {
        if (l == 0) count[i] = total;
        return;
    }
    if (!total)
        return;
    const int64_t base = offset[i];
    auto key_of = [&](int c, bool counted) {
        if (!counted)
            return 0x7fffffff;
        const int j = a.verlet[i * a.M + (int64_t)c * 64 + l];
        return a.n_real ? j % (int)a.n_real : j;
    };
    for (int c = 0; c < chunks; ++c) {
        const bool mine = (first >> c) & 1ull;
        const int key = key_of(c, mine);
        int rank = 0;
        for (int e = 0; e < chunks; ++e) {
            const bool theirs = (first >> e) & 1ull;
            const int ekey = e == c ? key : key_of(e, theirs);
            unsigned long long m = __ballot(theirs);
            while (m) {
                const int ks = __shfl(ekey, __builtin_ctzll(m), 64);
                if (ks < key) ++rank;
                m &= m - 1;
            }
        }
        const int64_t k = base + rank;
        if (mine && k >= 0 && k < cap) reinterpret_cast<int2 *>(bond)[k] = make_int2((int)i, key);
    }
}

constexpr int BOND_ROWS = 4; // rows a group of lanes takes (k_bond_rows)

template <int G>
static void launch_bond_rows(hipStream_t st, const BondList &a, int64_t rows, unsigned *count, const int *offset, int *bond, int64_t cap)
{
    const int64_t per_block = (int64_t)(256 / G) * BOND_ROWS;
    const dim3 grid((unsigned)((rows + per_block - 1) / per_block)), block(256);
    if (bond)
        hipLaunchKernelGGL((k_bond_rows<G, BOND_ROWS, true>), grid, block, 0, st, a, rows, count, offset, bond, cap);
    else
        hipLaunchKernelGGL((k_bond_rows<G, BOND_ROWS, false>), grid, block, 0, st, a, rows, count, offset, bond, cap);
}

static void bond_pass(hipStream_t st, const BondList &a, int64_t rows, unsigned *count, const int *offset, int *bond, int64_t cap)
{
    if (a.M > 64) {
        const dim3 grid((unsigned)grid_for(rows * 64, 256)), block(256);
        if (bond)
            hipLaunchKernelGGL(k_bond_rows_wide<true>, grid, block, 0, st, a, rows, count, offset, bond, cap);
        else
            hipLaunchKernelGGL(k_bond_rows_wide<false>, grid, block, 0, st, a, rows, count, offset, bond, cap);
    }
    else if (a.M > 32) launch_bond_rows<64>(st, a, rows, count, offset, bond, cap);
    else if (a.M > 16) launch_bond_rows<32>(st, a, rows, count, offset, bond, cap);
    else if (a.M > 8) launch_bond_rows<16>(st, a, rows, count, offset, bond, cap);
    else if (a.M > 4) launch_bond_rows<8>(st, a, rows, count, offset, bond, cap);
    else launch_bond_rows<4>(st, a, rows, count, offset, bond, cap);
}

// ---- compositions: comp[cluster - 1][type] += 1 per atom.  Integer addition commutes: any order of the adds gives the same
// table.  An id outside 1 .. n_cluster or a type outside 0 .. ntype - 1 raises the flag (the entry turns it into MDH_ERR_ARG).
__global__ __launch_bounds__(256) void k_cluster_composition(const int *__restrict__ cid, const int *__restrict__ type, int64_t N, int n_cluster,
                                                             int ntype, int *__restrict__ comp, int *__restrict__ bad)
{
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= N)
        return;
    const int c = cid[i], t = type[i];
    if ((unsigned)c - 1u >= (unsigned)n_cluster || (unsigned)t >= (unsigned)ntype) {
        *bad = 1; // (every lane that gets here stores the same word)
        return;
    }
    atomicAdd(&comp[(int64_t)(c - 1) * ntype + t], 1);
}

// label[c] = the LAST species whose row equals composition row c, or -1; counts[s] += 1 for EVERY species that equals it.  A wave
// counts its matches of a species with a ballot and adds once (all clusters add to the same few words).  No early return: every
// lane reaches every ballot.
__global__ __launch_bounds__(256) void k_species_match(const int *__restrict__ comp, int n_cluster, int ntype, const int *__restrict__ want,
                                                       int nspecies, int *__restrict__ label, unsigned long long *__restrict__ counts)
{
    const int64_t c = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    const bool live = c < n_cluster;
    const int *mine = comp + (live ? c : 0) * ntype;
    int last = -1;
    for (int s = 0; s < nspecies; ++s) {
        bool same = live;
        for (int t = 0; t < ntype && same; ++t) same = mine[t] == want[(int64_t)s * ntype + t];
        if (same) last = s;
        const unsigned n = (unsigned)__builtin_popcountll(__ballot(same));
        if (n && (threadIdx.x & 63) == 0) atomicAdd(&counts[s], (unsigned long long)n);
    }
    if (live) label[c] = last;
}

__global__ __launch_bounds__(256) void k_species_mol_id(const int *__restrict__ cid, int64_t N, int n_cluster, const int *__restrict__ label,
                                                        int *__restrict__ mol_id)
{
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= N)
        return;
    const int c = cid[i];
    mol_id[i] = (unsigned)c - 1u < (unsigned)n_cluster ? label[c - 1] : -1;
}

} // namespace mdh

using namespace mdh;

extern "C" {

int mdh_build_bond(const int *verlet, const double *dist, const int *nn, int64_t N, int64_t M, const int *type, const double *cutoff_host,
                   int ntype, int64_t n_real, int *bond, int64_t cap, int64_t *count_host, int space, void *stream)
{
    if (!count_host) { set_error("mdh_build_bond: count_host is NULL"); return MDH_ERR_ARG; }
    *count_host = 0;
    if (N < 0 || M <= 0 || cap < 0) { set_error("mdh_build_bond: bad sizes"); return MDH_ERR_ARG; }
    if (ntype < 1 || !cutoff_host) { set_error("mdh_build_bond: ntype must be at least 1, with an (ntype, ntype) cutoff matrix"); return MDH_ERR_ARG; }
    for (int64_t k = 0; k < (int64_t)ntype * ntype; ++k)
        if (!(cutoff_host[k] > 0.0) || !std::isfinite(cutoff_host[k])) { set_error("mdh_build_bond: every cutoff must be a positive number"); return MDH_ERR_ARG; }
    if (n_real < 0 || n_real > N) { set_error("mdh_build_bond: n_real is outside 0 .. N"); return MDH_ERR_ARG; }
    if (M > 4096) { set_error("mdh_build_bond: rows of more than 4096 slots"); return MDH_ERR_ARG; }
    const int64_t rows = n_real ? n_real : N;
    // (a row lists at most M pairs: the prefix sums and the pairs' slots are int32)
    if (N > 0x7fffffff || (double)rows * (double)M > 2147483647.0) { set_error("mdh_build_bond: the list can hold more bonds than int32 indexes"); return MDH_ERR_ARG; }
    if (N == 0)
        return MDH_OK;
    if (!verlet || !dist || !nn) { set_error("mdh_build_bond: verlet, dist or nn is NULL"); return MDH_ERR_ARG; }
    Scope sc(stream);
    hipStream_t st = sc.stream();
    BondList a;
    a.verlet = sc.stage_in(verlet, (size_t)(N * M), space);
    a.dist = sc.stage_in(dist, (size_t)(N * M), space);
    a.nn = sc.stage_in(nn, (size_t)N, space);
    a.type = type ? sc.stage_in(type, (size_t)N, space) : nullptr;
    a.cutoff = sc.stage_in(cutoff_host, (size_t)ntype * ntype, MDH_HOST);
    a.N = N; a.M = M; a.n_real = n_real; a.ntype = ntype;
    unsigned *count = sc.alloc_n<unsigned>((size_t)rows);
    int *offset = sc.alloc_n<int>((size_t)rows + 1);
    if (sc.failed())
        return sc.error();
    {
        ProfRange pr("k_bond_count", st);
        bond_pass(st, a, rows, count, nullptr, nullptr, 0);
    }
    {
        ProfRange pr("bond_scan", st);
        MDH_TRY(exclusive_scan_u32(sc, count, offset, rows));
    }
    int found = 0;
    MDH_HIP(hipMemcpyAsync(&found, offset + rows, sizeof(int), hipMemcpyDeviceToHost, st));
    MDH_HIP(hipStreamSynchronize(st)); // (also: the cutoffs were staged from caller memory)
    *count_host = found;
    if (!bond || found == 0)
        return sc.finish(space);
    if (found > cap) {
        set_error("mdh_build_bond: " + std::to_string(found) + " bonds, room for " + std::to_string(cap));
        return MDH_ERR_ARG;
    }
    int *db = sc.stage(bond, (size_t)found * 2, space, false, true);
    if (sc.failed())
        return sc.error();
    {
        ProfRange pr("k_bond_write", st);
        bond_pass(st, a, rows, count, offset, db, (int64_t)found);
    }
    MDH_HIP(hipGetLastError());
    return sc.finish(space);
}

int mdh_cluster_composition(const int *cluster_id, const int *type, int64_t N, int n_cluster, int ntype, int *comp, int space, void *stream)
{
    if (N < 0 || n_cluster < 0 || ntype < 1) { set_error("mdh_cluster_composition: bad sizes"); return MDH_ERR_ARG; }
    if (N > 0 && n_cluster == 0) { set_error("mdh_cluster_composition: atoms but no cluster"); return MDH_ERR_ARG; }
    if (n_cluster == 0)
        return MDH_OK;
    if (!comp || (N > 0 && (!cluster_id || !type))) { set_error("mdh_cluster_composition: an array is NULL"); return MDH_ERR_ARG; }
    if (N > (int64_t)0x7fffffff * 256) { set_error("mdh_cluster_composition: too many atoms for one launch"); return MDH_ERR_ARG; }
    const size_t cells = (size_t)n_cluster * (size_t)ntype;
    Scope sc(stream);
    hipStream_t st = sc.stream();
    const int *dc = sc.stage_in(cluster_id, (size_t)N, space), *dt = sc.stage_in(type, (size_t)N, space);
    int *dcomp = sc.stage(comp, cells, space, false, true);
    int *bad = sc.alloc_n<int>(1);
    if (sc.failed())
        return sc.error();
    MDH_HIP(hipMemsetAsync(dcomp, 0, cells * sizeof(int), st));
    MDH_HIP(hipMemsetAsync(bad, 0, sizeof(int), st));
    if (N > 0) {
        ProfRange pr("k_cluster_composition", st);
        hipLaunchKernelGGL(k_cluster_composition, dim3(grid_for(N, 256)), dim3(256), 0, st, dc, dt, N, n_cluster, ntype, dcomp, bad);
    }
    MDH_HIP(hipGetLastError());
    int flag = 0;
    MDH_HIP(hipMemcpyAsync(&flag, bad, sizeof(int), hipMemcpyDeviceToHost, st));
    MDH_HIP(hipStreamSynchronize(st));
    if (flag) {
        set_error("mdh_cluster_composition: a cluster id outside 1 .. " + std::to_string(n_cluster) + " or a type outside 0 .. " + std::to_string(ntype - 1));
        return MDH_ERR_ARG;
    }
    return sc.finish(space);
}

int mdh_species_match(const int *comp, int n_cluster, int ntype, const int *want_host, int nspecies, const int *cluster_id, int64_t N,
                      int *mol_id, int64_t *counts_host, int space, void *stream)
{
    if (n_cluster < 0 || ntype < 1 || nspecies < 0 || N < 0) { set_error("mdh_species_match: bad sizes"); return MDH_ERR_ARG; }
    if (nspecies > 0 && (!want_host || !counts_host)) { set_error("mdh_species_match: want_host or counts_host is NULL"); return MDH_ERR_ARG; }
    if (mol_id && N > 0 && !cluster_id) { set_error("mdh_species_match: mol_id needs cluster_id"); return MDH_ERR_ARG; }
    if (n_cluster > 0 && !comp) { set_error("mdh_species_match: comp is NULL"); return MDH_ERR_ARG; }
    if (N > (int64_t)0x7fffffff * 256) { set_error("mdh_species_match: too many atoms for one launch"); return MDH_ERR_ARG; }
    for (int s = 0; s < nspecies; ++s) counts_host[s] = 0;
    const bool atoms = mol_id && N > 0;
    if (nspecies == 0 && !atoms)
        return MDH_OK;
    Scope sc(stream);
    hipStream_t st = sc.stream();
    const int *dcomp = n_cluster ? sc.stage_in(comp, (size_t)n_cluster * (size_t)ntype, space) : nullptr;
    const int *dwant = nspecies ? sc.stage_in(want_host, (size_t)nspecies * (size_t)ntype, MDH_HOST) : nullptr;
    const int *dcid = atoms ? sc.stage_in(cluster_id, (size_t)N, space) : nullptr;
    int *dmol = atoms ? sc.stage(mol_id, (size_t)N, space, false, true) : nullptr;
    int *label = sc.alloc_n<int>((size_t)n_cluster);
    unsigned long long *counts = sc.alloc_n<unsigned long long>((size_t)nspecies);
    if (sc.failed())
        return sc.error();
    MDH_HIP(hipMemsetAsync(counts, 0, (size_t)(nspecies ? nspecies : 1) * sizeof(unsigned long long), st));
    {
        ProfRange pr("k_species_match", st);
        if (n_cluster > 0)
            hipLaunchKernelGGL(k_species_match, dim3(grid_for(n_cluster, 256)), dim3(256), 0, st, dcomp, n_cluster, ntype, dwant, nspecies, label, counts);
        if (atoms)
            hipLaunchKernelGGL(k_species_mol_id, dim3(grid_for(N, 256)), dim3(256), 0, st, dcid, N, n_cluster, label, dmol);
    }
    MDH_HIP(hipGetLastError());
    if (nspecies > 0) {
        static_assert(sizeof(unsigned long long) == sizeof(int64_t), "counts are copied as they are");
        MDH_HIP(hipMemcpyAsync(counts_host, counts, (size_t)nspecies * sizeof(int64_t), hipMemcpyDeviceToHost, st));
    }
    MDH_HIP(hipStreamSynchronize(st)); // (want_host was staged from caller memory)
    return sc.finish(space);
}
}

MDH_WARM_UNIT(bonds)
