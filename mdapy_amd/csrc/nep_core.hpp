// nep_core.hpp — what csrc/nep.hip shares with csrc/nep_charge.hip: the model's shape, the small device functions of the passes and
// the launchers of nep.hip's three kernels (defined there; its comments describe the model and the passes).
#pragma once
#include "common.hpp"
#include <algorithm>
#include <string>
#include <vector>

namespace mdh {

constexpr int NEP_MAX_N = 16, NEP_MAX_K = 17, NEP_MAX_NEURON = 128, NEP_MAX_DIM = NEP_MAX_N + 6 * NEP_MAX_N, NEP_MAX_FILE_TYPES = 96;
constexpr double NEP_PI = 3.14159265358979323846;
constexpr double NEP_COULOMB = 14.399645;  // e^2 / (4 pi eps0) in eV A
constexpr int NEP_GATHER_W = 8;

struct NepModel {
    int T, NR, KR, NA, KA, L3, L4, L5, H, dim, mode, nfile;
    int o_rc_r, o_rc_a, o_z, o_rcov, o_scaler, o_cr, o_ca, o_net, net_stride, o_b1;
    int charge, o_eps;  // charge models: the mode 1..3 (0: a potential model) and where sqrt(epsilon_inf) stands
    double zbl_inner, zbl_outer, zbl_factor;
    const double *p;
};
// a type of the FILE -> the model's own type, -1: none; by value, in the kernel's arguments
struct NepTypeMap { signed char local[NEP_MAX_FILE_TYPES]; };

// the minimum image of a difference.  Orthogonal boxes take d - L floor(d / L + 0.5) with the quotient as a product: the twelve
// thresholds of common.hpp's bit-exact form would sit in scalar registers beside the model's words, which are short here
template <bool TRI>
__device__ __forceinline__ void nep_image(const DBox &b, double &dx, double &dy, double &dz)
{
    if (TRI) {
        pbc<true>(b, dx, dy, dz);
    } else {
        if (b.pbc[0]) dx -= b.h[0] * floor(dx * b.hi[0] + 0.5);
        if (b.pbc[1]) dy -= b.h[4] * floor(dy * b.hi[4] + 0.5);
        if (b.pbc[2]) dz -= b.h[8] * floor(dz * b.hi[8] + 0.5);
    }
}

// the sum of v over the W lanes of a group, the same bits in every lane: a butterfly, so the order depends on W alone
template <int W>
__device__ __forceinline__ double group_sum(double v)
{
#pragma unroll
    for (int step = 1; step < W; step <<= 1) v += __shfl_xor(v, step, 64);
    return v;
}

// where row j names i (the list names a replica's copies by their own index, so the entry is unique); -1: nowhere
__device__ __forceinline__ int nep_back(const int *__restrict__ verlet, const int *__restrict__ nn, int64_t M, int j, int64_t i)
{
    const int nj = min(max(nn[j], 0), (int)M);
    const int *row = verlet + (int64_t)j * M;
    for (int q = 0; q < nj; ++q)
        if (row[q] == (int)i)
            return q;
    return -1;
}

// what every pass reads: the list, the box, the atoms' records, the model
struct NepPassArgs {
    const int *verlet;
    const double *dist;
    const int *nn;
    int64_t N, M;
    DBox b;
    const Pos4 *rec;
    NepModel m;
    bool wide() const { return std::max(m.NR, m.NA) > 8; }  // 16 lanes an atom instead of 8
};

// the header words -> the model's shape and the offsets into its block (m.p is left alone); len: the block's length.  charge: a
// charge model (w1 of 2 x neurons per type, sqrt(epsilon_inf) before the common bias).  -> MDH_OK, or MDH_ERR_ARG with the error set
int nep_model_of(const std::string &who, const int *h, int nfile, const double *zbl3_host, const int *type_map_host, bool charge, NepModel &m,
                 int64_t &len);
// positions and the model's own type of every atom as one 32-byte record (w = the type, -1: none)
void nep_launch_pack(hipStream_t st, const double *x, const double *y, const double *z, const int *type, const NepTypeMap &map, int64_t N,
                     const NepModel &m, Pos4 *rec);
// pass A.  charge != NULL: a charge model — the network's second output and its derivatives FpRq, Aq are written as well
void nep_launch_descriptor(hipStream_t st, const NepPassArgs &a, double *energy, double *FpR, double *A, double *descriptor, double *latent,
                           double *charge, double *FpRq, double *Aq);
// pass B1.  D != NULL: Fp + D_i FpRq and A + D_i Aq take the place of Fp and A
void nep_launch_pair(hipStream_t st, const NepPassArgs &a, const double *FpR, const double *A, double *table, const double *FpRq, const double *Aq,
                     const double *D);
// pass B2.  addf != NULL: the force and the virial start from addf, addv instead of zero
void nep_launch_gather(hipStream_t st, const NepPassArgs &a, const double *table, double *force, double *virial, const double *addf,
                       const double *addv);

} // namespace mdh
