// knn_geom.hpp — what the nearest-neighbour searches over a cell grid share (knn.hip: the k nearest atoms of the same set;
// wigner_seitz.hip: the nearest site of another set): the reference's wrap, its image count, the grid sizing and the mapping of an
// extended cell index to (stored cell, image).  src/fast_knn.cpp lines are cited where an expression is the reference's.
#pragma once
#include "common.hpp"
#include "grid.hpp"
#include <cmath>

namespace mdh {

struct KnnGeom {
    int nim[3];    // images per axis (0 on open axes)
    double wmin;   // smallest perpendicular cell width
    int rmax;      // ring index after which every (cell, image) has been visited
};

// the reference's wrap of a point into the primary cell, operation for operation (a stored atom and a query that coincide with it
// must come out bitwise equal):
//   orthogonal  s = floor((p-O)*(1/L)); if (s != 0) p -= s*L            (:688-703, :743-757)
//   triclinic   r = p.inv (NO origin shift); s = floor(r_d); p -= s*row_d (:86-99)
template <bool TRI>
__device__ __forceinline__ void knn_wrap_point(const DBox &b, double &px, double &py, double &pz)
{
    if (TRI) {
        const double r0 = px * b.hi[0] + py * b.hi[3] + pz * b.hi[6];
        const double r1 = px * b.hi[1] + py * b.hi[4] + pz * b.hi[7];
        const double r2 = px * b.hi[2] + py * b.hi[5] + pz * b.hi[8];
        const double r[3] = {r0, r1, r2};
#pragma unroll
        for (int d = 0; d < 3; ++d)
            if (b.pbc[d]) {
                const double s = floor(r[d]);
                if (s != 0.0) { px -= s * b.h[d * 3 + 0]; py -= s * b.h[d * 3 + 1]; pz -= s * b.h[d * 3 + 2]; }
            }
    } else {
        if (b.pbc[0]) { const double s = floor((px - b.o[0]) * (1.0 / b.h[0])); if (s != 0.0) px -= s * b.h[0]; }
        if (b.pbc[1]) { const double s = floor((py - b.o[1]) * (1.0 / b.h[4])); if (s != 0.0) py -= s * b.h[4]; }
        if (b.pbc[2]) { const double s = floor((pz - b.o[2]) * (1.0 / b.h[8])); if (s != 0.0) pz -= s * b.h[8]; }
    }
}

__device__ __forceinline__ int floordiv(int a, int n) { int q = a / n; return (a % n < 0) ? q - 1 : q; }

// extended cell index e along axis d -> (stored cell a, image number m); false: no such cell (beyond an open face, or more
// images away than the reference looks, fast_knn.cpp:806-816).  (The kernels of knn.hip carry this as a lambda of their own.)
__device__ __forceinline__ bool knn_fold_cell(const DBox &b, const Grid &g, const KnnGeom &kg, int d, int e, int &a, int &m)
{
    m = 0; a = e;
    if (b.pbc[d]) { m = floordiv(e, g.nc[d]); a = e - m * g.nc[d]; return !(m > kg.nim[d] || m < -kg.nim[d]); }
    return e >= 0 && e < g.nc[d];
}

// image shift, fast_knn.cpp:822-833.  An atom stored in cell (a0,a1,a2), seen through the extended cell e = a + m*nc, is the
// image a + m*L.  Its distance to the query is |a - (q - m*L)|: the reference's shifted query with shift = m*L (:759-763)
template <bool TRI>
__device__ __forceinline__ void knn_image_shift(const DBox &b, int m0, int m1, int m2, double &s0, double &s1, double &s2)
{
    if (TRI) {
        s0 = m0 * b.h[0] + m1 * b.h[3] + m2 * b.h[6];
        s1 = m0 * b.h[1] + m1 * b.h[4] + m2 * b.h[7];
        s2 = m0 * b.h[2] + m1 * b.h[5] + m2 * b.h[8];
    } else {
        s0 = m0 * b.h[0]; s1 = m1 * b.h[4]; s2 = m2 * b.h[8];
    }
}

inline double knn_box_volume(const DBox &b)
{
    return std::fabs(b.tri ? (b.h[0] * (b.h[4] * b.h[8] - b.h[5] * b.h[7]) - b.h[1] * (b.h[3] * b.h[8] - b.h[5] * b.h[6]) + b.h[2] * (b.h[3] * b.h[7] - b.h[4] * b.h[6])) : b.h[0] * b.h[4] * b.h[8]);
}

// images per periodic axis for a search among N atoms (fast_knn.cpp:806-816)
inline void knn_images(const DBox &b, int64_t N, KnnGeom &kg)
{
    int nim = 1;
    if (b.anypbc) {
        int64_t cl = N < 50 ? 50 : (N > 200 ? 200 : N);
        nim = (int)(200 / cl);
        if (nim < 1) nim = 1;
        if (nim < 2 && b.tri) nim = 2;
    }
    for (int d = 0; d < 3; ++d) kg.nim[d] = b.pbc[d] ? nim : 0;
}

// the grid of a search: equal cells across the box (Grid mode 1) that hold ~per_cell atoms each, at most ~4 cells per atom
// (sparse / slab-like systems); kg.wmin and kg.rmax follow (kg.nim: knn_images, before).  A function of (N, box, per_cell) alone.
inline void knn_size_grid(const DBox &b, int64_t N, double per_cell, Grid &g, KnnGeom &kg)
{
    double wtarget = std::cbrt(knn_box_volume(b) * per_cell / (double)N);
    if (!(wtarget > 0) || !std::isfinite(wtarget)) wtarget = 1.0;
    double tot = 1.0;
    kg.wmin = __builtin_huge_val();
    kg.rmax = 0;
    for (int d = 0; d < 3; ++d) {
        const double th = std::fabs(b.thick[d]);
        double f = std::floor(th / wtarget);
        int n = (f < 1.0 || !(f == f)) ? 1 : (f > 1024.0 ? 1024 : (int)f);
        g.nc[d] = n;
        tot *= n;
    }
    while (tot > 4.0 * (double)N + 64.0) {
        int dmax = 0;
        for (int d = 1; d < 3; ++d) if (g.nc[d] > g.nc[dmax]) dmax = d;
        if (g.nc[dmax] <= 1) break;
        tot /= g.nc[dmax];
        g.nc[dmax] = (g.nc[dmax] + 1) / 2;
        tot *= g.nc[dmax];
    }
    for (int d = 0; d < 3; ++d) {
        const double w = std::fabs(b.thick[d]) / g.nc[d];
        if (w < kg.wmin) kg.wmin = w;
        const int r = b.pbc[d] ? (kg.nim[d] + 1) * g.nc[d] : g.nc[d] - 1;
        if (r > kg.rmax) kg.rmax = r;
    }
    g.ncell = (int64_t)g.nc[0] * g.nc[1] * g.nc[2];
    g.rc_inv = 0.0;
    g.mode = 1;
}

} // namespace mdh
