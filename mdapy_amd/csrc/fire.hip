// fire.hip — the arithmetic of the FIRE minimizer (mdapy_amd/minimizer.py; the reference's is numpy, src/mdapy/minimizer.py:270-375)
// on (n, 3) f64 arrays that stay in HBM: the row dot products and their sums, the kick, the mix, the move and the row-times-3x3
// transform of the cell mode.  DESIGN.md §5m.
//
// Every kernel streams: one thread per row (24 contiguous bytes a lane, whole cache lines a wave), no LDS but the reductions'.
// Built with -ffp-contract=off: a product is rounded before it is added, as numpy rounds it.
//
// THE ORDER OF A SUM over the terms t_0 .. t_{n-1} (one per row) depends on n alone:
//   level 1  block b of 256 threads holds t_{256 b + k} in thread k (0.0 past the end) and halves: for h = 128, 64, .. 1,
//            thread k < h takes s_k = s_k + s_{k+h}; its partial is s_0.
//   level 2  one block of 256 threads: thread k starts from 0.0 and adds the partials k, k + 256, k + 512, .. in turn, then
//            the same halving.
// Level 2 is a launch of its own (k_fire_finish) that writes the result into the caller's record in HBM, where the next kernel
// reads it: no float atomics, no ticket, and no read by the host in between.
#include "common.hpp"

namespace mdh {

constexpr int FIRE_BLOCK = 256;
constexpr int FIRE_MAX_SUMS = 4;

__device__ __forceinline__ double fire_tree(double t, double *s)
{
    const int k = threadIdx.x;
    s[k] = t;
    __syncthreads();
#pragma unroll
    for (int h = FIRE_BLOCK / 2; h >= 1; h >>= 1) {
        if (k < h) s[k] = s[k] + s[k + h];
        __syncthreads();
    }
    const double r = s[0];
    __syncthreads();
    return r;
}

// the larger of two, a NaN wins (numpy's max)
__device__ __forceinline__ double fire_larger(double a, double b) { return (a > b || a != a) ? a : b; }

__device__ __forceinline__ double fire_tree_max(double t, double *s)
{
    const int k = threadIdx.x;
    s[k] = t;
    __syncthreads();
#pragma unroll
    for (int h = FIRE_BLOCK / 2; h >= 1; h >>= 1) {
        if (k < h) s[k] = fire_larger(s[k], s[k + h]);
        __syncthreads();
    }
    const double r = s[0];
    __syncthreads();
    return r;
}

__device__ __forceinline__ double row_dot(double ax, double ay, double az, double bx, double by, double bz)
{
    return (ax * bx + ay * by) + az * bz;
}

struct FireSlots {
    int count;
    int slot[FIRE_MAX_SUMS];   // word of the record the sum goes to
    int is_max[FIRE_MAX_SUMS]; // a maximum (of terms >= 0), not a sum
};

// level 2: block s combines the nb partials of sum s
__global__ void __launch_bounds__(FIRE_BLOCK) k_fire_finish(const double *__restrict__ part, int64_t nb, FireSlots fs, double *__restrict__ rec)
{
    __shared__ double s[FIRE_BLOCK];
    const int which = blockIdx.x, k = threadIdx.x;
    const double *p = part + (int64_t)which * nb;
    double r;
    if (fs.is_max[which]) {
        double acc = 0.0;
        for (int64_t j = k; j < nb; j += FIRE_BLOCK) acc = fire_larger(acc, p[j]);
        r = fire_tree_max(acc, s);
    } else {
        double acc = 0.0;
        for (int64_t j = k; j < nb; j += FIRE_BLOCK) acc = acc + p[j];
        r = fire_tree(acc, s);
    }
    if (k == 0) rec[fs.slot[which]] = r;
}

// v . f, f . f and max |f_i|^2 (the f . f term of a row is |f_i|^2).  v == nullptr: the first step, v . f = 0
__global__ void __launch_bounds__(FIRE_BLOCK) k_fire_dots(const double *__restrict__ v, const double *__restrict__ f, int64_t n, int64_t nb,
                                                            double *__restrict__ part)
{
    __shared__ double s[FIRE_BLOCK];
    const int64_t i = (int64_t)blockIdx.x * FIRE_BLOCK + threadIdx.x;
    double tvf = 0.0, tff = 0.0;
    if (i < n) {
        const double fx = f[3 * i], fy = f[3 * i + 1], fz = f[3 * i + 2];
        tff = row_dot(fx, fy, fz, fx, fy, fz);
        if (v) tvf = row_dot(v[3 * i], v[3 * i + 1], v[3 * i + 2], fx, fy, fz);
    }
    const double a = fire_tree(tvf, s), b = fire_tree(tff, s), c = fire_tree_max(tff, s);
    if (threadIdx.x == 0) {
        part[blockIdx.x] = a;
        part[nb + blockIdx.x] = b;
        part[2 * nb + blockIdx.x] = c;
    }
}

// v = v + dt * f (zero_first: v = v * 0.0 before, the uphill branch's reset); f . f and v . v of the new v
__global__ void __launch_bounds__(FIRE_BLOCK) k_fire_kick(double *__restrict__ v, const double *__restrict__ f, int64_t n, int64_t nb, double dt,
                                                            int zero_first, double *__restrict__ part)
{
    __shared__ double s[FIRE_BLOCK];
    const int64_t i = (int64_t)blockIdx.x * FIRE_BLOCK + threadIdx.x;
    double tff = 0.0, tvv = 0.0;
    if (i < n) {
        const double fx = f[3 * i], fy = f[3 * i + 1], fz = f[3 * i + 2];
        double vx = v[3 * i], vy = v[3 * i + 1], vz = v[3 * i + 2];
        if (zero_first) {
            vx = vx * 0.0;
            vy = vy * 0.0;
            vz = vz * 0.0;
        }
        vx = vx + dt * fx;
        vy = vy + dt * fy;
        vz = vz + dt * fz;
        v[3 * i] = vx;
        v[3 * i + 1] = vy;
        v[3 * i + 2] = vz;
        tff = row_dot(fx, fy, fz, fx, fy, fz);
        tvv = row_dot(vx, vy, vz, vx, vy, vz);
    }
    const double a = fire_tree(tff, s), b = fire_tree(tvv, s);
    if (threadIdx.x == 0) {
        part[blockIdx.x] = a;
        part[nb + blockIdx.x] = b;
    }
}

// v = (1 - a) v + ((a f) / sqrt(f.f)) sqrt(v.v), times `mult` with ABC; the sums the move needs: dr . dr of dr = dt v, and how
// many components of v are exactly zero (a sum of small integers: exact in any order)
__global__ void __launch_bounds__(FIRE_BLOCK) k_fire_mix(double *__restrict__ v, const double *__restrict__ f, int64_t n, int64_t nb, double a,
                                                           double mult, int use_abc, double dt, const double *__restrict__ rec, int ff_word,
                                                           int vv_word, double *__restrict__ part)
{
    __shared__ double s[FIRE_BLOCK];
    const int64_t i = (int64_t)blockIdx.x * FIRE_BLOCK + threadIdx.x;
    const double sf = sqrt(rec[ff_word]), sv = sqrt(rec[vv_word]), keep = 1.0 - a;
    double tdd = 0.0, tzero = 0.0;
    if (i < n) {
        double m[3];
#pragma unroll
        for (int c = 0; c < 3; ++c) {
            m[c] = keep * v[3 * i + c] + ((a * f[3 * i + c]) / sf) * sv;
            if (use_abc) m[c] = mult * m[c];
            v[3 * i + c] = m[c];
            if (m[c] == 0.0) tzero = tzero + 1.0;
        }
        const double dx = dt * m[0], dy = dt * m[1], dz = dt * m[2];
        tdd = row_dot(dx, dy, dz, dx, dy, dz);
    }
    const double p = fire_tree(tdd, s), q = fire_tree(tzero, s);
    if (threadIdx.x == 0) {
        part[blockIdx.x] = p;
        part[nb + blockIdx.x] = q;
    }
}

enum { FIRE_MOVE_NORM = 0, FIRE_MOVE_CAP = 1, FIRE_MOVE_PLAIN = 2 };

// dr = scale v, limited; the first n_atoms rows move the atoms: u += dr (u given: the cell mode's unstrained positions, in
// place) or xo = xi + dr column by column (out of place: a frame's columns never change)
__global__ void __launch_bounds__(FIRE_BLOCK) k_fire_move(double *__restrict__ v, double *__restrict__ dr, int64_t n, int64_t n_atoms, double scale,
                                                            double dt, double maxstep, int mode, const double *__restrict__ rec, int dd_word,
                                                            int zero_word, const double *__restrict__ xi, const double *__restrict__ yi,
                                                            const double *__restrict__ zi, double *__restrict__ xo, double *__restrict__ yo,
                                                            double *__restrict__ zo, double *__restrict__ u)
{
    const int64_t i = (int64_t)blockIdx.x * FIRE_BLOCK + threadIdx.x;
    if (i >= n) return;
    double w[3] = {v[3 * i], v[3 * i + 1], v[3 * i + 2]};
    if (mode == FIRE_MOVE_CAP && rec[zero_word] == 0.0) { // (ABC-FIRE caps per component, and only when no component is zero)
#pragma unroll
        for (int c = 0; c < 3; ++c) {
            const double size = fabs(w[c]);
            if (size * dt > maxstep) w[c] = (maxstep / dt) * (w[c] / size);
            v[3 * i + c] = w[c];
        }
    }
    double d[3] = {scale * w[0], scale * w[1], scale * w[2]};
    if (mode == FIRE_MOVE_NORM) {
        const double norm = sqrt(rec[dd_word]);
        if (norm > maxstep) {
#pragma unroll
            for (int c = 0; c < 3; ++c) d[c] = (maxstep * d[c]) / norm;
        }
    }
    dr[3 * i] = d[0];
    dr[3 * i + 1] = d[1];
    dr[3 * i + 2] = d[2];
    if (i < n_atoms) {
        if (u) {
            u[3 * i] = u[3 * i] + d[0];
            u[3 * i + 1] = u[3 * i + 1] + d[1];
            u[3 * i + 2] = u[3 * i + 2] + d[2];
        } else {
            xo[i] = xi[i] + d[0];
            yo[i] = yi[i] + d[1];
            zo[i] = zi[i] + d[2];
        }
    }
}

struct Mat9 { double m[9]; };

// row times 3x3: o_k = (x m_0k + y m_1k) + z m_2k, into rows (out) or into three columns
__global__ void __launch_bounds__(FIRE_BLOCK) k_fire_rowmat(const double *__restrict__ in, int64_t n, Mat9 M, double *__restrict__ out,
                                                              double *__restrict__ ox, double *__restrict__ oy, double *__restrict__ oz)
{
    const int64_t i = (int64_t)blockIdx.x * FIRE_BLOCK + threadIdx.x;
    if (i >= n) return;
    const double x = in[3 * i], y = in[3 * i + 1], z = in[3 * i + 2];
    const double a = (x * M.m[0] + y * M.m[3]) + z * M.m[6];
    const double b = (x * M.m[1] + y * M.m[4]) + z * M.m[7];
    const double c = (x * M.m[2] + y * M.m[5]) + z * M.m[8];
    if (out) {
        out[3 * i] = a;
        out[3 * i + 1] = b;
        out[3 * i + 2] = c;
    } else {
        ox[i] = a;
        oy[i] = b;
        oz[i] = c;
    }
}

// out[perm[p]] = in[p], rows of three (a twin's forces back in the caller's order); an entry outside [0, n) moves nothing
__global__ void __launch_bounds__(FIRE_BLOCK) k_fire_scatter_rows(const double *__restrict__ in, const int *__restrict__ perm, int64_t n,
                                                                    double *__restrict__ out)
{
    const int64_t p = (int64_t)blockIdx.x * FIRE_BLOCK + threadIdx.x;
    if (p >= n) return;
    const int64_t to = perm[p];
    if (to < 0 || to >= n) return;
    out[3 * to] = in[3 * p];
    out[3 * to + 1] = in[3 * p + 1];
    out[3 * to + 2] = in[3 * p + 2];
}

// the terms of a plain sum: the numbers themselves
__global__ void __launch_bounds__(FIRE_BLOCK) k_fire_sum(const double *__restrict__ a, int64_t n, double *__restrict__ part)
{
    __shared__ double s[FIRE_BLOCK];
    const int64_t i = (int64_t)blockIdx.x * FIRE_BLOCK + threadIdx.x;
    const double r = fire_tree(i < n ? a[i] : 0.0, s);
    if (threadIdx.x == 0) part[blockIdx.x] = r;
}

static bool fire_rows_ok(const char *what, int64_t n)
{
    if (n < 1 || n > (int64_t(1) << 36)) {
        set_error(std::string(what) + ": between 1 and 2^36 rows");
        return false;
    }
    return true;
}

static bool fire_word_ok(const char *what, int word)
{
    if (word < 0 || word >= MDH_FIRE_RECORD) {
        set_error(std::string(what) + ": a word of the record is 0 .. MDH_FIRE_RECORD - 1");
        return false;
    }
    return true;
}

static void fire_finish(Scope &sc, const double *part, int64_t nb, const FireSlots &fs, double *rec)
{
    hipLaunchKernelGGL(k_fire_finish, dim3(fs.count), dim3(FIRE_BLOCK), 0, sc.stream(), part, nb, fs, rec);
}

} // namespace mdh

using namespace mdh;

int mdh_fire_dots(const double *v, const double *f, int64_t n, double *record, int space, void *stream)
{
    if (!fire_rows_ok("mdh_fire_dots", n)) return MDH_ERR_ARG;
    if (!f || !record) { set_error("mdh_fire_dots: null array"); return MDH_ERR_ARG; }
    Scope sc(stream);
    const double *dv = v ? sc.stage_in(v, (size_t)n * 3, space) : nullptr;
    const double *df = sc.stage_in(f, (size_t)n * 3, space);
    double *drec = sc.stage(record, (size_t)MDH_FIRE_RECORD, space, true, true);
    const int64_t nb = grid_for(n, FIRE_BLOCK);
    double *part = sc.alloc_n<double>((size_t)nb * 3);
    if (sc.failed()) return sc.error();
    ProfRange pr("k_fire_dots", sc.stream()); // (with its k_fire_finish, where it has one)
    hipLaunchKernelGGL(k_fire_dots, dim3((unsigned)nb), dim3(FIRE_BLOCK), 0, sc.stream(), dv, df, n, nb, part);
    FireSlots fs = {3, {MDH_FIRE_VF, MDH_FIRE_FF, MDH_FIRE_FMAX2, 0}, {0, 0, 1, 0}};
    fire_finish(sc, part, nb, fs, drec);
    MDH_HIP(hipGetLastError());
    return sc.finish(space);
}

int mdh_fire_kick(double *v, const double *f, int64_t n, double dt, int zero_first, double *record, int space, void *stream)
{
    if (!fire_rows_ok("mdh_fire_kick", n)) return MDH_ERR_ARG;
    if (!v || !f || !record) { set_error("mdh_fire_kick: null array"); return MDH_ERR_ARG; }
    Scope sc(stream);
    double *dv = sc.stage(v, (size_t)n * 3, space, true, true);
    const double *df = sc.stage_in(f, (size_t)n * 3, space);
    double *drec = sc.stage(record, (size_t)MDH_FIRE_RECORD, space, true, true);
    const int64_t nb = grid_for(n, FIRE_BLOCK);
    double *part = sc.alloc_n<double>((size_t)nb * 2);
    if (sc.failed()) return sc.error();
    ProfRange pr("k_fire_kick", sc.stream()); // (with its k_fire_finish, where it has one)
    hipLaunchKernelGGL(k_fire_kick, dim3((unsigned)nb), dim3(FIRE_BLOCK), 0, sc.stream(), dv, df, n, nb, dt, zero_first, part);
    FireSlots fs = {2, {MDH_FIRE_FF, MDH_FIRE_VV, 0, 0}, {0, 0, 0, 0}};
    fire_finish(sc, part, nb, fs, drec);
    MDH_HIP(hipGetLastError());
    return sc.finish(space);
}

int mdh_fire_mix(double *v, const double *f, int64_t n, double a, double abc_multiplier, int use_abc, double dt, double *record, int space,
                 void *stream)
{
    if (!fire_rows_ok("mdh_fire_mix", n)) return MDH_ERR_ARG;
    if (!v || !f || !record) { set_error("mdh_fire_mix: null array"); return MDH_ERR_ARG; }
    Scope sc(stream);
    double *dv = sc.stage(v, (size_t)n * 3, space, true, true);
    const double *df = sc.stage_in(f, (size_t)n * 3, space);
    double *drec = sc.stage(record, (size_t)MDH_FIRE_RECORD, space, true, true);
    const int64_t nb = grid_for(n, FIRE_BLOCK);
    double *part = sc.alloc_n<double>((size_t)nb * 2);
    if (sc.failed()) return sc.error();
    ProfRange pr("k_fire_mix", sc.stream()); // (with its k_fire_finish, where it has one)
    hipLaunchKernelGGL(k_fire_mix, dim3((unsigned)nb), dim3(FIRE_BLOCK), 0, sc.stream(), dv, df, n, nb, a, abc_multiplier, use_abc, dt,
                       (const double *)drec, (int)MDH_FIRE_FF, (int)MDH_FIRE_VV, part);
    FireSlots fs = {2, {MDH_FIRE_DRDR, MDH_FIRE_ZEROS, 0, 0}, {0, 0, 0, 0}};
    fire_finish(sc, part, nb, fs, drec);
    MDH_HIP(hipGetLastError());
    return sc.finish(space);
}

int mdh_fire_move(double *v, double *dr, int64_t n, int64_t n_atoms, double scale, double dt, double maxstep, int mode, const double *record,
                  const double *x, const double *y, const double *z, double *x_out, double *y_out, double *z_out, double *unstrained,
                  int space, void *stream)
{
    if (!fire_rows_ok("mdh_fire_move", n)) return MDH_ERR_ARG;
    if (n_atoms < 0 || n_atoms > n || mode < FIRE_MOVE_NORM || mode > FIRE_MOVE_PLAIN) { set_error("mdh_fire_move: n_atoms within the rows, mode 0, 1 or 2"); return MDH_ERR_ARG; }
    const bool columns = !unstrained;
    if (!v || !dr || !record || (columns && n_atoms > 0 && (!x || !y || !z || !x_out || !y_out || !z_out))) { set_error("mdh_fire_move: null array"); return MDH_ERR_ARG; }
    if (columns && (x == x_out || y == y_out || z == z_out)) { set_error("mdh_fire_move: the new columns are written out of place"); return MDH_ERR_ARG; }
    Scope sc(stream);
    double *dv = sc.stage(v, (size_t)n * 3, space, true, mode == FIRE_MOVE_CAP);
    double *ddr = sc.stage(dr, (size_t)n * 3, space, false, true);
    const double *drec = sc.stage_in(record, (size_t)MDH_FIRE_RECORD, space);
    const double *dx = nullptr, *dy = nullptr, *dz = nullptr;
    double *dxo = nullptr, *dyo = nullptr, *dzo = nullptr, *du = nullptr;
    if (columns && n_atoms > 0) {
        dx = sc.stage_in(x, (size_t)n_atoms, space);
        dy = sc.stage_in(y, (size_t)n_atoms, space);
        dz = sc.stage_in(z, (size_t)n_atoms, space);
        dxo = sc.stage(x_out, (size_t)n_atoms, space, false, true);
        dyo = sc.stage(y_out, (size_t)n_atoms, space, false, true);
        dzo = sc.stage(z_out, (size_t)n_atoms, space, false, true);
    } else if (!columns && n_atoms > 0) {
        du = sc.stage(unstrained, (size_t)n_atoms * 3, space, true, true);
    }
    if (sc.failed()) return sc.error();
    const int64_t moved = (columns || du) ? n_atoms : 0;
    ProfRange pr("k_fire_move", sc.stream()); // (with its k_fire_finish, where it has one)
    hipLaunchKernelGGL(k_fire_move, dim3((unsigned)grid_for(n, FIRE_BLOCK)), dim3(FIRE_BLOCK), 0, sc.stream(), dv, ddr, n, moved, scale, dt, maxstep,
                       mode, drec, (int)MDH_FIRE_DRDR, (int)MDH_FIRE_ZEROS, dx, dy, dz, dxo, dyo, dzo, du);
    MDH_HIP(hipGetLastError());
    return sc.finish(space);
}

int mdh_fire_rowmat(const double *rows, int64_t n, const double *matrix9, double *out_rows, double *out_x, double *out_y, double *out_z,
                    int space, void *stream)
{
    if (!fire_rows_ok("mdh_fire_rowmat", n)) return MDH_ERR_ARG;
    if (!rows || !matrix9 || (!out_rows && (!out_x || !out_y || !out_z)) || rows == out_rows) { set_error("mdh_fire_rowmat: null array, or in place"); return MDH_ERR_ARG; }
    Scope sc(stream);
    const double *din = sc.stage_in(rows, (size_t)n * 3, space);
    double *dout = nullptr, *dx = nullptr, *dy = nullptr, *dz = nullptr;
    if (out_rows) {
        dout = sc.stage(out_rows, (size_t)n * 3, space, false, true);
    } else {
        dx = sc.stage(out_x, (size_t)n, space, false, true);
        dy = sc.stage(out_y, (size_t)n, space, false, true);
        dz = sc.stage(out_z, (size_t)n, space, false, true);
    }
    if (sc.failed()) return sc.error();
    Mat9 M;
    for (int k = 0; k < 9; ++k) M.m[k] = matrix9[k];
    ProfRange pr("k_fire_rowmat", sc.stream()); // (with its k_fire_finish, where it has one)
    hipLaunchKernelGGL(k_fire_rowmat, dim3((unsigned)grid_for(n, FIRE_BLOCK)), dim3(FIRE_BLOCK), 0, sc.stream(), din, n, M, dout, dx, dy, dz);
    MDH_HIP(hipGetLastError());
    return sc.finish(space);
}

int mdh_fire_scatter_rows(const double *rows, const int *perm, int64_t n, double *out_rows, int space, void *stream)
{
    if (!fire_rows_ok("mdh_fire_scatter_rows", n)) return MDH_ERR_ARG;
    if (!rows || !perm || !out_rows || rows == out_rows) { set_error("mdh_fire_scatter_rows: null array, or in place"); return MDH_ERR_ARG; }
    Scope sc(stream);
    const double *din = sc.stage_in(rows, (size_t)n * 3, space);
    const int *dp = sc.stage_in(perm, (size_t)n, space);
    double *dout = sc.stage(out_rows, (size_t)n * 3, space, true, true); // (in: a row no entry names keeps what it held)
    if (sc.failed()) return sc.error();
    ProfRange pr("k_fire_scatter_rows", sc.stream()); // (with its k_fire_finish, where it has one)
    hipLaunchKernelGGL(k_fire_scatter_rows, dim3((unsigned)grid_for(n, FIRE_BLOCK)), dim3(FIRE_BLOCK), 0, sc.stream(), din, dp, n, dout);
    MDH_HIP(hipGetLastError());
    return sc.finish(space);
}

int mdh_fire_sum(const double *values, int64_t n, int word, double *record, int space, void *stream)
{
    if (!fire_rows_ok("mdh_fire_sum", n) || !fire_word_ok("mdh_fire_sum", word)) return MDH_ERR_ARG;
    if (!values || !record) { set_error("mdh_fire_sum: null array"); return MDH_ERR_ARG; }
    Scope sc(stream);
    const double *da = sc.stage_in(values, (size_t)n, space);
    double *drec = sc.stage(record, (size_t)MDH_FIRE_RECORD, space, true, true);
    const int64_t nb = grid_for(n, FIRE_BLOCK);
    double *part = sc.alloc_n<double>((size_t)nb);
    if (sc.failed()) return sc.error();
    ProfRange pr("k_fire_sum", sc.stream()); // (with its k_fire_finish, where it has one)
    hipLaunchKernelGGL(k_fire_sum, dim3((unsigned)nb), dim3(FIRE_BLOCK), 0, sc.stream(), da, n, part);
    FireSlots fs = {1, {word, 0, 0, 0}, {0, 0, 0, 0}};
    fire_finish(sc, part, nb, fs, drec);
    MDH_HIP(hipGetLastError());
    return sc.finish(space);
}

MDH_WARM_UNIT(fire)
