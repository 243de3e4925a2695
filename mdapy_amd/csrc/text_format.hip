// text_format.hip — numeric columns in HBM -> the bytes of a text table (the output side).
//
// Reference behaviour: every writer of src/mdapy/load_save.py:1534-2017 (dump, data, xyz, poscar) hands its atom table to a
// CSV writer with separator " ", no header and float_precision=10: one row per atom, fields joined by one blank, rows ended by
// "\n", floats as format(v, ".10f"), integers in plain decimal, strings as they are.  The reference formats on the host; here
// the columns stay in HBM and three steps make the text there (the inverse of text.hip):
//   k_format_measure  one row per lane: the length of the row's text (conversion = text_format.hpp, exact)
//   exclusive scan    lengths -> the byte offset of every row (rows differ in length, and rounding can add a digit)
//   k_format_write    one row per lane: convert again and place the bytes.  A workgroup's 256 rows are one contiguous span of
//                     the text: it is built in LDS and stored in 16-byte words where it fits (narrow tables), and written
//                     field by field straight to HBM where it does not.
// Nothing is written unless the whole table can be: a field that cannot be formatted (a finite |x| >= 2^64, a string code
// outside its table) or a capacity that is too small leaves the text untouched and is reported in `status`.
#include "common.hpp"
#include "grid.hpp"
#include "text_format.hpp"
#include <algorithm>
#include <atomic>
#include <cstring>
#include <vector>

namespace mdh {

enum { FMT_F64 = 0, FMT_F32 = 1, FMT_I32 = 2, FMT_I64 = 3, FMT_STR = 4 };
constexpr int FMT_MAX_COLS = 64, FMT_THREADS = 256, FMT_LDS_WORDS = 2048; // 32 KB: rows of up to 128 bytes on average

struct FormatCols {
    const void *col[FMT_MAX_COLS];
    const char *blob[FMT_MAX_COLS]; // coded strings: the names, one after another
    const int *off[FMT_MAX_COLS];   //                name k = blob[off[k] .. off[k + 1])
    int names[FMT_MAX_COLS];
    int kind[FMT_MAX_COLS];
};

static std::atomic<int> g_format_variant{0};

// field (r, c): its length, or -1 when it cannot be formatted; WRITE: its bytes at `out` as well
template <bool WRITE>
__device__ __forceinline__ int format_field(const FormatCols &t, int c, int64_t r, char *out)
{
    const int kind = t.kind[c];
    if (kind == FMT_F64) {
        const uint64_t bits = static_cast<const uint64_t *>(t.col[c])[r];
        return WRITE ? mdtext::format_double(bits, out) : mdtext::format_double_len(bits);
    }
    if (kind == FMT_F32) {
        const uint64_t bits = mdtext::promote_f32_bits(static_cast<const uint32_t *>(t.col[c])[r]);
        return WRITE ? mdtext::format_double(bits, out) : mdtext::format_double_len(bits);
    }
    if (kind == FMT_I32 || kind == FMT_I64) {
        const int64_t v = kind == FMT_I32 ? (int64_t) static_cast<const int *>(t.col[c])[r] : static_cast<const int64_t *>(t.col[c])[r];
        return WRITE ? mdtext::format_int64(v, out) : mdtext::format_int64_len(v);
    }
    const int code = static_cast<const int *>(t.col[c])[r];
    if ((unsigned)code >= (unsigned)t.names[c])
        return -1;
    const int a = t.off[c][code], n = t.off[c][code + 1] - a;
    if (WRITE)
        for (int k = 0; k < n; ++k) out[k] = t.blob[c][a + k];
    return n;
}

__global__ __launch_bounds__(FMT_THREADS) void k_format_measure(int64_t nrows, int ncol, FormatCols t, unsigned *__restrict__ lens,
                                                                 unsigned long long *__restrict__ bad)
{
    const int64_t r = (int64_t)blockIdx.x * FMT_THREADS + threadIdx.x;
    if (r >= nrows)
        return;
    unsigned len = (unsigned)ncol; // the blanks between the fields and the line end
    unsigned refused = 0;
    for (int c = 0; c < ncol; ++c) {
        const int n = format_field<false>(t, c, r, nullptr);
        if (n < 0) ++refused;
        else len += (unsigned)n;
    }
    lens[r] = len;
    if (refused)
        atomicAdd(bad, (unsigned long long)refused);
}

// the text of row r at p (its length is known: the fields are formattable, or this kernel would not run)
__device__ __forceinline__ void write_row(const FormatCols &t, int ncol, int64_t r, char *p)
{
    for (int c = 0; c < ncol; ++c) {
        const int n = format_field<true>(t, c, r, p);
        p += n > 0 ? n : 0;
        *p++ = c + 1 < ncol ? ' ' : '\n';
    }
}

template <bool STAGED>
__global__ __launch_bounds__(FMT_THREADS) void k_format_write(int64_t nrows, int ncol, FormatCols t, const int *__restrict__ offs,
                                                               char *__restrict__ text, int64_t *__restrict__ row_end)
{
    __shared__ uint4 words[STAGED ? FMT_LDS_WORDS : 1];
    const int64_t r0 = (int64_t)blockIdx.x * FMT_THREADS, r = r0 + threadIdx.x;
    const int64_t last = r0 + FMT_THREADS < nrows ? r0 + FMT_THREADS : nrows;
    const int base = offs[r0], span = offs[last] - base; // this workgroup's bytes: text[base .. base + span)
    const bool mine = r < nrows;
    const int at = mine ? offs[r] : 0;
    if (mine)
        row_end[r] = (int64_t)offs[r + 1];
    // the span's image in LDS starts `lead` bytes in, so that 16-byte words of LDS are 16-byte words of the text
    const int lead = (int)((reinterpret_cast<uintptr_t>(text) + (uintptr_t)base) & 15u);
    if (STAGED && lead + span <= FMT_LDS_WORDS * 16) {
        char *image = reinterpret_cast<char *>(words);
        if (mine)
            write_row(t, ncol, r, image + lead + (at - base));
        __syncthreads();
        char *dst = text + base - lead; // 16-byte aligned
        const int nwords = (lead + span + 15) >> 4;
        for (int w = threadIdx.x; w < nwords; w += FMT_THREADS) {
            const int lo = w << 4;
            if (lo >= lead && lo + 16 <= lead + span) {
                *reinterpret_cast<uint4 *>(dst + lo) = words[w];
            } else { // the first and the last word of the span: only the bytes that are this workgroup's
                const int from = lo > lead ? lo : lead, to = lo + 16 < lead + span ? lo + 16 : lead + span;
                for (int k = from; k < to; ++k) dst[k] = image[k];
            }
        }
    } else if (mine) {
        write_row(t, ncol, r, text + at);
    }
}

// what the writers do to positions before they format them: minus the origin, then (ROTATE) times a 3x3 matrix — the rotation
// into LAMMPS' axes, the inverse cell for reduced coordinates.  o_k = ((x - o0) m_0k + (y - o1) m_1k) + (z - o2) m_2k, in this
// order and unfused, so that the host twin of the writers (numpy, the same expression) gives the same bits.
struct ShiftRotate { double o[3], m[9]; };
template <bool ROTATE>
__global__ __launch_bounds__(256) void k_shift_rotate(const double *__restrict__ x, const double *__restrict__ y, const double *__restrict__ z,
                                                      int64_t n, ShiftRotate p, double *__restrict__ ox, double *__restrict__ oy,
                                                      double *__restrict__ oz)
{
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= n)
        return;
    const double a = x[i] - p.o[0], b = y[i] - p.o[1], c = z[i] - p.o[2];
    if (ROTATE) {
        ox[i] = (a * p.m[0] + b * p.m[3]) + c * p.m[6];
        oy[i] = (a * p.m[1] + b * p.m[4]) + c * p.m[7];
        oz[i] = (a * p.m[2] + b * p.m[5]) + c * p.m[8];
    } else {
        ox[i] = a; oy[i] = b; oz[i] = c;
    }
}

} // namespace mdh

using namespace mdh;

extern "C" int mdh_shift_rotate(const double *x, const double *y, const double *z, int64_t N, const double *origin3, const double *matrix9,
                                double *out_x, double *out_y, double *out_z, int space, void *stream)
{
    if (N < 1 || !x || !y || !z || !origin3 || !out_x || !out_y || !out_z) {
        set_error("mdh_shift_rotate: at least one atom, no null pointers (the matrix alone may be null)");
        return MDH_ERR_ARG;
    }
    Scope sc(stream);
    if (sc.failed())
        return sc.error();
    ShiftRotate p;
    for (int k = 0; k < 3; ++k) p.o[k] = origin3[k];
    for (int k = 0; k < 9; ++k) p.m[k] = matrix9 ? matrix9[k] : 0.0;
    const double *dx = sc.stage_in(x, (size_t)N, space), *dy = sc.stage_in(y, (size_t)N, space), *dz = sc.stage_in(z, (size_t)N, space);
    double *ox = sc.stage(out_x, (size_t)N, space, false, true), *oy = sc.stage(out_y, (size_t)N, space, false, true);
    double *oz = sc.stage(out_z, (size_t)N, space, false, true);
    if (sc.failed())
        return sc.error();
    const dim3 grid((unsigned)((N + 255) / 256)), block(256);
    {
        ProfRange pr("k_shift_rotate", sc.stream());
        if (matrix9)
            hipLaunchKernelGGL((k_shift_rotate<true>), grid, block, 0, sc.stream(), dx, dy, dz, N, p, ox, oy, oz);
        else
            hipLaunchKernelGGL((k_shift_rotate<false>), grid, block, 0, sc.stream(), dx, dy, dz, N, p, ox, oy, oz);
    }
    MDH_HIP(hipGetLastError());
    return sc.finish(space);
}

// host twins of the field converters (tests pin them against format() without a GPU): the length, or -1 for "not formatted"
extern "C" int mdh_debug_format_double(double v, char *out32)
{
    union { double d; uint64_t u; } cv;
    cv.d = v;
    return mdtext::format_double(cv.u, out32);
}

extern "C" int mdh_debug_format_float(float v, char *out32)
{
    union { float f; uint32_t u; } cv;
    cv.f = v;
    return mdtext::format_double(mdtext::promote_f32_bits(cv.u), out32);
}

extern "C" int mdh_debug_format_int64(int64_t v, char *out32) { return mdtext::format_int64(v, out32); }

// 0: the library's choice (LDS image where the span fits), 1: always field by field to HBM (what profiles/text_format.md compares)
extern "C" int mdh_debug_set_format_variant(int v)
{
    if (v < 0 || v > 1)
        return MDH_ERR_ARG;
    g_format_variant.store(v);
    return MDH_OK;
}

extern "C" int mdh_format_table(int64_t nrows, int ncol, const int *kinds, const void *const *columns, const char *const *name_blobs,
                                const int *const *name_offsets, const int *name_counts, char *text, int64_t capacity, int64_t *row_end,
                                int64_t *status3, int space, void *stream)
{
    if (nrows < 1 || ncol < 1 || ncol > FMT_MAX_COLS || capacity < 0 || !kinds || !columns || !text || !row_end || !status3) {
        set_error("mdh_format_table: at least one row, 1..64 columns, no null pointers");
        return MDH_ERR_ARG;
    }
    static const size_t width[5] = {8, 4, 4, 8, 4};
    int64_t longest = ncol; // bytes of the longest row this table can have
    size_t name_ints = 0, name_bytes = 0;
    for (int c = 0; c < ncol; ++c) {
        if (kinds[c] < 0 || kinds[c] > 4) {
            set_error("mdh_format_table: column kind must be 0 (f64), 1 (f32), 2 (i32), 3 (i64) or 4 (coded string)");
            return MDH_ERR_ARG;
        }
        if (!columns[c]) {
            set_error("mdh_format_table: null column");
            return MDH_ERR_ARG;
        }
        if (kinds[c] == FMT_STR) {
            if (!name_blobs || !name_offsets || !name_counts || !name_blobs[c] || !name_offsets[c] || name_counts[c] < 1) {
                set_error("mdh_format_table: a coded-string column needs its table of names");
                return MDH_ERR_ARG;
            }
            const int *off = name_offsets[c];
            int widest = 0;
            for (int k = 0; k < name_counts[c]; ++k) {
                if (off[0] < 0 || off[k + 1] < off[k]) {
                    set_error("mdh_format_table: name offsets must start at 0 or above and never decrease");
                    return MDH_ERR_ARG;
                }
                widest = std::max(widest, off[k + 1] - off[k]);
            }
            longest += widest;
            name_ints += (size_t)name_counts[c] + 1;
            name_bytes += (size_t)off[name_counts[c]];
        } else {
            longest += kinds[c] <= FMT_F32 ? mdtext::FMT_DOUBLE_MAX : kinds[c] == FMT_I32 ? mdtext::FMT_INT32_MAX : mdtext::FMT_INT64_MAX;
        }
    }
    if (nrows > 2147483647LL / longest) { // (offsets are 32-bit: the caller formats a larger table in chunks of rows)
        set_error("mdh_format_table: too many rows for one call (row offsets are 32-bit); format the table in chunks");
        return MDH_ERR_ARG;
    }
    status3[0] = status3[1] = status3[2] = 0;
    Scope sc(stream);
    if (sc.failed())
        return sc.error();
    hipStream_t st = sc.stream();
    FormatCols t;
    for (int c = 0; c < FMT_MAX_COLS; ++c) { t.col[c] = nullptr; t.blob[c] = nullptr; t.off[c] = nullptr; t.names[c] = 0; t.kind[c] = FMT_I32; }
    // the tables of names of all string columns in one upload: the offsets of each, then the bytes of each
    std::vector<int> packed(name_ints + (name_bytes + 3) / 4 + 1, 0);
    int *dnames = sc.alloc_n<int>(packed.size());
    if (sc.failed())
        return sc.error();
    {
        size_t ints = 0, bytes = 0;
        char *blob0 = reinterpret_cast<char *>(packed.data() + name_ints);
        for (int c = 0; c < ncol; ++c) {
            if (kinds[c] != FMT_STR)
                continue;
            const int n = name_counts[c], first = name_offsets[c][0], total = name_offsets[c][n] - first;
            for (int k = 0; k <= n; ++k) packed[ints + k] = name_offsets[c][k] - first;
            memcpy(blob0 + bytes, name_blobs[c] + first, (size_t)total);
            t.off[c] = dnames + ints;
            t.blob[c] = reinterpret_cast<const char *>(dnames + name_ints) + bytes;
            t.names[c] = n;
            ints += (size_t)n + 1;
            bytes += (size_t)total;
        }
    }
    if (name_ints)
        MDH_HIP(hipMemcpyAsync(dnames, packed.data(), packed.size() * sizeof(int), hipMemcpyHostToDevice, st));
    for (int c = 0; c < ncol; ++c) {
        t.kind[c] = kinds[c];
        t.col[c] = sc.stage_in(static_cast<const unsigned char *>(columns[c]), (size_t)nrows * width[kinds[c]], space);
    }
    char *dtext = sc.stage(text, (size_t)capacity, space, true, true); // (host space: what is not written keeps its content)
    int64_t *dend = sc.stage(row_end, (size_t)nrows, space, true, true);
    unsigned *lens = sc.alloc_n<unsigned>((size_t)nrows + 1);
    int *offs = sc.alloc_n<int>((size_t)nrows + 2);
    unsigned long long *dbad = sc.alloc_n<unsigned long long>(1);
    if (sc.failed())
        return sc.error();
    MDH_HIP(hipMemsetAsync(dbad, 0, sizeof(unsigned long long), st));
    const dim3 grid((unsigned)((nrows + FMT_THREADS - 1) / FMT_THREADS)), block(FMT_THREADS);
    {
        ProfRange pr("k_format_measure", st);
        hipLaunchKernelGGL(k_format_measure, grid, block, 0, st, nrows, ncol, t, lens, dbad);
    }
    MDH_TRY(exclusive_scan_u32(sc, lens, offs, nrows)); // offs[nrows] = bytes of the whole table
    int total = 0;
    unsigned long long bad = 0;
    MDH_HIP(hipMemcpyAsync(&total, offs + nrows, sizeof(int), hipMemcpyDeviceToHost, st));
    MDH_HIP(hipMemcpyAsync(&bad, dbad, sizeof(bad), hipMemcpyDeviceToHost, st));
    MDH_HIP(hipStreamSynchronize(st)); // (the host decides whether anything is written at all)
    status3[0] = (int64_t)total;       // bytes of the table (of its formattable fields when [1] is not zero)
    status3[1] = (int64_t)bad;         // fields that cannot be formatted
    status3[2] = bad == 0 && (int64_t)total > capacity ? (int64_t)total : 0; // the capacity this table needs, when the given one is too small
    if (bad == 0 && (int64_t)total <= capacity) {
        ProfRange pr("k_format_write", st);
        if (g_format_variant.load() == 1)
            hipLaunchKernelGGL((k_format_write<false>), grid, block, 0, st, nrows, ncol, t, offs, dtext, dend);
        else
            hipLaunchKernelGGL((k_format_write<true>), grid, block, 0, st, nrows, ncol, t, offs, dtext, dend);
        MDH_HIP(hipGetLastError());
    }
    return sc.finish(space);
}

MDH_WARM_UNIT(text_format)
