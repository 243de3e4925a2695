// text_format.hpp — IEEE double / float / integer -> decimal text, written once for host and device.
//
// Output side of the hot path (reference: src/mdapy/load_save.py:1534-2017 — every writer hands its atom
// table to a CSV writer with separator " ", no header and float_precision=10, so every float field is what Python's
// format(v, ".10f") gives: fixed notation, ten decimals, the exact binary value rounded half-to-even).  The inverse of
// text_parse.hpp, and like it exact: integer arithmetic only, no table, no 128-bit division.
//
//   |x| = m * 2^e  (m < 2^53)  is split into  I + f  exactly; for e < 0, with s = -e,
//   f * 10^10 = (m mod 2^s) * 5^10 / 2^(s - 10):   the product is below 2^77 (two 64-bit words), the division a shift whose
//   dropped bits decide the rounding (above half: up; exactly half: to even); a fraction that reaches 10^10 carries into I.
//
// Every finite |x| < 2^64 is formatted (at most 32 bytes: sign, 20 digits, the point, 10 decimals); -0.0 and negatives that
// round to zero keep their sign, as format() does; non-finite values are "NaN", "inf" and "-inf" (the CSV writer's spelling,
// which this package's reader reads back); a finite |x| >= 2^64 is refused (the caller counts it and formats on the host).
#pragma once
#include "text_parse.hpp"

namespace mdtext {

constexpr int FMT_DOUBLE_MAX = 32, FMT_INT32_MAX = 11, FMT_INT64_MAX = 20;
constexpr uint64_t FMT_TEN10 = 10000000000ull, FMT_FIVE10 = 9765625ull;
enum { FMT_FINITE = 0, FMT_NAN = 1, FMT_INF = 2, FMT_REFUSED = 3 };

// bits of a double -> sign, integer part, ten decimals as an integer below 10^10 (FMT_FINITE), or what the value is instead
TXT_HD int split_fixed10(uint64_t bits, bool *neg, uint64_t *ip, uint64_t *frac)
{
    const int be = (int)((bits >> 52) & 0x7FF);
    uint64_t m = bits & (((uint64_t)1 << 52) - 1);
    *neg = (bits >> 63) != 0;
    *ip = 0;
    *frac = 0;
    if (be == 0x7FF)
        return m ? FMT_NAN : FMT_INF;
    if (be)
        m |= (uint64_t)1 << 52;
    const int e = (be ? be : 1) - 1075; // |x| = m * 2^e
    if (e >= 0) {
        if (e > 11)
            return FMT_REFUSED; // 2^64 and beyond
        *ip = m << e;
        return FMT_FINITE;
    }
    const int s = -e; // 1 .. 1074
    uint64_t I = 0, mf = m;
    if (s < 64) {
        I = m >> s;
        mf = m & (((uint64_t)1 << s) - 1);
    }
    uint64_t hi, lo;
    mul64(mf, FMT_FIVE10, &hi, &lo); // P = mf * 5^10 < 2^77
    const int t = s - 10;            // f * 10^10 = P / 2^t
    uint64_t F;
    if (t <= 0) {
        F = lo << -t; // (mf < 2^10 here: exact, one word)
    } else if (t >= 78) {
        F = 0; // P < 2^77 <= 2^(t-1): below half
    } else {
        uint64_t q, rem_hi, rem_lo, half_hi, half_lo;
        if (t < 64) {
            q = (lo >> t) | (hi << (64 - t)); // (the quotient is below 10^10: the bits of hi above it are zero)
            rem_hi = 0;
            rem_lo = lo & (((uint64_t)1 << t) - 1);
            half_hi = 0;
            half_lo = (uint64_t)1 << (t - 1);
        } else {
            const int u = t - 64; // 0 .. 13
            q = hi >> u;
            rem_hi = hi & (((uint64_t)1 << u) - 1);
            rem_lo = lo;
            half_hi = u ? (uint64_t)1 << (u - 1) : 0;
            half_lo = u ? 0 : (uint64_t)1 << 63;
        }
        const bool above = rem_hi > half_hi || (rem_hi == half_hi && rem_lo > half_lo);
        const bool tie = rem_hi == half_hi && rem_lo == half_lo;
        F = q + ((above || (tie && (q & 1))) ? 1 : 0);
    }
    if (F >= FMT_TEN10) { // 0.99999999995 -> 1.0000000000
        F -= FMT_TEN10;
        ++I;
    }
    *ip = I;
    *frac = F;
    return FMT_FINITE;
}

// a float's bits -> the bits of the double of the same value (exact; integer work, so that no rounding or flush mode matters)
TXT_HD uint64_t promote_f32_bits(uint32_t b)
{
    const uint64_t sign = (uint64_t)(b >> 31) << 63;
    int e = (int)((b >> 23) & 0xFF);
    uint32_t m = b & 0x7FFFFFu;
    if (e == 0xFF)
        return sign | 0x7FF0000000000000ull | ((uint64_t)m << 29);
    if (e == 0) {
        if (m == 0)
            return sign;
        const int up = clz64((uint64_t)m) - 40; // shift that brings the leading bit to bit 23
        m = (m << up) & 0x7FFFFFu;
        e = 1 - up;
    }
    return sign | ((uint64_t)(e - 127 + 1023) << 52) | ((uint64_t)m << 29);
}

TXT_HD int dec_digits(uint64_t v)
{
    int n = 1;
    uint64_t p = 10;
    while (n < 20 && v >= p) {
        p *= 10;
        ++n;
    }
    return n;
}

// the n = dec_digits(v) digits of v at out[0 .. n)
TXT_HD void put_dec(char *out, uint64_t v, int n)
{
    int k = n;
    while (v >> 32) { // (64-bit divisions only while the value needs them)
        const uint64_t q = v / 10;
        out[--k] = (char)('0' + (int)(v - q * 10));
        v = q;
    }
    uint32_t w = (uint32_t)v;
    while (k > 0) {
        const uint32_t q = w / 10;
        out[--k] = (char)('0' + (int)(w - q * 10));
        w = q;
    }
}

// exactly `width` digits of v (v < 10^width, width <= 9), zero padded
TXT_HD void put_padded(char *out, uint32_t v, int width)
{
    for (int k = width - 1; k >= 0; --k) {
        const uint32_t q = v / 10;
        out[k] = (char)('0' + (int)(v - q * 10));
        v = q;
    }
}

// length of format(x, ".10f") for the double with these bits (3 / 4 for the non-finite spellings); -1: refused
TXT_HD int format_double_len(uint64_t bits)
{
    bool neg;
    uint64_t ip, frac;
    const int what = split_fixed10(bits, &neg, &ip, &frac);
    if (what == FMT_REFUSED)
        return -1;
    if (what == FMT_NAN)
        return 3;
    if (what == FMT_INF)
        return neg ? 4 : 3;
    return (neg ? 1 : 0) + dec_digits(ip) + 11;
}

// the same, writing the bytes (at most FMT_DOUBLE_MAX, no terminator); nothing is written for a refused value
TXT_HD int format_double(uint64_t bits, char *out)
{
    bool neg;
    uint64_t ip, frac;
    const int what = split_fixed10(bits, &neg, &ip, &frac);
    if (what == FMT_REFUSED)
        return -1;
    if (what == FMT_NAN) {
        out[0] = 'N'; out[1] = 'a'; out[2] = 'N';
        return 3;
    }
    int at = 0;
    if (neg)
        out[at++] = '-';
    if (what == FMT_INF) {
        out[at] = 'i'; out[at + 1] = 'n'; out[at + 2] = 'f';
        return at + 3;
    }
    const int n = dec_digits(ip);
    put_dec(out + at, ip, n);
    at += n;
    out[at++] = '.';
    const uint32_t top = (uint32_t)(frac / 100000u); // frac < 10^10: two halves of five digits
    put_padded(out + at, top, 5);
    put_padded(out + at + 5, (uint32_t)(frac - (uint64_t)top * 100000u), 5);
    return at + 10;
}

TXT_HD int format_int64_len(int64_t v)
{
    const uint64_t mag = v < 0 ? (uint64_t)0 - (uint64_t)v : (uint64_t)v; // (INT64_MIN: its magnitude is 2^63, no overflow)
    return (v < 0 ? 1 : 0) + dec_digits(mag);
}

TXT_HD int format_int64(int64_t v, char *out)
{
    const uint64_t mag = v < 0 ? (uint64_t)0 - (uint64_t)v : (uint64_t)v;
    int at = 0;
    if (v < 0)
        out[at++] = '-';
    const int n = dec_digits(mag);
    put_dec(out + at, mag, n);
    return at + n;
}

} // namespace mdtext
