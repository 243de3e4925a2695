// text_sections.hpp — does a line of a LAMMPS data file start a section?  Written once for host and device.
//
// Input side of the hot path (reference: src/mdapy/load_save.py:1064-1092 — every line is stripped and split,
// and a line whose first token is one of the section words starts that section, the first such line counting).  Here a line is
// looked at where it lies: blanks are skipped, the first byte rejects nearly every line (rows begin with a digit or a sign, a
// comment with '#'), and what is left is compared with the few words that begin with that byte.  A token ends at a blank, at
// the end of the line or at the end of the text, so `Atoms#atomic` and `Atomsx` are no section starts and `Atoms\r` is one.
#pragma once
#include <stdint.h>

#ifdef __HIPCC__
#define SEC_HD __host__ __device__ __forceinline__
#else
#define SEC_HD inline
#endif

namespace mdtext {

constexpr int SEC_MAX_WORDS = 32, SEC_MAX_LEN = 15;

// the keyword table, passed to the kernel by value
struct SectionWords {
    int n;
    unsigned lo, hi;                   // the smallest and the largest first byte of a word
    unsigned first[8];                 // bit b set: some word begins with byte b
    unsigned char len[SEC_MAX_WORDS];
    char w[SEC_MAX_WORDS][SEC_MAX_LEN + 1];
};

// false: a word is empty or too long, or there are too many
inline bool section_words_init(SectionWords &t, const char *const *words, int nwords)
{
    if (!words || nwords < 1 || nwords > SEC_MAX_WORDS)
        return false;
    t.n = nwords;
    t.lo = 255u;
    t.hi = 0u;
    for (int k = 0; k < 8; ++k) t.first[k] = 0u;
    for (int k = 0; k < SEC_MAX_WORDS; ++k) {
        t.len[k] = 0;
        for (int j = 0; j <= SEC_MAX_LEN; ++j) t.w[k][j] = 0;
    }
    for (int k = 0; k < nwords; ++k) {
        const char *s = words[k];
        if (!s)
            return false;
        int n = 0;
        while (s[n]) {
            if (n == SEC_MAX_LEN || s[n] == ' ' || s[n] == '\t' || s[n] == '\r' || s[n] == '\n')
                return false;
            t.w[k][n] = s[n];
            ++n;
        }
        if (n == 0)
            return false;
        t.len[k] = (unsigned char)n;
        const unsigned b = (unsigned char)s[0];
        t.first[b >> 5] |= 1u << (b & 31);
        t.lo = b < t.lo ? b : t.lo;
        t.hi = b > t.hi ? b : t.hi;
    }
    return true;
}

SEC_HD bool sec_blank(char c) { return c == ' ' || c == '\t' || c == '\r'; }

// the line that starts at byte `at` of text[0 .. nbytes): index of the word its first token is, or -1
SEC_HD int match_section(const char *text, int64_t at, int64_t nbytes, const SectionWords &t)
{
    while (at < nbytes && sec_blank(text[at])) ++at;
    if (at >= nbytes)
        return -1;
    const unsigned b = (unsigned char)text[at];
    if (!((t.first[b >> 5] >> (b & 31)) & 1u))
        return -1;
    for (int k = 0; k < t.n; ++k) {
        const int n = t.len[k];
        if ((unsigned char)t.w[k][0] != b || at + n > nbytes)
            continue;
        int j = 1;
        while (j < n && text[at + j] == t.w[k][j]) ++j;
        if (j < n)
            continue;
        if (at + n == nbytes)
            return k;
        const char e = text[at + n];
        if (sec_blank(e) || e == '\n')
            return k;
    }
    return -1;
}

} // namespace mdtext
