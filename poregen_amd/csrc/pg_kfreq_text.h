// pg_kfreq_text.h -- the FASTQ walk of `poregen kmer_freq`, shared by the kernels (pg_kfreq.hip: k_kf_lines, k_kf_count) and the host test
// shim (pg_hosttest.cpp), which runs the same span / tile / unit decomposition on the CPU.
//
// Rules (pg_kfreq.hip has them with the reference's lines): lines end after each '\n'; line i is a sequence line iff i % 4 == 1; a window
// of k bytes ending at stream offset e is counted iff it holds no '\n', its line is a sequence line and e is not the last byte of the
// stream. A unit of n bytes is cut into tiles of PG_KF_TILE bytes (one workgroup) and spans of PG_KF_SPAN bytes (one thread). A thread is
// given the line index mod 4 at its first byte and walks its span after k - 1 bytes of warm-up inside the unit (pg_kf_walk); it leaves
// the window that ends on the unit's last byte alone. The windows that start in front of the unit, and that one window of the unit
// before, are the seam's (pg_kf_seam), which also forms the state the next unit starts from (KfState).
// Both are written over a sink: dense(code) takes an ACGT window (2-bit codes, first base most significant), odd(lo, hi) any other (its
// bytes, newest in the lowest byte of lo; pg_kf_odd_key puts them in key order).
#pragma once
#include <stdint.h>
#include "pg_kfreq_fasta.h" // pg_kf_base_code

#if defined(__HIPCC__)
#define PG_KF_HD __host__ __device__ __forceinline__
#else
#define PG_KF_HD static inline
#endif

#define PG_KF_THREADS 256                                     // threads of a workgroup: spans per tile
#define PG_KF_SPAN 128                                        // bytes per thread
#define PG_KF_TILE ((uint64_t)PG_KF_THREADS * PG_KF_SPAN)     // 32 KiB per workgroup
#define PG_KF_UNIT (16ull << 20)                              // bytes per unit (512 tiles)
#define PG_KF_MAX_K 12u
#define PG_KF_LDS_MAX_K 6u                                    // 4^6 u32 = 16 KiB of LDS
#define PG_KF_ODD_LDS 512u                                    // odd windows a workgroup stages in LDS

struct KfState {       // carried across units; two slots, unit u reads slot u&1 and writes slot (u+1)&1
    uint32_t mod4;     // index mod 4 of the line open at the unit's first byte
    uint32_t tail_len; // bytes of that line already seen, capped at k (all of them, if fewer)
    uint8_t tail[16];  // its last tail_len bytes, oldest first
};

// The smaller of two byte counts of different integer types. Under hipcc this is HIP's min over mixed types, as the kernels have always
// had it: it compares the two as doubles, which is exact below 2^53 (a unit has at most 2^24 bytes). Left as it is, so that moving the
// walk into this header leaves the kernels' code what it was.
#if defined(__HIPCC__)
#define PG_KF_MIN(a, b) min<uint64_t>(a, b)
#else
#define PG_KF_MIN(a, b) ((uint64_t)(a) < (uint64_t)(b) ? (uint64_t)(a) : (uint64_t)(b))
#endif

// lo/hi: the window's bytes, newest in the lowest byte of lo; key: the same bytes oldest first, four to a little-endian word, zero padded
PG_KF_HD void pg_kf_odd_key(uint64_t lo, uint32_t hi, uint32_t k, uint32_t (&key)[4]) {
    key[0] = key[1] = key[2] = key[3] = 0;
    for (uint32_t i = 0; i < k; i++) {
        const uint32_t sh = k - 1 - i; // byte i of the key is sh bytes older than the newest
        const uint32_t b = sh < 8 ? (uint32_t)(lo >> (8 * sh)) & 0xff : (hi >> (8 * (sh - 8))) & 0xff;
        key[i >> 2] |= b << (8 * (i & 3));
    }
}

// The count walk over the span that starts at byte `base` of the unit p[0, n) (base < n): `load(ch, ws)` gives the span's bytes
// [16 ch, 16 ch + 16) as four words, zero past n; `mod4` is the index mod 4 of the line open at the span's first byte. Every counted
// window that ends in the span goes to the sink. Returns whether a sequence line holds a NUL byte in this span.
template <class Load, class Sink>
PG_KF_HD bool pg_kf_walk(const uint8_t *__restrict__ p, uint64_t base, uint64_t n, uint32_t k, uint32_t mod4, Load &load, Sink &sink) {
    const uint64_t mask = (1u << (2 * k)) - 1;
    // warm-up: the k-1 bytes in front of this thread's span (inside the unit; earlier ones are the seam's)
    uint32_t len = 0, run = 0, code = 0;
    uint64_t lo = 0; uint32_t hi = 0;
    const uint64_t w0 = base >= k - 1 ? base - (k - 1) : 0;
    for (uint64_t q = w0; q < base; q++) {
        const uint32_t c = p[q];
        if (c == '\n') { len = 0; run = 0; continue; }
        len++;
        const int b = pg_kf_base_code(c);
        run = b >= 0 ? run + 1 : 0;
        code = (code << 2) | (uint32_t)(b & 3);
        hi = (hi << 8) | (uint32_t)(lo >> 56); lo = (lo << 8) | c;
    }
    bool bad = false;
    const uint32_t lim = (uint32_t)PG_KF_MIN(PG_KF_SPAN, n - base);
    // the last byte of the unit is not an end of a counted window here: the seam of the next unit (or finish) settles it
    const uint32_t last_ok = base + lim == n ? lim - 1 : lim;
    for (uint32_t ch = 0; ch < PG_KF_SPAN / 16; ch++) {
        if (ch * 16 >= lim) break;
        uint32_t ws[4];
        load(ch, ws);
#if defined(__HIPCC__)
#pragma unroll
#endif
        for (uint32_t j = 0; j < 16; j++) {
            const uint32_t i = ch * 16 + j;
            if (i >= lim) break;
            const uint32_t c = (ws[j >> 2] >> (8 * (j & 3))) & 0xff;
            if (c == '\n') { mod4 = (mod4 + 1) & 3; len = 0; run = 0; continue; }
            const bool seq = mod4 == 1;
            bad |= seq && c == 0;
            len++;
            const int b = pg_kf_base_code(c);
            run = b >= 0 ? run + 1 : 0;
            code = ((code << 2) | (uint32_t)(b & 3)) & (uint32_t)mask;
            hi = (hi << 8) | (uint32_t)(lo >> 56); lo = (lo << 8) | c;
            if (seq && len >= k && i < last_ok) {
                if (run >= k) sink.dense(code);
                else sink.odd(lo, hi);
            }
        }
    }
    return bad;
}

// One thread per unit: the windows that start in the carried tail of `s` and end in this unit p[0, n) go to the sink; returns the state
// the next unit starts from. total_nl: the newlines of the whole unit.
template <class Sink>
PG_KF_HD KfState pg_kf_seam(const KfState &s, const uint8_t *__restrict__ p, uint64_t n, uint32_t k, uint32_t total_nl, Sink &sink) {
    uint8_t v[2 * PG_KF_MAX_K];
    const uint32_t t = s.tail_len;
    const uint32_t head = (uint32_t)PG_KF_MIN(n, k - 1);
    for (uint32_t i = 0; i < t; i++) v[i] = s.tail[i];
    for (uint32_t i = 0; i < head; i++) v[t + i] = p[i];
    // window ending at v[e]: e >= k-1 (whole), e <= t+k-2 (starts in the tail), e <= t+n-2 (not the stream's last byte so far)
    if (s.mod4 == 1 && t >= 1) { // (k = 1: only the window of the tail's byte, left open by the last unit)
        const uint64_t e_hi = PG_KF_MIN(t + k - 2, t + n - 2);
        for (uint64_t e = k - 1; e <= e_hi; e++) {
            bool nl = false, acgt = true;
            uint32_t code = 0;
            uint64_t lo = 0; uint32_t hi = 0;
            for (uint32_t j = 0; j < k; j++) {
                const uint32_t c = v[e + 1 - k + j];
                nl |= c == '\n';
                const int b = pg_kf_base_code(c);
                acgt &= b >= 0;
                code = (code << 2) | (uint32_t)(b & 3);
                hi = (hi << 8) | (uint32_t)(lo >> 56); lo = (lo << 8) | c;
            }
            if (nl) break; // every later window holds the same newline
            if (acgt) sink.dense(code);
            else sink.odd(lo, hi);
        }
    }
    // the next state: the open line's last <= k bytes
    KfState o;
    o.mod4 = (s.mod4 + total_nl) & 3;
    int64_t nl = -1; // last newline among the unit's last min(n, k) bytes
    for (uint64_t i = n; i > 0 && n - i < k; i--)
        if (p[i - 1] == '\n') { nl = (int64_t)i - 1; break; }
    uint8_t cat[2 * PG_KF_MAX_K];
    uint32_t m = 0;
    if (nl < 0 && n < k) for (uint32_t i = 0; i < t; i++) cat[m++] = s.tail[i]; // the whole unit continues the open line
    for (uint64_t i = nl >= 0 ? (uint64_t)nl + 1 : (n > k ? n - k : 0); i < n; i++) cat[m++] = p[i];
    const uint32_t keep = m < k ? m : k;
    o.tail_len = keep;
    for (uint32_t i = 0; i < 16; i++) o.tail[i] = i < keep ? cat[m - keep + i] : 0;
    return o;
}
