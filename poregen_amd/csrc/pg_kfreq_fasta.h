// pg_kfreq_fasta.h -- the FASTA walk of `poregen kmer_freq`, shared by the kernels (pg_kfreq.hip: k_kf_fa_lines, k_kf_fa_count) and the
// host test shim (pg_hosttest.cpp), which runs the same span / tile / unit decomposition on the CPU.
//
// Rules (include/pgmove.h, pg_kfreq_submit_fasta): lines end at '\n' only; a line whose first byte is '>' is a header line, every other
// line a sequence line; a record's sequence is the bytes of a maximal run of sequence lines, newlines dropped; every k-byte window of a
// record's sequence is a key. So the state a sequential walk holds at a byte is
//   * the kind of the open line: header, sequence, or "fresh" (the line starts at this very byte, its kind is this byte's), and
//   * the last <= k - 1 sequence bytes of the open record (k <= 12: at most kFaTail = 11 bytes), however many line ends lie between them.
// The second part is a monoid: a stretch of bytes either holds a header line (it "resets": what was in front does not matter, the tail is
// what follows the last header) or it does not (its sequence bytes are appended to what was in front). PgFaSum is one element; spans,
// tiles and units are scanned with pg_fa_compose. The kind of the first line fragment of a stretch is not known inside the stretch, so a
// stretch is summarised in two parts -- `fa`, the bytes in front of its first newline taken as sequence, and `pb`, everything behind
// it, where every line starts inside the stretch and its kind is known -- and resolved (pg_fa_resolve) once a prefix maximum over
// the line starts has told where the open line began: its kind is the byte there (pg_fa_kind_at).
#pragma once
#include <stdint.h>

#if defined(__HIPCC__)
#define PG_FA_HD __host__ __device__ __forceinline__
#else
#define PG_FA_HD static inline
#endif

enum { PG_FA_FRESH = 0, PG_FA_SEQ = 1, PG_FA_HDR = 2 }; // FRESH = 0: a zeroed carried state is the start of a stream
enum { kFaTail = 11, kFaSpan = 128, kFaTileSpans = 256 };

PG_FA_HD int pg_kf_base_code(uint32_t c) {
    return c == 'A' ? 0 : c == 'C' ? 1 : c == 'G' ? 2 : c == 'T' ? 3 : -1;
}

struct PgFaSum {
    uint64_t lo;   // the newest 8 bytes, newest in the lowest byte
    uint32_t hi;   // the 3 bytes in front of them (low 24 bits)
    uint32_t meta; // number of bytes held (0..kFaTail) | 0x100 if a header line lies in the stretch
};

PG_FA_HD PgFaSum pg_fa_empty() { PgFaSum s; s.lo = 0; s.hi = 0; s.meta = 0; return s; }
PG_FA_HD PgFaSum pg_fa_reset() { PgFaSum s; s.lo = 0; s.hi = 0; s.meta = 0x100; return s; }
PG_FA_HD uint32_t pg_fa_count(const PgFaSum &s) { return s.meta & 0xff; }

PG_FA_HD void pg_fa_append(PgFaSum &s, uint32_t c) {
    s.hi = ((s.hi << 8) | (uint32_t)(s.lo >> 56)) & 0xffffffu;
    s.lo = (s.lo << 8) | c;
    if ((s.meta & 0xff) < kFaTail) s.meta++;
}

// byte j of the tail, j = 0 the newest
PG_FA_HD uint32_t pg_fa_byte(const PgFaSum &s, uint32_t j) {
    return j < 8 ? (uint32_t)(s.lo >> (8 * j)) & 0xff : (s.hi >> (8 * (j - 8))) & 0xff;
}

// a then b
PG_FA_HD PgFaSum pg_fa_compose(const PgFaSum &a, const PgFaSum &b) {
    if (b.meta & 0x100) return b;
    const uint32_t nb = b.meta & 0xff;
    if (nb == 0) return a;
    PgFaSum r;
    const uint32_t sh = 8 * nb; // a's bytes move up by b's: 8..88 bits of a 88-bit value
    if (sh < 64) {
        r.lo = (a.lo << sh) | b.lo;
        r.hi = ((uint32_t)(((uint64_t)a.hi << sh) | (a.lo >> (64 - sh))) | b.hi) & 0xffffffu;
    } else {
        r.lo = b.lo;
        r.hi = ((uint32_t)(a.lo << (sh - 64)) | b.hi) & 0xffffffu;
    }
    const uint32_t n = (a.meta & 0xff) + nb;
    r.meta = (n < kFaTail ? n : (uint32_t)kFaTail) | (a.meta & 0x100);
    return r;
}

// One span (or any stretch held as little-endian words): `lim` valid bytes.
struct PgFaSpan {
    PgFaSum fa;        // the bytes in front of the first newline (all of them, if there is none), taken as sequence
    PgFaSum pb;        // everything behind the first newline, kinds resolved; empty if there is no newline
    uint32_t has_nl;
    uint32_t last_nl;  // index of the last newline
};

template <int kWords>
PG_FA_HD void pg_fa_span_summary(const uint32_t (&w)[kWords], uint32_t lim, PgFaSpan &out) {
    PgFaSum acc = pg_fa_empty();
    out.fa = acc; out.pb = acc; out.has_nl = 0; out.last_nl = 0;
    bool fresh = false, hdr = false;
#if defined(__HIPCC__)
#pragma unroll
#endif
    for (uint32_t i = 0; i < 4 * (uint32_t)kWords; i++) {
        if (i >= lim) break;
        const uint32_t c = (w[i >> 2] >> (8 * (i & 3))) & 0xff;
        if (c == '\n') {
            if (!out.has_nl) { out.fa = acc; acc = pg_fa_empty(); out.has_nl = 1; }
            out.last_nl = i;
            fresh = true;
            continue;
        }
        if (fresh) { fresh = false; hdr = c == '>'; if (hdr) acc = pg_fa_reset(); }
        if (!hdr) pg_fa_append(acc, c);
    }
    if (out.has_nl) out.pb = acc; else out.fa = acc;
}

// The kind of the line open at byte `at` of the unit p (at <= the unit's length), where `line_start` is the offset behind the last newline
// in front of `at` (0: the unit holds none there, the line is the one the carried state `carried` describes). Never reads p[at].
PG_FA_HD uint32_t pg_fa_kind_at(const uint8_t *p, uint64_t line_start, uint64_t at, uint32_t carried) {
    if (line_start == 0) {
        if (carried != PG_FA_FRESH) return carried;
        if (at == 0) return PG_FA_FRESH;
        return p[0] == '>' ? PG_FA_HDR : PG_FA_SEQ;
    }
    if (line_start == at) return PG_FA_FRESH;
    return p[line_start] == '>' ? PG_FA_HDR : PG_FA_SEQ;
}

// A stretch's effect on the record tail, given the kind of the line open at its first byte (and that byte, for a fresh line). A header in
// front resets: more than once does no harm, nothing of a header line is ever appended.
PG_FA_HD PgFaSum pg_fa_resolve(uint32_t kind_in, uint32_t first_byte, const PgFaSum &fa, const PgFaSum &pb) {
    const bool hdr = kind_in == PG_FA_FRESH ? first_byte == '>' : kind_in == PG_FA_HDR;
    return pg_fa_compose(hdr ? pg_fa_reset() : fa, pb);
}

// The count walk over one span of `lim` bytes: `load(ch, ws)` gives bytes [16 ch, 16 ch + 16) as four words, `kind_in` and `rec` are the
// sequential walk's state at the span's first byte. Every window that ends in the span goes to sink.dense(code) or sink.odd(lo, hi)
// (the window's bytes, newest in the lowest byte of lo). Returns whether a sequence line holds a NUL byte.
template <class Load, class Sink>
PG_FA_HD bool pg_fa_walk(Load &load, uint32_t lim, uint32_t k, uint32_t kind_in, const PgFaSum &rec, Sink &sink) {
    const uint32_t mask = (1u << (2 * k)) - 1;
    uint32_t len = 0, run = 0, code = 0;
    uint64_t lo = 0; uint32_t hi = 0;
    const uint32_t have = pg_fa_count(rec);
    for (uint32_t j = have < k - 1 ? have : k - 1; j-- > 0;) { // warm-up: the open record's last min(k - 1, length) bytes
        const uint32_t c = pg_fa_byte(rec, j);
        const int b = pg_kf_base_code(c);
        len++;
        run = b >= 0 ? run + 1 : 0;
        code = ((code << 2) | (uint32_t)(b & 3)) & mask;
        hi = (hi << 8) | (uint32_t)(lo >> 56); lo = (lo << 8) | c;
    }
    bool fresh = kind_in == PG_FA_FRESH, hdr = kind_in == PG_FA_HDR, bad = false;
    for (uint32_t ch = 0; ch < kFaSpan / 16; ch++) {
        if (ch * 16 >= lim) break;
        uint32_t ws[4];
        load(ch, ws);
#if defined(__HIPCC__)
#pragma unroll
#endif
        for (uint32_t j = 0; j < 16; j++) {
            if (ch * 16 + j >= lim) break;
            const uint32_t c = (ws[j >> 2] >> (8 * (j & 3))) & 0xff;
            if (fresh) { fresh = false; hdr = c == '>'; if (hdr) { len = 0; run = 0; } }
            if (c == '\n') { fresh = true; continue; } // the record goes on: no reset
            if (hdr) continue;
            bad |= c == 0;
            len++;
            const int b = pg_kf_base_code(c);
            run = b >= 0 ? run + 1 : 0;
            code = ((code << 2) | (uint32_t)(b & 3)) & mask;
            hi = (hi << 8) | (uint32_t)(lo >> 56); lo = (lo << 8) | c;
            if (len >= k) {
                if (run >= k) sink.dense(code);
                else sink.odd(lo, hi);
            }
        }
    }
    return bad;
}
