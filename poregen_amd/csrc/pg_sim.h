// pg_sim.h -- the rule of `poregen simulate`: raw signal and the alignment that is true by construction, drawn from a k-mer model. Plain
// C++ that the kernels (pg_sim.hip), the library's host side, the command and a host test (pg_hosttest.cpp: pgt_sim_*) all compile. Not
// installed. This is the project's own rule, the inverse of fit's (pg_fit.h); it is not squigulator's algorithm.
//
// Random numbers. Philox4x32-10, key (seed_lo, seed_hi), counter (i, stream, read_lo, read_hi) with read the GLOBAL number of the read
// (first_read + r). Stream 0: per read (i = 0: the offset, i = 1: the command's read drawing); stream 1: the dwell of op i; stream 2:
// sample i of the read. Every draw is addressed, so nothing depends on how the work is cut into batches, pieces or lanes.
//
// Tables, per slot (a k-mer's rank in ACGT order): level in 1e-3 pA, 0 < level < 2^18, 0 = the k-mer has no level; stdv in 1e-3 pA,
// 0 <= stdv < 2^18; dwell in samples, 1 .. 2^12.
//
// Events. A read of Lb bases has Lb events; event e takes the slot of the k-mer at i = clamp(e - m, 0, Lb - k): seq[i, i + k), or
// seq[Lb - i - k, Lb - i) with rna (U reads as T). Refused, in this order: Lb < k (too_short); a letter of the read outside ACGTU
// (bad_base); an event whose k-mer has no level (no_level). A refused read has no ops and no samples.
//
// Dwell. D the slot's dwell: w = D spread_pct div 100, lo = max(1, D - w), hi = D + w, n_e = lo + ((x0 (hi - lo + 1)) >> 32), x0 of
// stream 1, i = e.       hi <= 2^13: 256 ops of a piece stay below 2^21 samples.
//
// Samples. `lead` samples under (lead_level, lead_stdv), then the events back to back. Sample j of the read under level l and spread s:
//   G = the sum of the 12 bytes of x0, x1, x2 of stream 2, i = j, minus 1530        |G| <= 1530, standard deviation sqrt(65535) = 255.998
//   v = l + floor((s G + 128) / 256)                                                |s G| < 2^18 * 1530 < 2^29, |v| < 2^18 + 2^21 < 2^22
//   t = (v Q + 2^31) >> 32 (arithmetic)                                             Q < 2^40: |v Q| < 2^62
//   raw = clamp(t - off_r, -32768, 32767)
// Q = floor((digitisation 10 2^32 + R div 2) / R), R the range in 1e-4 pA, digitisation <= 2^16 (the numerator stays below 2^53);
// off_r = offset - off_spread + ((x0 (2 off_spread + 1)) >> 32), x0 of stream 0, i = 0.
#pragma once
#include <stdint.h>
#include "pg_fit.h"

#if defined(__HIPCC__)
#define PG_SIM_HD __host__ __device__ __forceinline__
#else
#define PG_SIM_HD static inline
#endif

#define PG_SIM_MAX_LEVEL (1u << 18)          // levels and stdvs lie below this
#define PG_SIM_MAX_DWELL (1u << 12)          // a slot's dwell
#define PG_SIM_MAX_DIGITISATION (1u << 16)
#define PG_SIM_MAX_Q (1ull << 40)
#define PG_SIM_MAX_OFFSET (1 << 20)          // |offset|
#define PG_SIM_MAX_OFF_SPREAD (1u << 16)
#define PG_SIM_MAX_LEAD (1u << 20)
#define PG_SIM_BATCH_SAMPLES (1ull << 28)    // samples of one generate
#define PG_SIM_PIECE 256u                    // ops per piece: the unit of work of one wave
#define PG_SIM_THREADS 256                   // four waves, a piece each
#ifndef PG_SIM_LANE
#define PG_SIM_LANE 8u                       // consecutive samples a lane owns: one 16-byte store (16: two; measured)
#endif
static_assert(PG_SIM_MAX_LEVEL == PG_FIT_MAX_LEVEL && PG_SIM_PIECE == PG_FIT_PIECE, "a simulated batch is one fit takes");
static_assert((uint64_t)(PG_SIM_MAX_LEVEL - 1) * 1530 < (1ull << 29), "s G fits an int32 with room");
static_assert((1ull << 18) + (1ull << 21) < (1ull << 22), "|v| < 2^22");
static_assert(22 + 40 <= 62, "|v Q| < 2^62, and the 2^31 added to it leaves an int64 whole");
static_assert((uint64_t)PG_SIM_MAX_DIGITISATION * 10 < (1ull << 20), "digitisation 10 2^32 + R div 2 < 2^53");
static_assert(2ull * PG_SIM_MAX_DWELL * PG_SIM_PIECE <= (1ull << 21), "a piece's samples fit 32 bits with room");
static_assert((2ull * PG_SIM_MAX_OFF_SPREAD + 1) < (1ull << 32) && 2ull * PG_SIM_MAX_DWELL + 1 < (1ull << 32), "the spans of the two uniform draws fit 32 bits");

enum { PG_SIM_OK = 0, PG_SIM_TOO_SHORT = 1, PG_SIM_BAD_BASE = 2, PG_SIM_NO_LEVEL = 3 }; // = PG_SIM_ST_* of include/pgmove.h
enum { PG_SIM_STREAM_READ = 0, PG_SIM_STREAM_DWELL = 1, PG_SIM_STREAM_SAMPLE = 2 };
enum { PG_SIM_FLAG_BAD_BASE = 1, PG_SIM_FLAG_NO_LEVEL = 2 };                             // what a piece reports of its ops

struct PgSimX { uint32_t x0, x1, x2, x3; };

PG_SIM_HD uint32_t pg_sim_mulhi(uint32_t a, uint32_t b) {
#if defined(__HIP_DEVICE_COMPILE__)
    return __umulhi(a, b);
#else
    return (uint32_t)(((uint64_t)a * b) >> 32);
#endif
}

PG_SIM_HD PgSimX pg_sim_philox(uint32_t c0, uint32_t c1, uint32_t c2, uint32_t c3, uint32_t k0, uint32_t k1) {
#if defined(__HIP_DEVICE_COMPILE__)
#pragma unroll
#endif
    for (int r = 0; r < 10; r++) {
        const uint32_t h0 = pg_sim_mulhi(0xD2511F53u, c0), l0 = 0xD2511F53u * c0, h1 = pg_sim_mulhi(0xCD9E8D57u, c2), l1 = 0xCD9E8D57u * c2;
        c0 = h1 ^ c1 ^ k0; c1 = l1; c2 = h0 ^ c3 ^ k1; c3 = l0;
        k0 += 0x9E3779B9u; k1 += 0xBB67AE85u;
    }
    return PgSimX{c0, c1, c2, c3};
}
PG_SIM_HD PgSimX pg_sim_draw(uint64_t seed, uint64_t read, uint32_t stream, uint32_t i) {
    return pg_sim_philox(i, stream, (uint32_t)read, (uint32_t)(read >> 32), (uint32_t)seed, (uint32_t)(seed >> 32));
}
// lo + floor(x span / 2^32): uniform over span values
PG_SIM_HD uint32_t pg_sim_below(uint32_t x, uint32_t span) { return pg_sim_mulhi(x, span); }

PG_SIM_HD int32_t pg_sim_bytes(uint32_t x) {
#if defined(__HIP_DEVICE_COMPILE__)
    return (int32_t)__builtin_amdgcn_sad_u8(x, 0u, 0u);
#else
    return (int32_t)((x & 0xffu) + ((x >> 8) & 0xffu) + ((x >> 16) & 0xffu) + (x >> 24));
#endif
}
PG_SIM_HD int32_t pg_sim_noise(const PgSimX &x) { return pg_sim_bytes(x.x0) + pg_sim_bytes(x.x1) + pg_sim_bytes(x.x2) - 1530; }

// one sample: level l and spread s in 1e-3 pA, the run's Q, the read's off_r
PG_SIM_HD int32_t pg_sim_raw(int32_t l, int32_t s, int32_t G, int64_t Q, int32_t off_r) {
    const int32_t v = l + ((s * G + 128) >> 8);
    const int64_t t = ((int64_t)v * Q + (1ll << 31)) >> 32;
    const int64_t x = t - off_r;
    return (int32_t)(x < -32768 ? -32768 : x > 32767 ? 32767 : x);
}
PG_SIM_HD int32_t pg_sim_sample(uint64_t seed, uint64_t read, uint32_t j, int32_t l, int32_t s, int64_t Q, int32_t off_r) {
    return pg_sim_raw(l, s, s ? pg_sim_noise(pg_sim_draw(seed, read, PG_SIM_STREAM_SAMPLE, j)) : 0, Q, off_r);
}

PG_SIM_HD uint32_t pg_sim_dwell(uint64_t seed, uint64_t read, uint32_t e, uint32_t D, uint32_t spread_pct) {
    const uint32_t w = D * spread_pct / 100u, lo = D > w + 1u ? D - w : 1u, hi = D + w;
    return lo + pg_sim_below(pg_sim_draw(seed, read, PG_SIM_STREAM_DWELL, e).x0, hi - lo + 1u);
}
PG_SIM_HD int32_t pg_sim_off_r(uint64_t seed, uint64_t read, int32_t offset, uint32_t off_spread) {
    return offset - (int32_t)off_spread + (int32_t)pg_sim_below(pg_sim_draw(seed, read, PG_SIM_STREAM_READ, 0).x0, 2u * off_spread + 1u);
}

// 0..3 for ACGTU, -1 for every other byte
PG_SIM_HD int pg_sim_base(uint32_t c) { return c == 'U' ? 3 : pg_fit_base(c); }
// the first base of event e's k-mer in a read of lb >= k bases
PG_SIM_HD uint32_t pg_sim_kmer_first(uint32_t lb, uint32_t k, uint32_t m, bool rna, uint32_t e) {
    uint32_t i = e > m ? e - m : 0u;
    if (i > lb - k) i = lb - k;
    return rna ? lb - i - k : i;
}
// its slot, or -1 when a letter is outside ACGTU
template <class Seq> PG_SIM_HD int32_t pg_sim_code(const Seq seq, uint32_t first, uint32_t k) {
    int32_t code = 0;
    for (uint32_t j = 0; j < k; j++) {
        const int b = pg_sim_base(seq[first + j]);
        if (b < 0) return -1;
        code = code * 4 + b;
    }
    return code;
}

// ---- host only ----------------------------------------------------------------------------------------------------------------------

// Q of a run, or 0 when it is refused (no range, a digitisation outside 1 .. 2^16, Q >= 2^40)
static inline uint64_t pg_sim_q(uint32_t digitisation, uint64_t range_e4) {
    if (digitisation < 1 || digitisation > PG_SIM_MAX_DIGITISATION || range_e4 < 1 || range_e4 > (1ull << 40)) return 0;
    const uint64_t q = (((uint64_t)digitisation * 10u << 32) + range_e4 / 2) / range_e4;
    return q < PG_SIM_MAX_Q ? q : 0;
}

struct PgSimRule {
    uint32_t k, m; bool rna; uint64_t seed; uint64_t Q; int32_t offset; uint32_t off_spread, spread_pct, lead, lead_level, lead_stdv;
};
// null, or what is wrong with the parameters (pg_sim_create's message)
static inline const char *pg_sim_rule_error(uint32_t k, uint32_t m, uint32_t digitisation, uint64_t range_e4, int32_t offset, uint32_t off_spread, uint32_t spread_pct, uint32_t lead,
                                            uint32_t lead_level, uint32_t lead_stdv) {
    if (k < 1 || k > PG_FIT_MAX_K) return "kmer_size of 1 to 9 is required";
    if (m > 64) return "sig_move_offset of at most 64 is required";
    if (digitisation < 1 || digitisation > PG_SIM_MAX_DIGITISATION) return "digitisation of 1 to 65536 is required";
    if (range_e4 < 1) return "a range above 0 is required";
    if (!pg_sim_q(digitisation, range_e4)) return "digitisation / range is too large: Q = digitisation 10 2^32 / range_e4 must stay below 2^40";
    if (offset < -PG_SIM_MAX_OFFSET || offset > PG_SIM_MAX_OFFSET) return "an offset within +-2^20 is required";
    if (off_spread > PG_SIM_MAX_OFF_SPREAD) return "off_spread of at most 65536 is required";
    if (spread_pct > 100) return "spread_pct of 0 to 100 is required";
    if (lead > PG_SIM_MAX_LEAD) return "lead of at most 2^20 samples is required";
    if (lead_level >= PG_SIM_MAX_LEVEL || lead_stdv >= PG_SIM_MAX_LEVEL) return "lead_level and lead_stdv below 262144 (262.144 pA) are required";
    return nullptr;
}
// null, or what is wrong with the tables of 4^k slots
static inline const char *pg_sim_tables_error(const uint32_t *levels, const uint32_t *stdvs, const uint32_t *dwells, uint32_t k, uint64_t &slot) {
    for (slot = 0; slot < (1ull << (2 * k)); slot++) {
        if (levels[slot] >= PG_SIM_MAX_LEVEL) return "a level lies below 262144";
        if (stdvs[slot] >= PG_SIM_MAX_LEVEL) return "a stdv lies below 262144";
        if (dwells[slot] < 1 || dwells[slot] > PG_SIM_MAX_DWELL) return "a dwell is 1 to 4096 samples";
    }
    return nullptr;
}

// One read by the rule, event after event and sample after sample. Returns the status; ops gets lb values and sig lead + sum(ops) samples
// for PG_SIM_OK and nothing otherwise. *off_r is set for every read.
static inline uint32_t pg_sim_walk_host(const PgSimRule &R, const uint32_t *levels, const uint32_t *stdvs, const uint32_t *dwells, const uint8_t *seq, uint32_t lb, uint64_t read,
                                        std::vector<uint32_t> &ops, std::vector<int16_t> &sig, int32_t *off_r) {
    ops.clear(); sig.clear();
    const int32_t off = pg_sim_off_r(R.seed, read, R.offset, R.off_spread);
    if (off_r) *off_r = off;
    if (lb < R.k) return PG_SIM_TOO_SHORT;
    for (uint32_t i = 0; i < lb; i++)
        if (pg_sim_base(seq[i]) < 0) return PG_SIM_BAD_BASE;
    std::vector<int32_t> slot(lb);
    for (uint32_t e = 0; e < lb; e++) {
        slot[e] = pg_sim_code(seq, pg_sim_kmer_first(lb, R.k, R.m, R.rna, e), R.k);
        if (!levels[slot[e]]) return PG_SIM_NO_LEVEL;
    }
    uint32_t j = 0;
    for (; j < R.lead; j++) sig.push_back((int16_t)pg_sim_sample(R.seed, read, j, (int32_t)R.lead_level, (int32_t)R.lead_stdv, (int64_t)R.Q, off));
    for (uint32_t e = 0; e < lb; e++) {
        const uint32_t n = pg_sim_dwell(R.seed, read, e, dwells[slot[e]], R.spread_pct);
        ops.push_back(n);
        for (uint32_t t = 0; t < n; t++, j++) sig.push_back((int16_t)pg_sim_sample(R.seed, read, j, (int32_t)levels[slot[e]], (int32_t)stdvs[slot[e]], (int64_t)R.Q, off));
    }
    return PG_SIM_OK;
}

// The file `poregen model --dwell_model` writes: rows KMER<TAB>median, the median rounded to whole samples with halves up (a median of an
// even count ends in .5). A row whose median is empty or "nan" (a k-mer without events) is skipped. dwells[4^k]: 0 for a k-mer the file
// does not give. false: the file is refused, err names the line and the reason.
static inline bool pg_sim_parse_dwell_text(const char *text, size_t n, uint32_t want_k, uint32_t &k_out, std::vector<uint32_t> &dwells, std::string &err) {
    std::vector<uint32_t> dw; uint32_t kk = 0;
    size_t line_no = 0;
    auto fail = [&](const std::string &why) { err = "line " + std::to_string(line_no) + ": " + why; return false; };
    for (size_t p = 0; p < n;) {
        const char *nl = (const char *)memchr(text + p, '\n', n - p);
        size_t end = nl ? (size_t)(nl - text) : n;
        const size_t next = nl ? end + 1 : n;
        line_no++;
        if (end > p && text[end - 1] == '\r') end--;
        const char *ln = text + p; const size_t len = end - p;
        p = next;
        if (len == 0 || ln[0] == '#') continue;
        const char *t = (const char *)memchr(ln, '\t', len);
        if (!t) return fail("a row needs KMER<TAB>median");
        const size_t kl = (size_t)(t - ln);
        const char *f = t + 1; size_t fl = len - kl - 1;
        if (const char *t2 = (const char *)memchr(f, '\t', fl)) fl = (size_t)(t2 - f);
        if (kl < 1 || kl > PG_FIT_MAX_K) return fail("a k-mer has 1 to 9 letters");
        if (kk == 0) {
            if (want_k && kl != want_k) return fail("the file's k-mers have " + std::to_string(kl) + " letters, the model's " + std::to_string(want_k));
            kk = (uint32_t)kl; dw.assign((size_t)1 << (2 * kk), 0u);
        } else if (kl != kk) return fail("k-mers of two lengths");
        const int32_t slot = pg_sim_code(ln, 0, kk);
        if (slot < 0) return fail("a k-mer with a letter outside ACGTU");
        if (fl == 0 || (fl == 3 && memcmp(f, "nan", 3) == 0)) continue;
        pgbc::Dec d; uint32_t v = 0;
        if (!pgbc::parse(f, fl, d)) return fail("the median is no number");
        if (d.neg || pg_fit_round_dec(d, 1, v) || v < 1 || v > PG_SIM_MAX_DWELL) return fail("a dwell outside 1 to 4096 samples");
        if (dw[slot]) return fail("a k-mer twice");
        dw[slot] = v;
    }
    if (kk == 0) { err = "the file holds no k-mer"; return false; }
    k_out = kk; dwells = std::move(dw);
    return true;
}

// The command's read drawing (stream 0, i = 1): x0 and x1 give the position over the `total` concatenated bases, x2 the length in
// [read_len / 2, 3 read_len / 2], x3 & 1 the strand (forward alone with rna). The caller cuts the read at its contig's end.
struct PgSimPick { uint64_t pos; uint32_t len; bool reverse; };
static inline PgSimPick pg_sim_pick(uint64_t seed, uint64_t read, uint64_t total, uint32_t read_len, bool rna) {
    const PgSimX x = pg_sim_draw(seed, read, PG_SIM_STREAM_READ, 1);
    const uint64_t u = ((uint64_t)x.x0 << 32) | x.x1;
    PgSimPick o;
    o.pos = (uint64_t)(((unsigned __int128)u * total) >> 64);
    const uint32_t lo = read_len / 2, hi = read_len + read_len / 2;
    o.len = lo + pg_sim_below(x.x2, hi - lo + 1u);
    o.reverse = !rna && (x.x3 & 1u);
    return o;
}
// a true boundary B (a sample of the read) rounded to the stride from ts = lead: the element of the move table it falls on, times the stride
static inline uint64_t pg_sim_round_stride(uint64_t B, uint32_t lead, uint32_t stride) { return (uint64_t)stride * ((B - lead + stride / 2) / stride); }
