// pg_evalign.h -- the rule of `poregen eventalign`: one row per event that `poregen fit` counts -- where it lies, its level and spread in
// the model's units, the model's level for its k-mer, and how many standard deviations apart they are. Plain C++ that the kernels
// (pg_evalign.hip), the library's host side and a host test (pg_hosttest.cpp: pgt_evalign_*) all compile. Not installed.
//
// Which events. Exactly the events fit counts (pg_fit.h: pg_fit_kmer_at / pg_fit_gap_kmer_at, the duration limits, ACGT letters, a level)
// of the reads whose fit has the status ok. Narrower than fit in two places, both refused before a batch is taken: 1 <= min_dur and
// max_dur <= PG_EV_MAX_LEN = 4096, so that pg_evstat.h's bounds hold as written; and a k-mer with a level has level_stdv > 0.
//
// Per event: n raw samples r_1 .. r_n, its k-mer's level L and spread SD in 1e-3 pA (0 < L < 2^18, 0 < SD < 2^18), its read's fit
// sample = a + b * level.
//   u_i = 1000 r_i: the samples in 1e-3 raw counts. d_i = u_i - u_1, S1 = sum d_i, S2 = sum d_i^2.
//   m_raw = pg_ev_mean(u_1, n, S1)           the mean, halves up
//   s_raw = pg_ev_spread(n, S1, S2)          the sample standard deviation, halves up, for n >= 2; 0 for n = 1
//   per read, on the host, one IEEE operation each: A = 1000.0 * a, G = (1.0 / b) / 1000.0
//   mean_u = llrint(cut(((double)m_raw - A) * G)), stdv_u = llrint(cut((double)s_raw * G))     in 1e-3 pA; cut clamps to +-2^21 as
//       pg_fit_resid does, so that no conversion leaves an int64 -- and with it an int32 -- whatever a and b are
//   z_c = floor((200 (mean_u - L) + SD) / (2 SD))      (mean_u - L) / SD in hundredths, halves up, floor towards -infinity
// On the device the two conversions are an exact int -> double conversion, one subtraction, one multiplication (-ffp-contract=off: no
// fused multiply-add) and __double2ll_rn: no division and no square root beyond pg_ev_isqrt's.
// Bounds (the static_asserts below). |r| <= 2^15, so |u_i| <= 32768000 < 2^25 and |d_i| <= 65535000 < 2^26, far inside PG_EV_MAX_DEV =
// 2^41. With n <= 2^12: |S1| < 2^38, d_i^2 < 2^52, S2 < 2^64 -- a uint64 on the device (an LDS atomic per sample), the high word of
// PgEvSums stays 0. |m_raw| < 2^25 and s_raw < 2^26 are exact doubles. |mean_u| <= 2^21, L < 2^18: |200 (mean_u - L) + SD| < 200 (2^21 + 2^18) +
// 2^18 < 2^29, 2 SD < 2^19: z_c fits an int32, every step an int64.
//
// Text. One tab-separated line per row, nanopolish / f5c `eventalign --scale-events --signal-index` columns (PG_EA_HEADER). The numbers
// are printed from the integers: three decimals for 1e-3 pA, two for z_c (-1 is "-0.01"), event_length n in samples -- or, with a
// sample_rate R (1 .. 10^6), seconds with five decimals from floor((2 * 10^5 n + R) / (2 R)) < 2^31. One emitter writes a row into a
// sink; pg_ea_row_len counts with it and pg_ea_row_write stores with it, on the host and on the device alike.
#pragma once
#include "pg_fit.h"
#include <cmath>

#if defined(__HIPCC__)
#define PG_EA_HD __host__ __device__ __forceinline__
#define PG_EA_M __host__ __device__ __forceinline__
#else
#define PG_EA_HD static inline
#define PG_EA_M inline
#endif

#define PG_EA_MAX_DUR PG_EV_MAX_LEN          // the largest max_dur a handle takes
#define PG_EA_MAX_RATE 1000000u              // the largest sample_rate
#define PG_EA_CUT 2097152.0                  // 2^21: both conversions are cut to +-this before they are rounded
#define PG_EA_HEADER "contig\tposition\treference_kmer\tread_index\tstrand\tevent_index\tevent_level_mean\tevent_stdv\tevent_length\tmodel_kmer\tmodel_mean\tmodel_stdv\tstandardized_level\tstart_idx\tend_idx\n"
// |u_i - u_1| <= 1000 * 65535 < 2^26, far inside PG_EV_MAX_DEV: pg_evstat.h's rule takes every event of at most PG_EV_MAX_LEN samples
static_assert(1000ll * 65535 < (1ll << 26) && (1ll << 26) < PG_EV_MAX_DEV && PG_EA_MAX_DUR == (1u << 12), "an event's deviations lie inside pg_evstat.h's window");
static_assert(12 + 26 < 63 && 12 + 2 * 26 <= 64, "S1 fits an int64 and S2 a uint64: 2^12 samples of |d| < 2^26");
static_assert(200ll * ((1ll << 21) + (1ll << 18)) + (1ll << 18) < (1ll << 31) && PG_FIT_MAX_LEVEL == (1u << 18), "200 (mean_u - L) + SD fits an int32: |mean_u| <= 2^21, L, SD < 2^18");
static_assert(200000ull * PG_EA_MAX_DUR + PG_EA_MAX_RATE < (1ull << 31), "the event_length numerator fits 32 bits");

// one row: 40 bytes (pg_evalign_row of include/pgmove.h is this struct)
struct PgEaRow { uint32_t read, event; uint64_t start; uint32_t n, slot, first; int32_t mean_u, stdv_u, z_c; };
static_assert(sizeof(PgEaRow) == 40, "a row is 40 bytes");

PG_EA_HD bool pg_ea_params_ok(uint32_t min_dur, uint32_t max_dur, uint32_t sample_rate) { return min_dur >= 1 && min_dur <= max_dur && max_dur <= PG_EA_MAX_DUR && sample_rate <= PG_EA_MAX_RATE; }

// A and G of a read from its fit; false when they are no numbers to convert with (a fit's are)
static inline bool pg_ea_read_scale(double a, double b, double &A, double &G) {
    A = 1000.0 * a;
    const double inv_b = 1.0 / b;
    G = inv_b / 1000.0;
    return std::isfinite(A) && std::isfinite(G) && b > 0 && G >= 0;
}

PG_EA_HD int64_t pg_ea_round_cut(double x) {
    x = x > PG_EA_CUT ? PG_EA_CUT : x < -PG_EA_CUT ? -PG_EA_CUT : x;
#if defined(__HIP_DEVICE_COMPILE__)
    return __double2ll_rn(x);
#else
    return llrint(x);
#endif
}
PG_EA_HD int32_t pg_ea_z(int64_t mean_u, uint32_t L, uint32_t SD) { // SD >= 1
    const int64_t num = 200 * (mean_u - (int64_t)L) + (int64_t)SD, den = 2 * (int64_t)SD;
    int64_t q = num / den;
    if (num - q * den < 0) q--; // floor
    return (int32_t)q;
}
// One event from its sums about its first sample (first_raw = r_1; s1, s2 in 1e-3 raw counts and their squares)
PG_EA_HD void pg_ea_event(int32_t first_raw, uint32_t n, int64_t s1, uint64_t s2, double A, double G, uint32_t L, uint32_t SD, int32_t &mean_u, int32_t &stdv_u, int32_t &z_c) {
    const int64_t m_raw = pg_ev_mean(1000ll * first_raw, n, s1);
    const int64_t s_raw = n >= 2 ? pg_ev_spread(n, PgEvSums{s1, s2, 0}) : 0;
    mean_u = (int32_t)pg_ea_round_cut(((double)m_raw - A) * G);
    stdv_u = (int32_t)pg_ea_round_cut((double)s_raw * G);
    z_c = pg_ea_z(mean_u, L, SD);
}

// ---- the text of a row --------------------------------------------------------------------------------------------------------------------
struct PgEaCount { uint32_t n = 0; PG_EA_M void put(char) { n++; } };
struct PgEaStore { char *p; PG_EA_M void put(char c) { *p++ = c; } };

template <class S> PG_EA_HD void pg_ea_put_u64(S &s, uint64_t v) {
    uint64_t p = 1;
    while (v / p >= 10) p *= 10;
    for (; p; p /= 10) s.put((char)('0' + (v / p) % 10));
}
// v / 10^digits with `digits` decimals, from the integer: the sign, the integer part, '.', the fraction zero-padded
template <class S> PG_EA_HD void pg_ea_put_dec(S &s, int64_t v, uint32_t digits) {
    const uint64_t mag = v < 0 ? 0 - (uint64_t)v : (uint64_t)v;
    uint64_t pw = 1;
    for (uint32_t i = 0; i < digits; i++) pw *= 10;
    if (v < 0) s.put('-');
    pg_ea_put_u64(s, mag / pw);
    s.put('.');
    uint64_t f = mag % pw;
    for (pw /= 10; pw; pw /= 10) s.put((char)('0' + (f / pw) % 10));
}
PG_EA_HD char pg_ea_complement(uint8_t c) { return c == 'A' ? 'T' : c == 'C' ? 'G' : c == 'G' ? 'C' : c == 'T' ? 'A' : 'N'; }

// everything a row's line is made of. kmer: the k letters of seq at the row's `first`; S: the bases of the read's seq (its slice)
struct PgEaText {
    const uint8_t *contig, *label, *kmer;
    uint32_t contig_len, label_len, k, S, first, reverse, event, n, sample_rate, L, SD;
    int32_t mean_u, stdv_u, z_c;
    int64_t ref_start;
    uint64_t start;
};
PG_EA_HD int64_t pg_ea_position(int64_t ref_start, uint32_t S, uint32_t first, uint32_t k, bool reverse) {
    return ref_start + (int64_t)(reverse ? S - first - k : first);
}
PG_EA_HD uint32_t pg_ea_seconds_e5(uint32_t n, uint32_t rate) { return (uint32_t)((200000ull * n + rate) / (2ull * rate)); }

template <class S> PG_EA_HD void pg_ea_row_emit(S &s, const PgEaText &t) {
    for (uint32_t i = 0; i < t.contig_len; i++) s.put((char)t.contig[i]);
    s.put('\t');
    const int64_t pos = pg_ea_position(t.ref_start, t.S, t.first, t.k, t.reverse != 0);
    if (pos < 0) s.put('-');
    pg_ea_put_u64(s, pos < 0 ? 0 - (uint64_t)pos : (uint64_t)pos);
    s.put('\t');
    for (uint32_t i = 0; i < t.k; i++) s.put(t.reverse ? pg_ea_complement(t.kmer[t.k - 1 - i]) : (char)t.kmer[i]);
    s.put('\t');
    for (uint32_t i = 0; i < t.label_len; i++) s.put((char)t.label[i]);
    s.put('\t'); s.put('t'); s.put('\t');
    pg_ea_put_u64(s, t.event); s.put('\t');
    pg_ea_put_dec(s, t.mean_u, 3); s.put('\t');
    pg_ea_put_dec(s, t.stdv_u, 3); s.put('\t');
    if (t.sample_rate) pg_ea_put_dec(s, pg_ea_seconds_e5(t.n, t.sample_rate), 5); else pg_ea_put_u64(s, t.n);
    s.put('\t');
    for (uint32_t i = 0; i < t.k; i++) s.put((char)t.kmer[i]);
    s.put('\t');
    pg_ea_put_dec(s, t.L, 3); s.put('\t');
    pg_ea_put_dec(s, t.SD, 3); s.put('\t');
    pg_ea_put_dec(s, t.z_c, 2); s.put('\t');
    pg_ea_put_u64(s, t.start); s.put('\t');
    pg_ea_put_u64(s, t.start + t.n); s.put('\n');
}
PG_EA_HD uint32_t pg_ea_row_len(const PgEaText &t) { PgEaCount c; pg_ea_row_emit(c, t); return c.n; }
PG_EA_HD uint32_t pg_ea_row_write(char *dst, const PgEaText &t) { PgEaStore w{dst}; pg_ea_row_emit(w, t); return (uint32_t)(w.p - dst); }

// ---- host only: the walk of one fitted read -----------------------------------------------------------------------------------------------
// The rows of one read by the rule, `read` left 0. op_t null: a read of an all-matches batch (S = lb bases). Returns PG_FIT_OK,
// PG_FIT_OUT_OF_SIGNAL or PG_FIT_REF_LENGTH (no rows then), -1 for an op code above 2, -2 for a slice above PG_FIT_MAX_SLICE, -3 for a
// k-mer with a level and no spread.
static inline int pg_ea_walk_host(const uint8_t *seq, uint64_t S, const uint32_t *op_n, const uint8_t *op_t, uint32_t lb, int64_t q, const int16_t *sig, uint64_t n_sig,
                                  const uint32_t *levels, const uint32_t *stdvs, uint32_t k, uint32_t m, bool rna, uint32_t min_dur, uint32_t max_dur, double a, double b,
                                  std::vector<PgEaRow> &rows) {
    rows.clear();
    uint64_t total = 0, cols = 0;
    if (op_t) { if (!pg_fit_gap_totals(op_n, op_t, lb, total, cols)) return -1; }
    else { for (uint32_t e = 0; e < lb; e++) total += op_n[e]; cols = S; }
    if (S > PG_FIT_MAX_SLICE) return -2;
    const uint32_t st = pg_fit_gap_status(q, total, n_sig, cols, S);
    if (st != PG_FIT_OK) return (int)st;
    double A, G;
    pg_ea_read_scale(a, b, A, G);
    uint64_t pos = (uint64_t)q; uint32_t col = 0;
    for (uint32_t e = 0; e < lb; e++) {
        const uint32_t t = op_t ? op_t[e] : (uint32_t)PG_FIT_OP_MATCH, n = op_n[e];
        const uint64_t at = pos; const uint32_t c = col;
        pos += pg_fit_op_samples(t, n); col += op_t ? pg_fit_op_cols(t, n) : 0u;
        uint32_t first;
        if (t != PG_FIT_OP_MATCH || !pg_fit_dur_ok(n, min_dur, max_dur)) continue;
        if (op_t ? !pg_fit_gap_kmer_at(op_t, lb, (uint32_t)S, k, m, rna, e, c, first) : !pg_fit_kmer_at(lb, k, m, rna, e, first)) continue;
        const int32_t slot = pg_fit_code(seq, first, k);
        if (slot < 0 || !levels[slot]) continue;
        if (!stdvs[slot]) return -3;
        int64_t s1 = 0; uint64_t s2 = 0;
        for (uint32_t i = 0; i < n; i++) { const int64_t d = 1000ll * ((int64_t)sig[at + i] - (int64_t)sig[at]); s1 += d; s2 += (uint64_t)(d * d); }
        PgEaRow r{0, e, at, n, (uint32_t)slot, first, 0, 0, 0};
        pg_ea_event(sig[at], n, s1, s2, A, G, levels[slot], stdvs[slot], r.mean_u, r.stdv_u, r.z_c);
        rows.push_back(r);
    }
    return PG_FIT_OK;
}
