// pg_fit.h -- the rule of `poregen fit`: how well a k-mer model explains the samples of the basecaller's own segmentation. Plain C++ that
// the kernels (pg_fit.hip), the library's host side and a host test (pg_hosttest.cpp: pgt_fit_*) all compile. Not installed.
//
// Model. L[slot] is a k-mer's level in units of 1e-3 pA, 0 < L < 2^18 (PG_FIT_MAX_LEVEL); 0 stands for "no level". A k-mer's slot is its
// rank in ACGT order (first base most significant).
//
// Events. An accepted read has Lb bases seq, ops n_0 .. n_{Lb-1} (all matches) and query_start q; event e is the samples
// [q + n_0 + .. + n_{e-1}, .. + n_e). For i = 0 .. Lb - k the event e = i + m (if e < Lb) carries the k-mer seq[i, i + k), or
// seq[Lb - i - k, Lb - i) with rna. It counts when min_dur <= n_e <= max_dur, every letter is one of ACGT and the k-mer has a level.
//
// Pass 1, per read, over the samples r (raw int16) of the counted events, l the event's level:
//   N = sum 1, SL = sum l, SLL = sum l^2, SR = sum r, SRL = sum r l, SRR = sum r^2, E = counted events.
// Bounds (the static_asserts below). With N <= PG_FIT_MAX_N = 2^24, 0 < l < 2^18 and |r| <= 2^15:
//   SL < 2^42, SLL < 2^60, |SR| <= 2^39, |SRL| < 2^57, SRR <= 2^54        every sum an int64
//   N SLL, SL^2 < 2^84;  N SRL, SL SR < 2^81;  SR SLL, SL SRL < 2^99;  N SRR, SR^2 <= 2^78      every product an __int128
// A read with more counted samples is reported as too_long; only its N and E are kept.
//
// Solve, on the host: den = N SLL - SL^2, numb = N SRL - SL SR, numa = SR SLL - SL SRL exactly; b = (double)numb / (double)den,
// a = (double)numa / (double)den, inv_b = 1.0 / b, each conversion and division one correctly rounded IEEE operation. On the device
// (pg_fit_calibrate: k_fit_solve) the same numbers bit for bit from pg_fit_solve_hd, whose conversion is written out by hand.
//
// Pass 2, per k-mer, over the fitted reads: c = llrint(((double)r - a) * inv_b) (ties to even), d = c - l clamped to |d| <= 2^18 - 1
// (PG_FIT_CLAMP; clamped samples are counted). |(r - a) * inv_b| >= 2^21 clamps whatever l is, so the product is cut to +-2^21 before it is
// rounded: no conversion leaves the range of an int64. Per slot n_samples, n_events, sum d, sum d^2.
//   per event (n <= PG_FIT_MAX_DUR = 2^20 samples):  |sum d| < 2^38, sum d^2 < 2^56
//   per batch (at most PG_FIT_BATCH_SAMPLES = 2^28 samples of signal): sum d^2 <= 2^28 (2^18 - 1)^2 < 2^64: a uint64 per slot on the device
//   per run: the host adds the batches' sums in 128 bits: exact up to 2^92 samples per k-mer, far beyond the 2^40 asked for.
//
// Text. mean_resid = floor((2 sum d + n) / (2 n)), rms_resid = (isqrt(floor(4 sum d^2 / n)) + 1) div 2 (pg_evstat.h has the root),
// both in 1e-3 pA, printed with three decimals from the integers.
#pragma once
#include <stdint.h>
#include <math.h>
#include <stdio.h>
#include <string.h>
#include <string>
#include <vector>
#include "pg_evstat.h"
#include "pg_bcdec.h"

#if defined(__HIPCC__)
#define PG_FIT_HD __host__ __device__ __forceinline__
#else
#define PG_FIT_HD static inline
#endif

#define PG_FIT_MAX_K 9u
#define PG_FIT_MAX_LEVEL (1u << 18)          // levels lie below this (262.144 pA)
#define PG_FIT_CLAMP ((1 << 18) - 1)         // |d| is clamped to this
#define PG_FIT_MAX_N (1ll << 24)             // counted samples of a read that is fitted
#define PG_FIT_MAX_DUR (1u << 20)            // the largest max_dur a handle takes
#define PG_FIT_BATCH_SAMPLES (1ull << 28)    // samples of signal in one submitted batch
#define PG_FIT_STEP 64u                      // ops a wave takes at a time, one per lane
#define PG_FIT_PIECE 256u                    // ops per piece: the unit of work of one wave
#define PG_FIT_THREADS 256                   // threads of a workgroup of either pass: four waves, a piece each
#define PG_FIT_LDS_K 5u                      // pass 2 keeps the per-slot sums of a workgroup in LDS up to this k (4^5 slots * 32 bytes)
#define PG_FIT_GRID 1024u                    // workgroups of pass 2 at most: its waves loop over the pieces
static_assert(PG_FIT_MAX_LEVEL == (1u << 18) && PG_FIT_MAX_N == (1ll << 24), "the overflow argument above is written for levels below 2^18 and 2^24 samples");
static_assert(24 + 18 < 63 && 24 + 2 * 18 < 63 && 24 + 15 + 18 < 63 && 24 + 2 * 15 < 63, "SL, SLL, SRL and SRR fit an int64");
static_assert(2 * 24 + 2 * 18 < 127 && 24 + 15 + 24 + 2 * 18 < 127 && 2 * 24 + 2 * 15 < 127, "den, numb, numa and Syy fit an __int128");
static_assert(20 + 18 < 63 && 20 + 2 * 18 < 63, "an event's sum d and sum d^2 fit 64 bits");
static_assert(28 + 2 * 18 <= 64, "a batch's sum d^2 per slot fits a uint64: 2^28 (2^18 - 1)^2 < 2^64");
static_assert(PG_FIT_PIECE % PG_FIT_STEP == 0 && PG_FIT_STEP == 64, "a step is one op per lane of a wave");

enum { PG_FIT_OK = 0, PG_FIT_OUT_OF_SIGNAL = 1, PG_FIT_TOO_LONG = 2, PG_FIT_FEW_EVENTS = 3, PG_FIT_FLAT = 4, PG_FIT_NEGATIVE_SCALE = 5, PG_FIT_REF_LENGTH = 6,
       PG_FIT_SKIPPED = 16 }; // PG_FIT_SKIPPED + c: the caller's skip code c (the expander's status of a read reform refuses)
enum { PG_FIT_OP_MATCH = 0, PG_FIT_OP_I = 1, PG_FIT_OP_D = 2 }; // op_t of a gapped batch
#define PG_FIT_MAX_SLICE 0xffffffffull       // bases of a gapped read's reference slice at most: a column of a read that takes part fits 32 bits

struct PgFitSums { int64_t n, sl, sll, sr, srl, srr, e; }; // 56 bytes per read

// 0..3 for ACGT, -1 for every other byte
PG_FIT_HD int pg_fit_base(uint32_t c) { return c == 'A' ? 0 : c == 'C' ? 1 : c == 'G' ? 2 : c == 'T' ? 3 : -1; }

// The k-mer of event e of a read of lb bases: false when the event carries none (e < m, or the k-mer would leave the read), else its first
// base in seq.
PG_FIT_HD bool pg_fit_kmer_at(uint32_t lb, uint32_t k, uint32_t m, bool rna, uint32_t e, uint32_t &first) {
    if (e < m || e >= lb) return false;
    const uint32_t i = e - m;
    if (lb < k || i > lb - k) return false;
    first = rna ? lb - i - k : i;
    return true;
}
// its slot, or -1 when a letter is none of ACGT
template <class Seq> PG_FIT_HD int32_t pg_fit_code(const Seq seq, uint32_t first, uint32_t k) {
    int32_t code = 0;
    for (uint32_t j = 0; j < k; j++) {
        const int b = pg_fit_base(seq[first + j]);
        if (b < 0) return -1;
        code = code * 4 + b;
    }
    return code;
}
PG_FIT_HD bool pg_fit_dur_ok(uint32_t n, uint32_t min_dur, uint32_t max_dur) { return n >= min_dur && n <= max_dur; }

// ---- the gapped rule (PG_BATCH_GAPPED): ops on the signal-to-reference alignment ---------------------------------------------------------
// op_t is 0 (match), 1 (I) or 2 (D), and seq is the read's reference slice of S bases. A match of n and an I of n take n samples, a D takes
// none; a match takes one reference column, a D of n takes n, an I none. c_j is the column in front of op j, C the read's total; a read with
// S != C is ref_length (behind out_of_signal) and no kernel reads its seq. Event j counts iff it is a match, ops j - m .. j - m + k - 1 all
// exist and are all matches (a clean window: its columns are consecutive), min_dur <= n_j <= max_dur, and its k-mer -- seq[c_j - m,
// c_j - m + k), with rna seq[S - (c_j - m) - k, S - (c_j - m)) -- lies inside the slice, has ACGT letters and a level. On a batch of only
// matches with S = Lb this is the rule above. Bounds: a read has fewer than 2^31 ops of fewer than 2^32 columns, so C < 2^63 (a uint64 per
// piece and per read); a read takes part only with C == S <= PG_FIT_MAX_SLICE, so inside a kernel every column fits 32 bits.
PG_FIT_HD uint32_t pg_fit_op_samples(uint32_t t, uint32_t n) { return t == PG_FIT_OP_D ? 0u : n; }
PG_FIT_HD uint32_t pg_fit_op_cols(uint32_t t, uint32_t n) { return t == PG_FIT_OP_MATCH ? 1u : t == PG_FIT_OP_D ? n : 0u; }
// The k-mer of event e (a match) of a gapped read of lb ops whose column is col: false when it carries none, else its first base in seq.
// Reads at most k bytes of op_t, all inside the read, and names no base outside [0, S).
template <class Ops> PG_FIT_HD bool pg_fit_gap_kmer_at(const Ops op_t, uint32_t lb, uint32_t S, uint32_t k, uint32_t m, bool rna, uint32_t e, uint32_t col, uint32_t &first) {
    if (e < m || e >= lb || lb < k || e - m > lb - k) return false;
    for (uint32_t j = 0; j < k; j++)
        if (op_t[e - m + j] != PG_FIT_OP_MATCH) return false;
    if (col < m || S < k || col - m > S - k) return false;
    first = rna ? S - (col - m) - k : col - m;
    return true;
}

PG_FIT_HD void pg_fit_add(PgFitSums &s, int32_t r, int32_t l) {
    s.n += 1; s.sl += l; s.sll += (int64_t)l * l; s.sr += r; s.srl += (int64_t)r * l; s.srr += (int64_t)r * r;
}

// one sample's residual in 1e-3 pA
PG_FIT_HD int32_t pg_fit_resid(int32_t r, double a, double inv_b, int32_t l, bool &clamped) {
    double x = ((double)r - a) * inv_b;
    const double cut = 2097152.0; // 2^21: beyond it d clamps for every level
    x = x > cut ? cut : x < -cut ? -cut : x;
#if defined(__HIP_DEVICE_COMPILE__)
    const int64_t c = __double2ll_rn(x);
#else
    const int64_t c = llrint(x);
#endif
    int64_t d = c - l;
    clamped = d > PG_FIT_CLAMP || d < -PG_FIT_CLAMP;
    if (d > PG_FIT_CLAMP) d = PG_FIT_CLAMP;
    if (d < -PG_FIT_CLAMP) d = -PG_FIT_CLAMP;
    return (int32_t)d;
}

struct PgFitSolve { uint32_t status; double a, b, inv_b; };

// ---- the solve for host and device (k_fit_solve, pg_fit_calibrate; the host seam pgt_fit_solve_hd) -------------------------------------
// The same numbers as pg_fit_solve below, bit for bit, without what a device lacks: the conversion of an __int128 to a double is a
// library call there, so it is written out. The products and sums are the compiler's 128-bit + - x on both sides.

// A signed 128-bit integer to the nearest double, ties to even: the leading bit, 53 bits kept, the guard bit and the sticky bits decide,
// and a carry out of the 53 bits goes into the exponent (the mantissa is then a power of two). Exact for |v| < 2^53.
PG_FIT_HD double pg_fit_i128_to_double(__int128 v) {
    const bool neg = v < 0;
    const unsigned __int128 u = neg ? (unsigned __int128)0 - (unsigned __int128)v : (unsigned __int128)v;
    const uint64_t hi = (uint64_t)(u >> 64), lo = (uint64_t)u;
    if (!(hi | lo)) return 0.0;
    const int top = hi ? 127 - __builtin_clzll(hi) : 63 - __builtin_clzll(lo); // index of the leading bit
    uint64_t mant; // the 53 leading bits
    int exp2 = top - 52; // the value is mant * 2^exp2
    if (top <= 52) { mant = lo; exp2 = 0; }
    else {
        const int sh = top - 52; // bits dropped, 1 .. 75
        mant = (uint64_t)(u >> sh);
        const bool guard = (uint64_t)(u >> (sh - 1)) & 1u;
        const bool sticky = sh > 1 && (u & ((((unsigned __int128)1) << (sh - 1)) - 1)) != 0;
        if (guard && (sticky || (mant & 1u))) mant++;
        if (mant >> 53) { mant >>= 1; exp2++; } // all ones rounded up: 2^53 -> 2^52 one exponent higher
    }
    // mant < 2^53 converts exactly; 2^exp2 is built from its bits (exp2 <= 75: a normal number), and the product is exact
    union { uint64_t b; double d; } p2;
    p2.b = (uint64_t)(1023 + exp2) << 52;
    const double r = (double)(int64_t)mant * p2.d;
    return neg ? -r : r;
}

// pg_fit_solve for host and device
PG_FIT_HD PgFitSolve pg_fit_solve_hd(const PgFitSums &s, uint32_t min_events) {
    PgFitSolve o{PG_FIT_OK, 0.0, 0.0, 0.0};
    if (s.n > PG_FIT_MAX_N) { o.status = PG_FIT_TOO_LONG; return o; }
    if (s.e < (int64_t)min_events) { o.status = PG_FIT_FEW_EVENTS; return o; }
    const __int128 den = (__int128)s.n * s.sll - (__int128)s.sl * s.sl;
    if (den == 0) { o.status = PG_FIT_FLAT; return o; }
    const __int128 numb = (__int128)s.n * s.srl - (__int128)s.sl * s.sr;
    if (numb <= 0) { o.status = PG_FIT_NEGATIVE_SCALE; return o; }
    const __int128 numa = (__int128)s.sr * s.sll - (__int128)s.sl * s.srl;
    const double dd = pg_fit_i128_to_double(den);
    o.b = pg_fit_i128_to_double(numb) / dd;
    o.a = pg_fit_i128_to_double(numa) / dd;
    o.inv_b = 1.0 / o.b;
    return o;
}

// ---- a read's place on the model's pA scale (gmove --reform --scale_model; pg_params.scaling == PG_SCALING_PER_READ) --------------------
// The fit says sample = a + b * level with the level in 1e-3 pA, so a sample's pA is g (a + offset) + (1000 g b) * (level in pA), and
//   g      = range / digitisation          (the expression PgStatRec::scale uses)
//   center = (a + offset) * g
//   spread = (b * 1000.0) * g
//   use    = status == PG_FIT_OK  &&  center is finite  &&  spread is finite and > 0
// each line one rounded IEEE double operation. The collector stores (pA - center) / spread per sample: the sample on the model's pA scale.
// A sample whose pA lies outside [pa_min, pa_max] is zeroed FIRST, as for med-MAD (gmove.cpp:756-759, 774): it is stored as
// (0 - center) / spread. A read with use == 0 has center = spread = 0.
struct PgFitScale { double center, spread; uint8_t use; };
PG_FIT_HD bool pg_fit_finite(double x) { return x - x == 0.0; } // (false for NaN and the infinities; no library call)
PG_FIT_HD PgFitScale pg_fit_scale_rule(uint32_t status, double a, double b, double digitisation, double offset, double range) {
    PgFitScale o{0.0, 0.0, 0};
    if (status != PG_FIT_OK) return o;
    const double g = range / digitisation;
    const double center = (a + offset) * g, spread = (b * 1000.0) * g;
    if (!pg_fit_finite(center) || !pg_fit_finite(spread) || !(spread > 0.0)) return o;
    o.center = center; o.spread = spread; o.use = 1;
    return o;
}

// ---- host only: the solve, the text rules, the model parser, the walk of one read -----------------------------------------------------

// the statuses behind out_of_signal, tested in the order of the enum; a and b only with PG_FIT_OK
static inline PgFitSolve pg_fit_solve(const PgFitSums &s, uint32_t min_events) {
    PgFitSolve o{PG_FIT_OK, 0.0, 0.0, 0.0};
    if (s.n > PG_FIT_MAX_N) { o.status = PG_FIT_TOO_LONG; return o; }
    if (s.e < (int64_t)min_events) { o.status = PG_FIT_FEW_EVENTS; return o; }
    const __int128 den = (__int128)s.n * s.sll - (__int128)s.sl * s.sl;
    if (den == 0) { o.status = PG_FIT_FLAT; return o; }
    const __int128 numb = (__int128)s.n * s.srl - (__int128)s.sl * s.sr;
    if (numb <= 0) { o.status = PG_FIT_NEGATIVE_SCALE; return o; }
    const __int128 numa = (__int128)s.sr * s.sll - (__int128)s.sl * s.srl;
    o.b = (double)numb / (double)den;
    o.a = (double)numa / (double)den;
    o.inv_b = 1.0 / o.b;
    return o;
}

// what the per-read table prints, in pA: shift, scale, rms (status PG_FIT_OK only)
static inline void pg_fit_report(const PgFitSums &s, double digitisation, double offset, double range, long double out[3]) {
    const __int128 den = (__int128)s.n * s.sll - (__int128)s.sl * s.sl;
    const __int128 numb = (__int128)s.n * s.srl - (__int128)s.sl * s.sr;
    const __int128 numa = (__int128)s.sr * s.sll - (__int128)s.sl * s.srl;
    const __int128 syy = (__int128)s.n * s.srr - (__int128)s.sr * s.sr;
    const long double g = (long double)range / (long double)digitisation, ld = (long double)den, lb = (long double)numb;
    out[0] = g * ((long double)numa / ld + (long double)offset);
    out[1] = 1000.0L * g * (lb / ld);
    long double rss = ((long double)syy - lb * lb / ld) / (long double)s.n;
    if (rss < 0) rss = 0;
    out[2] = g * sqrtl(rss / (long double)s.n);
}

// per-slot residuals from the sums, n > 0: the mean and the root mean square, each rounded to the nearest unit with halves up
static inline void pg_fit_slot_resid(uint64_t n, int64_t sum_d, uint64_t dd_lo, uint64_t dd_hi, int64_t &mean, int64_t &rms) {
    const __int128 num = 2 * (__int128)sum_d + (__int128)n, den = 2 * (__int128)n;
    __int128 q = num / den;
    if (num - q * den < 0) q--; // floor
    mean = (int64_t)q;
    const unsigned __int128 dd = ((unsigned __int128)dd_hi << 64) | dd_lo, q4 = dd * 4 / n; // (dd < 2^126: the bound of the header, with room)
    rms = (int64_t)((pg_ev_isqrt((uint64_t)(q4 >> 64), (uint64_t)q4) + 1) >> 1);
}
// an integer of 1e-3 units with three decimals: -1 is "-0.001"
static inline std::string pg_fit_units_text(int64_t v) {
    char buf[40];
    const uint64_t a = v < 0 ? 0 - (uint64_t)v : (uint64_t)v;
    snprintf(buf, sizeof buf, "%s%llu.%03u", v < 0 ? "-" : "", (unsigned long long)(a / 1000), (unsigned)(a % 1000));
    return buf;
}

struct PgFitModel { uint32_t k = 0; bool uses_u = false; std::vector<uint32_t> levels; }; // levels[4^k], 0 = the k-mer is not in the file

// floor((2 mult |v| + 1) / 2) of a decimal text's value v: the nearest multiple of 1 / mult with halves up, exactly. 0, or 1: too many
// digits, 2: the result does not fit 32 bits.
static inline int pg_fit_round_dec(const pgbc::Dec &v, uint32_t mult, uint32_t &q_out) {
    pgbc::Big num = v.m, den, half, q;
    den.w[0] = 1; den.n = 1; half = den;
    if (!pgbc::big_muladd_small(num, 2 * mult, 0) || !pgbc::big_mul_pow10(den, v.scale) || !pgbc::big_mul_pow10(half, v.scale) || !pgbc::big_muladd_small(den, 2, 0) ||
        !pgbc::big_add(num, half, num))
        return 1;
    pgbc::big_div(num, den, q);
    if (q.n > 1) return 2;
    q_out = q.n ? q.w[0] : 0u;
    return 0;
}

// A model file in the format `poregen transform` writes. false: the model is refused, err names the line and the reason. stdvs (may be
// null: the column is not kept, a row may lack it): level_stdv of every slot in 1e-3 pA, rounded as the level is; with it a row without a
// level_stdv below 262.144 pA refuses the model (`poregen simulate`, pg_sim.h).
static inline bool pg_fit_parse_model_text(const char *text, size_t n, uint32_t want_k, PgFitModel &out, std::string &err, std::vector<uint32_t> *stdvs = nullptr) {
    PgFitModel md;
    std::vector<uint32_t> sd;
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
        if (len == 0 || ln[0] == '#' || (len >= 5 && memcmp(ln, "kmer\t", 5) == 0)) continue;
        const char *f[3]; size_t fl[3]; int nf = 0;
        for (size_t s = 0; nf < 3;) {
            const char *t = (const char *)memchr(ln + s, '\t', len - s);
            const size_t e = t ? (size_t)(t - ln) : len;
            f[nf] = ln + s; fl[nf] = e - s; nf++;
            if (!t) break;
            s = e + 1;
        }
        if (nf < 2) return fail("a row needs KMER<TAB>level_mean");
        const uint32_t k = (uint32_t)fl[0];
        if (fl[0] < 1 || fl[0] > PG_FIT_MAX_K) return fail("a k-mer has 1 to 9 letters");
        if (md.k == 0) {
            if (want_k && k != want_k) return fail("the model's k-mers have " + std::to_string(k) + " letters, -k says " + std::to_string(want_k));
            md.k = k; md.levels.assign((size_t)1 << (2 * k), 0u);
            if (stdvs) sd.assign((size_t)1 << (2 * k), 0u);
        } else if (k != md.k) return fail("k-mers of two lengths");
        uint32_t slot = 0;
        for (uint32_t j = 0; j < k; j++) {
            const char c = f[0][j];
            if (c == 'U') md.uses_u = true;
            const int b = pg_fit_base(c == 'U' ? 'T' : (uint32_t)(unsigned char)c);
            if (b < 0) return fail("a k-mer with a letter outside ACGTU");
            slot = slot * 4 + (uint32_t)b;
        }
        pgbc::Dec mean, stdv;
        if (!pgbc::parse(f[1], fl[1], mean)) return fail("level_mean is no number");
        if (nf > 2 && !pgbc::parse(f[2], fl[2], stdv)) return fail("level_stdv is no number");
        // L = floor((2000 m + 10^scale) / (2 * 10^scale)): the level in 1e-3 pA, the nearest unit with halves up, on the decimal text
        uint32_t lv = 0;
        const int rc = pg_fit_round_dec(mean, 1000, lv);
        if (rc == 1) return fail("level_mean has too many digits");
        if (mean.neg || rc || lv == 0 || lv >= PG_FIT_MAX_LEVEL) return fail("a level outside (0, 262.144) pA");
        if (md.levels[slot]) return fail("a k-mer twice");
        md.levels[slot] = lv;
        if (stdvs) {
            uint32_t sv = 0;
            if (nf < 3) return fail("a row needs KMER<TAB>level_mean<TAB>level_stdv");
            if (pg_fit_round_dec(stdv, 1000, sv) || (stdv.neg && sv != 0) || sv >= PG_FIT_MAX_LEVEL) return fail("a level_stdv outside [0, 262.144) pA");
            sd[slot] = sv;
        }
    }
    if (md.k == 0) { line_no = 0; err = "the model holds no k-mer"; return false; }
    if (stdvs) *stdvs = std::move(sd);
    out = std::move(md);
    return true;
}

// One read walked on the host by the rule the kernels follow: its counted events (first sample in the read, samples, slot) and the pass-1
// sums. false: out_of_signal (q < 0, or the ops run past the n_sig samples).
struct PgFitEvent { uint64_t start; uint32_t n; int32_t slot; };
static inline bool pg_fit_walk_host(const uint8_t *seq, uint32_t lb, const uint32_t *op_n, int64_t q, const int16_t *sig, uint64_t n_sig, const uint32_t *levels, uint32_t k,
                                    uint32_t m, bool rna, uint32_t min_dur, uint32_t max_dur, std::vector<PgFitEvent> &events, PgFitSums &sums) {
    events.clear(); sums = PgFitSums{0, 0, 0, 0, 0, 0, 0};
    uint64_t total = 0;
    for (uint32_t e = 0; e < lb; e++) total += op_n[e];
    if (q < 0 || (uint64_t)q > n_sig || total > n_sig - (uint64_t)q) return false;
    uint64_t pos = (uint64_t)q;
    for (uint32_t e = 0; e < lb; pos += op_n[e], e++) {
        uint32_t first;
        if (!pg_fit_kmer_at(lb, k, m, rna, e, first) || !pg_fit_dur_ok(op_n[e], min_dur, max_dur)) continue;
        const int32_t slot = pg_fit_code(seq, first, k);
        if (slot < 0 || !levels[slot]) continue;
        events.push_back(PgFitEvent{pos, op_n[e], slot});
        sums.e++;
        for (uint32_t t = 0; t < op_n[e]; t++) pg_fit_add(sums, sig[pos + t], (int32_t)levels[slot]);
    }
    return true;
}

// The sample and column totals of a gapped read. false: an op code above 2.
static inline bool pg_fit_gap_totals(const uint32_t *op_n, const uint8_t *op_t, uint32_t lb, uint64_t &samples, uint64_t &cols) {
    samples = cols = 0;
    for (uint32_t e = 0; e < lb; e++) {
        if (op_t[e] > PG_FIT_OP_D) return false;
        samples += pg_fit_op_samples(op_t[e], op_n[e]); cols += pg_fit_op_cols(op_t[e], op_n[e]);
    }
    return true;
}
// The status a gapped read has before any k-mer is read: PG_FIT_OK, PG_FIT_OUT_OF_SIGNAL or PG_FIT_REF_LENGTH
static inline uint32_t pg_fit_gap_status(int64_t q, uint64_t samples, uint64_t n_sig, uint64_t cols, uint64_t S) {
    if (q < 0 || (uint64_t)q > n_sig || samples > n_sig - (uint64_t)q) return PG_FIT_OUT_OF_SIGNAL;
    return S != cols ? PG_FIT_REF_LENGTH : PG_FIT_OK;
}
// pg_fit_walk_host for a gapped read: seq is the slice of S bases. Returns PG_FIT_OK, PG_FIT_OUT_OF_SIGNAL or PG_FIT_REF_LENGTH, -1 for
// an op code above 2, -2 for a slice above PG_FIT_MAX_SLICE (the library refuses such a batch).
static inline int pg_fit_gap_walk_host(const uint8_t *seq, uint64_t S, const uint32_t *op_n, const uint8_t *op_t, uint32_t lb, int64_t q, const int16_t *sig, uint64_t n_sig,
                                       const uint32_t *levels, uint32_t k, uint32_t m, bool rna, uint32_t min_dur, uint32_t max_dur, std::vector<PgFitEvent> &events, PgFitSums &sums) {
    events.clear(); sums = PgFitSums{0, 0, 0, 0, 0, 0, 0};
    uint64_t total, cols;
    if (!pg_fit_gap_totals(op_n, op_t, lb, total, cols)) return -1;
    if (S > PG_FIT_MAX_SLICE) return -2;
    const uint32_t st = pg_fit_gap_status(q, total, n_sig, cols, S);
    if (st != PG_FIT_OK) return (int)st;
    uint64_t pos = (uint64_t)q; uint32_t col = 0;
    for (uint32_t e = 0; e < lb; pos += pg_fit_op_samples(op_t[e], op_n[e]), col += pg_fit_op_cols(op_t[e], op_n[e]), e++) {
        uint32_t first;
        if (op_t[e] != PG_FIT_OP_MATCH || !pg_fit_dur_ok(op_n[e], min_dur, max_dur) || !pg_fit_gap_kmer_at(op_t, lb, (uint32_t)S, k, m, rna, e, col, first)) continue;
        const int32_t slot = pg_fit_code(seq, first, k);
        if (slot < 0 || !levels[slot]) continue;
        events.push_back(PgFitEvent{pos, op_n[e], slot});
        sums.e++;
        for (uint32_t t = 0; t < op_n[e]; t++) pg_fit_add(sums, sig[pos + t], (int32_t)levels[slot]);
    }
    return PG_FIT_OK;
}
