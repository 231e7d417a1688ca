// pg_realign.h -- the rule of `poregen realign`: the event boundaries of the basecaller's move table, which lie on multiples of the stride,
// moved by up to `band` samples each so that the samples fit the levels of a k-mer model best. Plain C++ that the kernels
// (pg_realign.hip), the library's host side and a host test (pg_hosttest.cpp: pgt_realign_*) all compile. Not installed.
//
// Input. A read as pg_fit.h walks it -- Lb bases, ops n_0 .. n_{Lb-1} (all matches), query_start q -- with the a and b its fit returned
// (status PG_FIT_OK) under the same model, m, rna, min_dur and max_dur. Parameters: band W (0 .. PG_RL_MAX_BAND), min_len
// (1 .. min_dur), max_dur <= PG_RL_MAX_DUR.
//
// A gapped read (PG_BATCH_GAPPED, pg_fit.h) is taken by the same rule: B advances by n for a match and an I and by 0 for a D, an event is
// refinable iff the gapped fit counts it -- an I or a D never is, so both boundaries beside it are pinned -- the pinned period counts ops, and
// the refined ops keep op_t and the op_n of every I and D.
//
// Boundaries. B_0 = q, B_e = q + n_0 + .. + n_{e-1}. Event e is REFINABLE iff it counts by fit's rule (pg_fit_kmer_at, pg_fit_code, a
// level, pg_fit_dur_ok); l_e is its level. Boundary e, 0 < e < Lb, is FREE iff events e - 1 and e are both refinable and
// e % PG_FIT_PIECE != phase (0 .. PG_FIT_PIECE - 1; 0 unless the caller asks); every other boundary is PINNED (B_0 and B_Lb too) and keeps
// its position. The pinned period cuts a read into PIECES that no run of free boundaries leaves: ops [0, min(phase, Lb)) when phase > 0,
// then [phase + 256 i, phase + 256 (i + 1)) cut at Lb (pg_rl_pieces, pg_rl_piece). Rounds that alternate the phase between 0 and 128 refine
// in one round what the other pins.
//
// Cost. A sample r_t under level l costs d^2, d = pg_fit_resid(r_t, a, 1.0 / b, l): fit's pass-2 residual, clamp included. Event e - 1
// laid on [p', p) costs the sum of those squares under l_{e-1}.
//
// Dynamic program, per maximal run of free boundaries e0 < e < e1 between the pinned P0 = B_{e0} and P1 = B_{e1}. A candidate for
// boundary e is p = B_e + j, |j| <= W, admissible iff P0 + (e - e0) min_len <= p <= P1 - (e1 - e) min_len. D[e0][P0] = 0; D[e][p] is
// the minimum of D[e-1][p'] + cost_{e-1}(p', p) over the reachable admissible p' with p' + min_len <= p; a tie takes the smallest p';
// a candidate without such a predecessor is not reachable. At e1 the only candidate is P1; the new boundaries are traced back from it.
// The original boundaries are admissible (a refinable event has n >= min_dur >= min_len), so there is always a solution and
// cost_after <= cost_before.
//
// Bounds (the static_asserts below). A run lies within one piece: at most PG_FIT_PIECE = 2^8 events of at most 2^12 + 2 * 31 < 2^13
// samples, each d^2 <= (2^18 - 1)^2 < 2^36: every D < 2^57, an int64. (The kernel drops what is constant per boundary and works with the
// window sums alone: 2 W < 2^6 samples per boundary, |value| < 2^8 * 2^6 * 2^36 = 2^50; it packs the lane into the low 6 bits of the
// value it scans: < 2^56.) A piece's cost is at most 2^8 * 2^13 * 2^36 = 2^57: a uint64 per piece on the device. A read of 2^24 counted
// samples, every boundary moved out by 31, has up to 2^24 + 62 * 2^24 samples: 2^30 * 2^36 passes 2^64, so the pieces' sums are
// added per read in 128 bits (k_rl_reads on the device, pg_rl_walk_host here).
#pragma once
#include "pg_fit.h"

#define PG_RL_MAX_BAND 31u                   // 2 W + 1 candidates fit a wave
#define PG_RL_MAX_DUR 4096u                  // the largest max_dur a realign handle takes
#define PG_RL_INF (1ll << 60)                // "not reachable" (values at or above half of it)
static_assert(2 * PG_RL_MAX_BAND + 1 <= PG_FIT_STEP, "a lane per candidate");
static_assert(PG_FIT_PIECE == 256 && PG_RL_MAX_DUR == 4096 && PG_FIT_CLAMP < (1 << 18), "the overflow argument above is written for 2^8 events of 2^12 samples and |d| < 2^18");
static_assert(8 + 13 + 36 <= 57 && 57 < 60, "every DP value stays below PG_RL_INF / 2 and a piece's cost fits a uint64");
static_assert(8 + 6 + 36 + 6 < 60, "the kernel's packed (value, lane) stays below PG_RL_INF / 2");
static_assert(2 * 18 <= 36 && 20 + 6 <= 32 && 36 - 20 + 6 <= 32, "a d^2 fits 36 bits, and 64 of its low 20 bits or of the 16 above them fit a 32-bit scan");

PG_FIT_HD bool pg_rl_params_ok(uint32_t band, uint32_t min_len, uint32_t min_dur, uint32_t max_dur) {
    return band <= PG_RL_MAX_BAND && min_len >= 1 && min_len <= min_dur && min_dur <= max_dur && max_dur <= PG_RL_MAX_DUR;
}
// the level of event e of a read when the event is refinable, else 0
template <class Seq> PG_FIT_HD uint32_t pg_rl_level(const Seq seq, uint32_t lb, uint32_t n, uint32_t e, const uint32_t *levels, uint32_t k, uint32_t m, bool rna, uint32_t min_dur,
                                                    uint32_t max_dur) {
    uint32_t first;
    if (!pg_fit_dur_ok(n, min_dur, max_dur) || !pg_fit_kmer_at(lb, k, m, rna, e, first)) return 0u;
    const int32_t code = pg_fit_code(seq, first, k);
    return code < 0 ? 0u : levels[code];
}
// the same for a gapped read (pg_fit.h: PG_BATCH_GAPPED): op e of type t in front of column col, the slice has S bases. An I or a D is
// never refinable, so both boundaries beside it are pinned; a D has no samples between them.
template <class Seq, class Ops> PG_FIT_HD uint32_t pg_rl_gap_level(const Seq seq, uint32_t S, const Ops op_t, uint32_t lb, uint32_t t, uint32_t n, uint32_t e, uint32_t col,
                                                                   const uint32_t *levels, uint32_t k, uint32_t m, bool rna, uint32_t min_dur, uint32_t max_dur) {
    uint32_t first;
    if (t != PG_FIT_OP_MATCH || !pg_fit_dur_ok(n, min_dur, max_dur) || !pg_fit_gap_kmer_at(op_t, lb, S, k, m, rna, e, col, first)) return 0u;
    const int32_t code = pg_fit_code(seq, first, k);
    return code < 0 ? 0u : levels[code];
}
PG_FIT_HD bool pg_rl_free(uint32_t e, uint32_t lb, uint32_t lvl_before, uint32_t lvl_at, uint32_t phase) {
    return e > 0 && e < lb && lvl_before && lvl_at && e % PG_FIT_PIECE != phase;
}
// the pieces of a read of lb ops: one in front of the first pinned boundary when 0 < phase, then one per period
PG_FIT_HD uint64_t pg_rl_pieces(uint64_t lb, uint32_t phase) {
    const uint64_t head = phase < lb ? phase : lb;
    return (head ? 1u : 0u) + (lb - head + PG_FIT_PIECE - 1) / PG_FIT_PIECE;
}
// piece j < pg_rl_pieces(lb, phase): its first op and its ops (1 .. PG_FIT_PIECE)
PG_FIT_HD void pg_rl_piece(uint32_t lb, uint32_t phase, uint32_t j, uint32_t &e0, uint32_t &cnt) {
    const uint32_t head = phase < lb ? phase : lb;
    if (head && j == 0) { e0 = 0; cnt = head; return; }
    e0 = head + (j - (head ? 1u : 0u)) * PG_FIT_PIECE;
    cnt = lb - e0 < PG_FIT_PIECE ? lb - e0 : PG_FIT_PIECE;
}
// the admissible positions of boundary e of the run (e0, e1) between P0 and P1: [lo, hi]
PG_FIT_HD void pg_rl_admissible(int64_t P0, int64_t P1, uint32_t e0, uint32_t e1, uint32_t e, uint32_t min_len, int64_t &lo, int64_t &hi) {
    lo = P0 + (int64_t)(e - e0) * min_len; hi = P1 - (int64_t)(e1 - e) * min_len;
}
PG_FIT_HD uint64_t pg_rl_cost(int32_t r, double a, double inv_b, uint32_t l) { bool c; const int64_t d = pg_fit_resid(r, a, inv_b, (int32_t)l, c); return (uint64_t)(d * d); }

// ---- host only: one read walked by the rule, the recurrence over all pairs of candidates as it is stated ---------------------------------
struct PgRlRead { uint32_t n_free = 0, n_moved = 0; uint64_t sum_abs_shift = 0; unsigned __int128 cost_before = 0, cost_after = 0; };

// op_out[lb]: the refined ops. false: out_of_signal (such a read has no fit), nothing is written. op_t != null: a gapped read whose slice
// seq has S bases (false as well for ref_length, an op code above 2 or a slice above PG_FIT_MAX_SLICE); the refined ops keep op_t and the
// op_n of every I and D.
static inline bool pg_rl_walk_any(const uint8_t *seq, uint64_t S, const uint8_t *op_t, uint32_t lb, const uint32_t *op_n, int64_t q, const int16_t *sig, uint64_t n_sig, const uint32_t *levels, uint32_t k, uint32_t m,
                                   bool rna, uint32_t min_dur, uint32_t max_dur, uint32_t band, uint32_t min_len, uint32_t phase, double a, double b, uint32_t *op_out,
                                   PgRlRead &out) {
    out = PgRlRead();
    uint64_t total = 0;
    if (op_t) {
        uint64_t cols;
        if (!pg_fit_gap_totals(op_n, op_t, lb, total, cols) || S > PG_FIT_MAX_SLICE || pg_fit_gap_status(q, total, n_sig, cols, S) != PG_FIT_OK) return false;
    } else {
        for (uint32_t e = 0; e < lb; e++) total += op_n[e];
        if (q < 0 || (uint64_t)q > n_sig || total > n_sig - (uint64_t)q) return false;
    }
    const double inv_b = 1.0 / b;
    const int64_t W = band;
    std::vector<int64_t> B(lb + 1), Bn;
    std::vector<uint32_t> lvl(lb + 1, 0u);
    B[0] = q;
    uint32_t col = 0;
    for (uint32_t e = 0; e < lb; e++) {
        if (op_t) {
            B[e + 1] = B[e] + pg_fit_op_samples(op_t[e], op_n[e]);
            lvl[e] = pg_rl_gap_level(seq, (uint32_t)S, op_t, lb, op_t[e], op_n[e], e, col, levels, k, m, rna, min_dur, max_dur);
            col += pg_fit_op_cols(op_t[e], op_n[e]);
        } else { B[e + 1] = B[e] + op_n[e]; lvl[e] = pg_rl_level(seq, lb, op_n[e], e, levels, k, m, rna, min_dur, max_dur); }
    }
    Bn = B;
    auto is_free = [&](uint32_t e) { return e > 0 && e < lb && pg_rl_free(e, lb, lvl[e - 1], lvl[e], phase); };
    auto cost = [&](uint32_t e, int64_t lo, int64_t hi) { unsigned __int128 s = 0; for (int64_t t = lo; t < hi; t++) s += pg_rl_cost(sig[t], a, inv_b, lvl[e]); return s; };
    const size_t nc = (size_t)(2 * W + 1);
    for (uint32_t e0 = 0; e0 < lb;) {
        if (!is_free(e0 + 1)) { e0++; continue; }
        uint32_t e1 = e0 + 1;
        while (is_free(e1)) e1++;
        const int64_t P0 = B[e0], P1 = B[e1];
        const uint32_t ne = e1 - e0;                                   // rows 0 .. ne: boundaries e0 .. e1
        std::vector<int64_t> D((size_t)(ne + 1) * nc, PG_RL_INF);
        std::vector<int32_t> from((size_t)(ne + 1) * nc, -1);
        D[(size_t)W] = 0;                                              // boundary e0: P0 alone
        for (uint32_t i = 1; i <= ne; i++) {
            const uint32_t e = e0 + i;
            int64_t lo, hi, plo, phi;
            pg_rl_admissible(P0, P1, e0, e1, e, min_len, lo, hi);
            pg_rl_admissible(P0, P1, e0, e1, e - 1, min_len, plo, phi);
            // S[x]: the cost of the samples [base, base + x) under l_{e-1}, over everything a pair of candidates can span
            const int64_t base = B[e - 1] - W > P0 ? B[e - 1] - W : P0, end = B[e] + W < P1 ? B[e] + W : P1;
            std::vector<int64_t> S((size_t)(end - base + 1), 0);
            for (int64_t t = base; t < end; t++) S[(size_t)(t - base + 1)] = S[(size_t)(t - base)] + (int64_t)pg_rl_cost(sig[t], a, inv_b, lvl[e - 1]);
            for (int64_t j = -W; j <= W; j++) {
                const int64_t p = B[e] + j;
                if (p < lo || p > hi || (i == ne && j != 0)) continue;
                for (int64_t jp = -W; jp <= W; jp++) {                  // ascending p': the first minimum is the smallest p'
                    const int64_t pp = B[e - 1] + jp, dp = D[(size_t)(i - 1) * nc + (size_t)(jp + W)];
                    if (pp < plo || pp > phi || (i == 1 && jp != 0) || dp >= PG_RL_INF / 2 || pp + (int64_t)min_len > p) continue;
                    const int64_t v = dp + (S[(size_t)(p - base)] - S[(size_t)(pp - base)]);
                    if (v < D[(size_t)i * nc + (size_t)(j + W)]) { D[(size_t)i * nc + (size_t)(j + W)] = v; from[(size_t)i * nc + (size_t)(j + W)] = (int32_t)(jp + W); }
                }
            }
        }
        int32_t c = (int32_t)W;
        for (uint32_t i = ne; i >= 1; i--) {
            c = from[(size_t)i * nc + (size_t)c];
            if (c < 0) return false;                                    // (cannot happen: the original boundaries are a solution)
            if (i > 1) Bn[e0 + i - 1] = B[e0 + i - 1] + (c - W);
        }
        e0 = e1;
    }
    for (uint32_t e = 0; e < lb; e++) {
        op_out[e] = op_t && op_t[e] != PG_FIT_OP_MATCH ? op_n[e] : (uint32_t)(Bn[e + 1] - Bn[e]);
        if (is_free(e)) { out.n_free++; const int64_t s = Bn[e] - B[e]; if (s) { out.n_moved++; out.sum_abs_shift += (uint64_t)(s < 0 ? -s : s); } }
        if (lvl[e]) { out.cost_before += cost(e, B[e], B[e + 1]); out.cost_after += cost(e, Bn[e], Bn[e + 1]); }
    }
    return true;
}
static inline bool pg_rl_walk_host(const uint8_t *seq, uint32_t lb, const uint32_t *op_n, int64_t q, const int16_t *sig, uint64_t n_sig, const uint32_t *levels, uint32_t k, uint32_t m,
                                   bool rna, uint32_t min_dur, uint32_t max_dur, uint32_t band, uint32_t min_len, uint32_t phase, double a, double b, uint32_t *op_out,
                                   PgRlRead &out) {
    return pg_rl_walk_any(seq, lb, nullptr, lb, op_n, q, sig, n_sig, levels, k, m, rna, min_dur, max_dur, band, min_len, phase, a, b, op_out, out);
}
