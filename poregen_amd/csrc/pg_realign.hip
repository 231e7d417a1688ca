// pg_realign.hip -- `poregen realign`: the boundaries of the basecaller's move table refined against a k-mer model (the rule: pg_realign.h).
//
// A batch is laid out as for pg_fit.hip, and the unit of work is the same: a read is cut into pieces of at most PG_FIT_PIECE = 256 ops, a
// WAVE takes a piece, a workgroup is four waves. The pieces end on the pinned boundaries, e % 256 == phase (pg_rl_piece: with a phase the
// first piece is the ops in front of boundary `phase`), so a run of free boundaries never leaves its piece and no wave needs another.
//   k_rl_span    per piece the sum of its ops' lengths and a look at op_t (a batch with an op that is no match is refused).
//   k_rl_starts  one wave per read: the sums scanned into every piece's first sample; a fitted read whose ops leave its samples raises the
//                refusal. The host waits for that word (and the op_t flag beside it) before any kernel indexes the signal.
//   k_rl_reads   one wave per read: the pieces' records of k_rl_align added into the read's 48 bytes, which is all that comes back.
//   k_rl_align   one piece by one wave:
//     1. lane j owns op j of a step of 64: its length, its level (0: not refinable), its first sample by a wave scan; the positions, levels
//        and the free boundaries (four 64-bit masks from ballots) go to the wave's LDS.
//     2. per run of free boundaries the dynamic program, boundary after boundary. Lane c = j + W owns the candidate B_e + j; lane i < 2 W
//        also owns the window's sample B_e - W + i. The cost of event e - 1 on [p', p) is S(p) - S(p') with S a prefix sum of d^2 under
//        the one level l_{e-1}, so
//            D[e][c'] = G_e(c') + min over c <= c' + n_{e-1} - min_len of (D[e-1][c] - F_{e-1}(c))
//        with G_e and F_e the EXCLUSIVE wave prefix sums of the window's d^2 under l_{e-1} and under l_e: what either leaves out of S is
//        the same for every candidate of the boundary and cancels in every argmin, and the costs come from step 4. The minimum is a wave
//        prefix-minimum of value * 64 + lane -- the smaller value wins, then the smaller lane, which is the rule's tie -- read at lane
//        c' + n_{e-1} - min_len (clipped to 2 W). A boundary costs two sum scans, one min scan and one shuffle instead of (2 W + 1)^2
//        steps. Candidates that are not admissible are masked before their samples are loaded: a sample is loaded only inside
//        [lowest admissible candidate, highest admissible candidate), which lies inside [P0, P1). The window of boundary e + 1 is
//        requested before the scans of boundary e run.
//     3. the back-pointers, one byte per (boundary, lane), are in the wave's LDS (16 KiB per piece: no scratch buffer to size, no global
//        round trip in the sequential part); the traceback is a chain of wave-uniform reads that leaves every boundary's shift in LDS.
//     4. the refined ops, the counts, and both costs: lane j takes the samples of the union of the old and the new span of ITS event of a
//        step once and adds d^2 to either sum. Per piece two 64-bit sums; k_rl_reads adds a read's pieces in 128 bits.
// Every number is an integer behind pg_fit_resid; nothing depends on the order of execution. No workgroup waits for another, and the four
// waves of a workgroup never meet.
// Gapped batches (PG_BATCH_GAPPED; the rule: pg_fit.h, pg_realign.h) run the <kGapped = true> instances: k_rl_span adds a piece's reference
// columns, k_rl_starts scans them into every piece's first column and raises the refusal for a read whose slice does not fit them, and
// step 1 of k_rl_align reads op_t -- a D takes no samples, a third wave scan gives the column, an I or a D has no level and so pins both
// boundaries beside it. Step 4 writes a D's op_n back as it was. Steps 2 and 3 and the LDS layout are untouched.
#include "../../include/pgmove.h"
#include <hip/hip_runtime.h>
#include "pg_realign.h"
#include "pg_dev.h"
#include "pg_hip_host.h"

#include <cmath>
#include <cstring>
#include <string>
#include <vector>

static_assert(sizeof(pg_realign_read) == 48, "a read's result is 48 bytes");

namespace {

constexpr int kWave = WAVE;
constexpr int kThreads = PG_FIT_THREADS;
constexpr int kWaves = kThreads / kWave;
constexpr uint32_t kPiece = PG_FIT_PIECE;
constexpr uint32_t kSteps = kPiece / kWave;
constexpr uint32_t kUnroll = 4;        // samples a lane has in flight in the cost pass
constexpr int64_t kKeyInf = 1ll << 62; // the packed (value, lane) of a candidate that is not reachable
typedef unsigned long long u64;
static_assert(PG_FIT_STEP == kWave && kSteps == 4, "four steps of one op per lane; the free boundaries are four 64-bit masks");

struct RlBatch {
    const int16_t *sig; const uint64_t *sig_off;
    const uint8_t *seq; const uint64_t *seq_off;
    const uint32_t *op_n; const uint8_t *op_t; const uint64_t *op_off;
    const uint32_t *piece_read, *piece_first; // the read of every piece; the first piece of every read (n_reads + 1)
    const uint64_t *piece_start;              // the first sample of the piece's first op, counted in its read (query_start included)
    const uint64_t *piece_col;                // gapped batches: the reference column in front of the piece's first op
    const uint8_t *part;                     // per read: it is refined
    const int32_t *qs;                        // per read: query_start
    const uint32_t *levels;
    const double *ab;                         // a and 1 / b of every read
    uint32_t n_reads, n_pieces, k, m, rna, min_dur, max_dur, band, min_len, phase;
};
struct RlPiece { uint32_t n_free, n_moved; u64 sum_abs, cost_before, cost_after; }; // 32 bytes per piece
static_assert(sizeof(RlPiece) == 32, "the pieces' results come back as 32 bytes each");

struct RlLds {
    uint64_t pos[kPiece + 1];      // the first sample of every op of the piece in its read; pos[ops of the piece ..] = one past the last
    uint32_t lvl[kPiece];          // 0: the event is not refinable
    uint64_t freem[kSteps];        // bit i of the 256: boundary i of the piece is free
    int8_t shift[kPiece + 8];      // new - old position of every boundary
    uint8_t bp[kPiece * kWave];    // bp[(i - 1) * 64 + c]: the lane of boundary i - 1 that candidate c of boundary i comes from
};

// LDS written by some lanes of a wave and read by others of the same wave (as in pg_fit.hip)
__device__ __forceinline__ void wave_lds_sync() {
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}
__device__ __forceinline__ u64 wave_sum(u64 v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, kWave);
    return v;
}
// a value every lane holds alike, as a scalar
__device__ __forceinline__ uint32_t uni(uint32_t v) { return (uint32_t)__builtin_amdgcn_readfirstlane((int)v); }
__device__ __forceinline__ uint64_t uni64(uint64_t v) { return (uint64_t)uni((uint32_t)v) | ((uint64_t)uni((uint32_t)(v >> 32)) << 32); }

// Inclusive wave prefix-minimum of signed 64-bit values, in the shape of wave_incl_scan_u32 (pg_dev.h): DPP row shifts, then the row
// broadcasts. A lane without a source keeps its own value (bound_ctrl off, old = the value itself), and min(v, v) = v.
template <int CTRL, int ROW_MASK> __device__ __forceinline__ int64_t dpp_keep_i64(int64_t x) {
    const int lo = (int)(uint32_t)(uint64_t)x, hi = (int)(uint32_t)((uint64_t)x >> 32);
    const uint32_t tl = (uint32_t)__builtin_amdgcn_update_dpp(lo, lo, CTRL, ROW_MASK, 0xF, false), th = (uint32_t)__builtin_amdgcn_update_dpp(hi, hi, CTRL, ROW_MASK, 0xF, false);
    return (int64_t)(((uint64_t)th << 32) | tl);
}
__device__ __forceinline__ int64_t wave_incl_min_i64(int64_t v) {
    int64_t t;
    t = dpp_keep_i64<0x111, 0xF>(v); v = t < v ? t : v; // row_shr:1
    t = dpp_keep_i64<0x112, 0xF>(v); v = t < v ? t : v; // row_shr:2
    t = dpp_keep_i64<0x114, 0xF>(v); v = t < v ? t : v; // row_shr:4
    t = dpp_keep_i64<0x118, 0xF>(v); v = t < v ? t : v; // row_shr:8
    t = dpp_keep_i64<0x142, 0xA>(v); v = t < v ? t : v; // row_bcast:15 -> rows 1 and 3
    t = dpp_keep_i64<0x143, 0xC>(v); v = t < v ? t : v; // row_bcast:31 -> rows 2 and 3
    return v;
}
// Exclusive wave prefix sum of values below 2^36 (a d^2), as two 32-bit DPP scans: the low 20 bits (64 of them stay below 2^26) and the
// rest (below 2^16 each, 2^22 together)
__device__ __forceinline__ u64 wave_excl_sum_36(u64 v) {
    const uint32_t lo = wave_incl_scan_u32((uint32_t)v & 0xfffffu), hi = wave_incl_scan_u32((uint32_t)(v >> 20));
    return (((u64)hi << 20) + lo) - v;
}

struct RlGeo { uint32_t r, e0, cnt, lb; uint64_t o0, s0, sig0; };
__device__ __forceinline__ RlGeo rl_geo(const RlBatch &B, uint32_t pid) {
    RlGeo g;
    g.r = B.piece_read[pid];
    g.o0 = B.op_off[g.r];
    g.lb = (uint32_t)(B.op_off[g.r + 1] - g.o0);
    pg_rl_piece(g.lb, B.phase, pid - B.piece_first[g.r], g.e0, g.cnt);
    g.cnt = min(kPiece, g.cnt);                                           // (it is: said once more where the compiler sees it, as before the phase)
    g.s0 = B.seq_off[g.r]; g.sig0 = B.sig_off[g.r];
    return g;
}

// flag[0]: bit 0 an op that is no match, bit 1 an op code above 2. Gapped: pcol gets the piece's reference columns beside its samples.
template <bool kGapped> __global__ __launch_bounds__(kThreads) void k_rl_span(const RlBatch B, uint64_t *__restrict__ psum, uint64_t *__restrict__ pcol, uint32_t *__restrict__ flag) {
    const uint32_t lane = threadIdx.x & (kWave - 1), pid = blockIdx.x * kWaves + threadIdx.x / kWave;
    if (pid >= B.n_pieces) return;                                        // (the whole wave)
    const RlGeo g = rl_geo(B, pid);
    u64 s = 0, c = 0; uint32_t bad = 0;
    for (uint32_t i = lane; i < g.cnt; i += kWave) {
        const uint32_t n = B.op_n[g.o0 + g.e0 + i], t = B.op_t[g.o0 + g.e0 + i];
        bad |= t > PG_FIT_OP_D ? 2u : t ? 1u : 0u;
        if (kGapped) { s += pg_fit_op_samples(t, n); c += pg_fit_op_cols(t, n); } else s += n;
    }
    s = wave_sum(s);
    if (kGapped) c = wave_sum(c);
    bad = (__any(bad & 1u) ? 1u : 0u) | (__any(bad & 2u) ? 2u : 0u);
    if (bad && lane == 0) atomicOr(flag, bad);
    if (lane == 0) { psum[pid] = s; if (kGapped) pcol[pid] = c; }
}

// One wave per read: the pieces' sums scanned into every piece's first sample, 64 pieces a step. A read that is to be refined and does not
// lie inside its samples raises the refusal: the smallest such read's index into flag[1], which starts at UINT32_MAX. Nothing here indexes
// the signal. A read has fewer than 2^31 ops of fewer than 2^32 samples and a query_start below 2^31: every sum stays below 2^64.
static_assert(31 + 32 < 64, "a read's samples, summed over its ops, fit a uint64");
// Gapped: the columns are scanned beside the samples (fewer than 2^31 ops of fewer than 2^32 columns: below 2^63), and flag[1] gets
// 2 r for a read whose ops leave its samples, 2 r + 1 for one whose slice has not as many bases as its ops have columns -- the smallest
// read, and of its two reasons the first, as fit ranks them.
template <bool kGapped> __global__ __launch_bounds__(kThreads) void k_rl_starts(const RlBatch B, const uint64_t *__restrict__ psum, const uint64_t *__restrict__ pcsum,
                                                                                uint64_t *__restrict__ piece_start, uint64_t *__restrict__ piece_col, uint32_t *__restrict__ flag) {
    const uint32_t lane = threadIdx.x & (kWave - 1), r = blockIdx.x * kWaves + threadIdx.x / kWave;
    if (r >= B.n_reads) return;                                           // (the whole wave)
    const uint32_t p0 = B.piece_first[r], p1 = B.piece_first[r + 1];
    const int32_t q = B.qs[r];
    uint64_t at = q < 0 ? 0ull : (uint64_t)q, col = 0;
    for (uint32_t p = p0; p < p1; p += kWave) {                           // (uniform)
        const uint32_t i = p + lane;
        const uint64_t v = i < p1 ? psum[i] : 0ull, incl = wave_incl_scan_u64(v);
        if (i < p1) piece_start[i] = at + (incl - v);
        at += __shfl(incl, kWave - 1, kWave);
        if (kGapped) {
            const uint64_t cv = i < p1 ? pcsum[i] : 0ull, cincl = wave_incl_scan_u64(cv);
            if (i < p1) piece_col[i] = col + (cincl - cv);
            col += __shfl(cincl, kWave - 1, kWave);
        }
    }
    const bool out = q < 0 || at > B.sig_off[r + 1] - B.sig_off[r];
    if (!kGapped) { if (lane == 0 && B.part[r] && out) atomicMin(flag + 1, r); }
    else if (lane == 0 && B.part[r] && (out || col != B.seq_off[r + 1] - B.seq_off[r])) atomicMin(flag + 1, 2u * r + (out ? 0u : 1u));
}

// the first set bit of the 256 at or behind i, or 256; with `clear`, the first bit that is not set
__device__ __forceinline__ uint32_t next_bit(const RlLds &L, uint32_t i, bool clear) {
    for (uint32_t w = i >> 6; w < kSteps; w++) {
        uint64_t bits = uni64(L.freem[w]);
        if (clear) bits = ~bits;
        if (w == (i >> 6)) bits &= ~0ull << (i & 63u);
        if (bits) return w * 64u + (uint32_t)__builtin_ctzll(bits);
    }
    return kPiece;
}

template <bool kGapped> __global__ __launch_bounds__(kThreads) void k_rl_align(const RlBatch B, uint32_t *__restrict__ out_n, RlPiece *__restrict__ pstats) {
    __shared__ RlLds lds[kWaves];
    const uint32_t lane = threadIdx.x & (kWave - 1), w = threadIdx.x / kWave, pid = blockIdx.x * kWaves + w;
    if (pid >= B.n_pieces) return;                                        // (the whole wave; this kernel has no workgroup barrier)
    const RlGeo g = rl_geo(B, pid);
    const uint32_t *__restrict__ op_n = B.op_n + g.o0 + g.e0;
    uint32_t *__restrict__ out = out_n + g.o0 + g.e0;
    if (!B.part[g.r]) {                                                   // not refined: the ops as they are, zeros
        for (uint32_t i = lane; i < g.cnt; i += kWave) out[i] = op_n[i];
        if (lane == 0) pstats[pid] = RlPiece{0, 0, 0, 0, 0};
        return;
    }
    RlLds &L = lds[w];
    const int16_t *__restrict__ sig = B.sig + g.sig0;
    const double a = B.ab[2ull * g.r], inv_b = B.ab[2ull * g.r + 1];
    const int32_t W = (int32_t)B.band, min_len = (int32_t)B.min_len;

    // ---- 1. positions, levels, free boundaries
    uint64_t ref[kSteps];
    {
        uint64_t pos = B.piece_start[pid];
        // gapped: a D takes no samples, and a third scan gives the op's column, carried from step to step as pos is (a read that is
        // refined has as many columns as its slice has bases, below 2^32)
        const uint32_t S = kGapped ? (uint32_t)(B.seq_off[g.r + 1] - g.s0) : 0u;
        uint32_t col = kGapped ? (uint32_t)B.piece_col[pid] : 0u;
#pragma unroll
        for (uint32_t st = 0; st < kSteps; st++) {
            const uint32_t i = st * kWave + lane;
            uint32_t n = i < g.cnt ? op_n[i] : 0u, lvl;
            if (kGapped) {
                const uint32_t t = i < g.cnt ? B.op_t[g.o0 + g.e0 + i] : (uint32_t)PG_FIT_OP_I, cols = pg_fit_op_cols(t, n), colincl = wave_incl_scan_u32(cols);
                lvl = i < g.cnt ? pg_rl_gap_level(B.seq + g.s0, S, B.op_t + g.o0, g.lb, t, n, g.e0 + i, col + (colincl - cols), B.levels, B.k, B.m, B.rna != 0, B.min_dur, B.max_dur) : 0u;
                col += (uint32_t)__shfl((int)colincl, kWave - 1, kWave);
                n = pg_fit_op_samples(t, n);
            } else lvl = i < g.cnt ? pg_rl_level(B.seq + g.s0, g.lb, n, g.e0 + i, B.levels, B.k, B.m, B.rna != 0, B.min_dur, B.max_dur) : 0u;
            const uint64_t incl = wave_incl_scan_u64(n);
            L.pos[i] = pos + (incl - n); L.lvl[i] = lvl; L.shift[i] = 0;
            ref[st] = __ballot(lvl != 0);
            pos += __shfl(incl, kWave - 1, kWave);
        }
        if (lane == 0) { L.pos[kPiece] = pos; L.shift[kPiece] = 0; }
    }
    uint32_t n_free = 0;
#pragma unroll
    for (uint32_t st = 0; st < kSteps; st++) { // boundary i is free iff ops i - 1 and i are refinable; boundary 0 of a piece is a pinned one (pg_rl_piece), bits from cnt on are clear
        const uint64_t fm = ref[st] & ((ref[st] << 1) | (st ? ref[st - 1] >> 63 : 0ull));
        if (lane == 0) L.freem[st] = fm;
        n_free += (uint32_t)__popcll(fm);
    }
    wave_lds_sync();

    // ---- 2. and 3. run after run
    for (uint32_t at = 1;;) {
        const uint32_t f = next_bit(L, at, false);
        if (f >= kPiece) break;
        const uint32_t r0 = f - 1, r1 = next_bit(L, f, true);             // the pinned boundaries around the run: r0 < f <= r1 - 1, r1 <= cnt
        const int64_t P0 = (int64_t)uni64(L.pos[r0]), P1 = (int64_t)uni64(L.pos[r1]);
        // the window of boundary e: lane i < 2 W holds sample B_e - W + i where a candidate can use it
        auto window = [&](uint32_t e, int64_t Be, bool &have) {
            const int64_t p = Be - W + (int64_t)lane, lo = P0 + (int64_t)(e - r0) * min_len, hi = P1 - (int64_t)(r1 - e) * min_len;
            have = e < r1 && (int32_t)lane < 2 * W && p >= lo && p < hi;
            return have ? (int32_t)sig[p] : 0;
        };
        int64_t A = (int32_t)lane == W ? 0 : PG_RL_INF;                   // D - F of boundary r0: P0 alone
        int64_t Bprev = P0, Bnext = (int64_t)uni64(L.pos[r0 + 1]);
        bool have_next;
        int32_t raw_next = window(r0 + 1, Bnext, have_next);
        for (uint32_t e = r0 + 1; e <= r1; e++) {                         // (uniform)
            const int64_t Be = Bnext;
            const int32_t raw = raw_next; const bool have = have_next;
            if (e < r1) { Bnext = (int64_t)uni64(L.pos[e + 1]); raw_next = window(e + 1, Bnext, have_next); }
            const uint32_t l_prev = uni(L.lvl[e - 1]), l_at = e < kPiece ? uni(L.lvl[e]) : 0u;
            const int64_t p = Be - W + (int64_t)lane, lo = P0 + (int64_t)(e - r0) * min_len, hi = P1 - (int64_t)(r1 - e) * min_len;
            const bool adm = e < r1 ? ((int32_t)lane <= 2 * W && p >= lo && p <= hi) : (int32_t)lane == W;
            const u64 cg = have ? pg_rl_cost(raw, a, inv_b, l_prev) : 0ull, cf = have && l_at ? pg_rl_cost(raw, a, inv_b, l_at) : 0ull;
            const int64_t G = (int64_t)wave_excl_sum_36(cg), F = (int64_t)wave_excl_sum_36(cf);
            const int64_t key = wave_incl_min_i64(A >= PG_RL_INF / 2 ? kKeyInf : A * 64 + (int64_t)lane);
            const int64_t s = (int64_t)lane + (Be - Bprev) - min_len;     // the last lane of boundary e - 1 that leaves min_len samples
            const int64_t best = (int64_t)__shfl((long long)key, (int)(s < 0 ? 0 : s > 2 * W ? 2 * W : s), kWave);
            const bool reach = adm && s >= 0 && best < kKeyInf / 2;
            L.bp[(e - 1) * kWave + lane] = reach ? (uint8_t)(best & 63) : (uint8_t)0xff;
            A = reach ? G + (best >> 6) - F : PG_RL_INF;
            Bprev = Be;
        }
        wave_lds_sync();
        uint32_t c = (uint32_t)W;
        for (uint32_t e = r1; e > r0 + 1; e--) {                          // boundary e - 1 is free
            c = uni(L.bp[(e - 1) * kWave + c]) & 63u;
            if (lane == 0) L.shift[e - 1] = (int8_t)((int32_t)c - W);
        }
        at = r1 + 1;
    }
    wave_lds_sync();

    // ---- 4. the refined ops, the counts, the costs
    u64 moved = 0, abs_shift = 0, cost_before = 0, cost_after = 0;
    for (uint32_t st = 0; st * kWave < g.cnt; st++) {                      // (uniform)
        const uint32_t i = st * kWave + lane;
        const bool valid = i < g.cnt;
        const int32_t s_lo = valid ? L.shift[i] : 0, s_hi = valid ? L.shift[i + 1] : 0;
        const uint64_t o_lo = valid ? L.pos[i] : 0, o_hi = valid ? L.pos[i + 1] : 0;
        const uint32_t lvl = valid ? L.lvl[i] : 0u;
        if (kGapped && valid && B.op_t[g.o0 + g.e0 + i] == PG_FIT_OP_D) out[i] = op_n[i]; // (its columns; an I keeps its samples below: both boundaries are pinned)
        else if (valid) out[i] = (uint32_t)((int64_t)(o_hi - o_lo) + s_hi - s_lo);
        moved += s_lo != 0 ? 1u : 0u; abs_shift += (u64)(s_lo < 0 ? -s_lo : s_lo);
        const int64_t n_lo = (int64_t)o_lo + s_lo, n_hi = (int64_t)o_hi + s_hi;
        // the costs: every lane walks the union of the old and the new span of ITS event, four samples in flight; neighbouring lanes
        // read neighbouring events, and a lane's next round hits the lines its last one brought
        const int64_t lo = o_lo < (uint64_t)n_lo ? (int64_t)o_lo : n_lo, hi = (int64_t)o_hi > n_hi ? (int64_t)o_hi : n_hi;
        const uint32_t len = lvl ? (uint32_t)(hi - lo) : 0u;              // (a refinable event has at most 4096 + 62 samples)
        for (uint32_t it = 0; __any(it < len); it += kUnroll) {
            int32_t raw[kUnroll];
#pragma unroll
            for (uint32_t u = 0; u < kUnroll; u++) raw[u] = it + u < len ? (int32_t)sig[lo + it + u] : 0;
#pragma unroll
            for (uint32_t u = 0; u < kUnroll; u++) {
                const int64_t t = lo + it + u;
                const u64 cst = it + u < len ? pg_rl_cost(raw[u], a, inv_b, lvl) : 0ull;
                cost_before += t >= (int64_t)o_lo && t < (int64_t)o_hi ? cst : 0ull;
                cost_after += t >= n_lo && t < n_hi ? cst : 0ull;
            }
        }
    }
    moved = wave_sum(moved); abs_shift = wave_sum(abs_shift); cost_before = wave_sum(cost_before); cost_after = wave_sum(cost_after);
    if (lane == 0) pstats[pid] = RlPiece{n_free, (uint32_t)moved, abs_shift, cost_before, cost_after};
}

// One wave per read: its pieces' records added into the read's. A read has fewer than 2^31 ops, so fewer than 2^24 pieces (phase 0: 2^23;
// a phase adds one): the counts stay below 2^31, the shifts below 2^31 * 31 < 2^36. A piece's cost is below 2^57 (pg_realign.h); the low
// and the high 32 bits of the pieces' costs are summed apart -- below 2^32 * 2^24 and 2^25 * 2^24, a uint64 each over the whole read, in
// any order -- and put together as a 128-bit number at the end: lo + hi * 2^32, with the carry.
static_assert(PG_FIT_PIECE == 256 && 31 - 8 + 1 <= 24 && 32 + 24 < 64 && 57 - 32 + 24 < 64, "the halves of the pieces' costs add up in 64 bits");
__device__ __forceinline__ void put_128(u64 lo_sum, u64 hi_sum, uint64_t &lo, uint64_t &hi) {
    lo = lo_sum + (hi_sum << 32);
    hi = (hi_sum >> 32) + (lo < lo_sum ? 1ull : 0ull);
}
__global__ __launch_bounds__(kThreads) void k_rl_reads(const RlBatch B, const RlPiece *__restrict__ pstats, pg_realign_read *__restrict__ reads) {
    const uint32_t lane = threadIdx.x & (kWave - 1), r = blockIdx.x * kWaves + threadIdx.x / kWave;
    if (r >= B.n_reads) return;                                           // (the whole wave)
    const uint32_t p0 = B.piece_first[r], p1 = B.piece_first[r + 1];
    u64 n_free = 0, n_moved = 0, sum_abs = 0, b_lo = 0, b_hi = 0, a_lo = 0, a_hi = 0;
    for (uint32_t p = p0 + lane; p < p1; p += kWave) {
        const RlPiece q = pstats[p];
        n_free += q.n_free; n_moved += q.n_moved; sum_abs += q.sum_abs;
        b_lo += q.cost_before & 0xffffffffull; b_hi += q.cost_before >> 32;
        a_lo += q.cost_after & 0xffffffffull; a_hi += q.cost_after >> 32;
    }
    n_free = wave_sum(n_free); n_moved = wave_sum(n_moved); sum_abs = wave_sum(sum_abs);
    b_lo = wave_sum(b_lo); b_hi = wave_sum(b_hi); a_lo = wave_sum(a_lo); a_hi = wave_sum(a_hi);
    if (lane == 0) {
        pg_realign_read o;
        o.n_free = (uint32_t)n_free; o.n_moved = (uint32_t)n_moved; o.sum_abs_shift = sum_abs;
        put_128(b_lo, b_hi, o.cost_before_lo, o.cost_before_hi); put_128(a_lo, a_hi, o.cost_after_lo, o.cost_after_hi);
        reads[r] = o;
    }
}

} // namespace

struct pg_realign {
    int device = 0;
    pg_realign_params prm{};
    PgStream own;
    hipStream_t s = nullptr;
    PgEvent ev[2];
    uint32_t k = 0;
    double ms = 0;
    int cur = 0;                   // d_out[cur] holds the last submit's ops; the next one writes the other
    bool busy = false;             // a submit left work queued (it failed half way)
    PgDev<uint32_t> d_levels, d_opn, d_pread, d_pfirst, d_out[2], d_flag;
    PgDev<int16_t> d_sig;
    PgDev<int32_t> d_qs;
    PgDev<uint64_t> d_sigoff, d_seqoff, d_opoff, d_pstart, d_psum, d_pcol, d_pcsum; // (d_pcol, d_pcsum: gapped batches)
    PgDev<uint8_t> d_seq, d_opt, d_part;
    PgDev<RlPiece> d_pstats;
    PgDev<pg_realign_read> d_reads;
    PgDev<double> d_ab;
    std::vector<uint64_t> sig_off, seq_off, op_off;
    std::vector<int32_t> qs;
    std::vector<uint32_t> piece_read, piece_first;
    std::vector<uint8_t> part;
    std::vector<double> ab;
    std::vector<pg_realign_read> reads;
    std::string err;
};

static pg_status rl_check_params(pg_realign *h, const pg_realign_params *p, const char *who) {
    if (p->struct_size != sizeof(pg_realign_params)) return pg_fail(h, PG_ERR_INVALID_ARG, "%s: struct_size %u, this library has %zu", who, p->struct_size, sizeof(pg_realign_params));
    if (!pg_rl_params_ok(p->band, p->min_len, p->min_dur, p->max_dur))
        return pg_fail(h, PG_ERR_INVALID_ARG, "%s: band <= %u, 1 <= min_len <= min_dur <= max_dur <= %u are required (got band %u, min_len %u, min_dur %u, max_dur %u)", who, PG_RL_MAX_BAND,
                       PG_RL_MAX_DUR, p->band, p->min_len, p->min_dur, p->max_dur);
    if (p->sig_move_offset > 64) return pg_fail(h, PG_ERR_INVALID_ARG, "%s: sig_move_offset %u (at most 64)", who, p->sig_move_offset);
    if (p->phase >= kPiece) return pg_fail(h, PG_ERR_INVALID_ARG, "%s: phase %u (0 to %u)", who, p->phase, kPiece - 1);
    return PG_OK;
}

extern "C" {

const char *pg_realign_last_error(const pg_realign *h) { return h ? h->err.c_str() : pg_create_error<pg_realign>().c_str(); }

pg_status pg_realign_create(const pg_realign_params *p, int32_t device, pg_realign **out) {
    if (!out || !p) return pg_fail<pg_realign>(nullptr, PG_ERR_INVALID_ARG, "pg_realign_create: null argument");
    *out = nullptr;
    if (pg_status st = rl_check_params(nullptr, p, "pg_realign_create")) return st;
    if (pg_status st = pg_select_device<pg_realign>(device)) return st;
    pg_realign *h = new pg_realign();
    h->device = device; h->prm = *p;
    hipError_t e = hipStreamCreateWithFlags(&h->own.h, hipStreamNonBlocking);
    for (int i = 0; i < 2 && e == hipSuccess; i++) e = hipEventCreate(&h->ev[i].h);
    if (e != hipSuccess) {
        pg_fail(h, PG_ERR_HIP, "pg_realign_create: %s", hipGetErrorString(e));
        return pg_create_failed(h, PG_ERR_HIP, pg_realign_destroy);
    }
    h->s = h->own;
    *out = h;
    return PG_OK;
}

void pg_realign_destroy(pg_realign *h) {
    if (!h) return;
    (void)hipSetDevice(h->device);
    if (h->s) (void)hipStreamSynchronize(h->s);
    delete h;
}

pg_status pg_realign_set_stream(pg_realign *h, void *hip_stream) {
    if (!h) return pg_fail<pg_realign>(nullptr, PG_ERR_INVALID_ARG, "pg_realign_set_stream: null handle");
    PG_HIP_TRY(h, hipSetDevice(h->device));
    PG_HIP_TRY(h, hipStreamSynchronize(h->s));
    h->s = hip_stream ? (hipStream_t)hip_stream : (hipStream_t)h->own;
    return PG_OK;
}

pg_status pg_realign_set_phase(pg_realign *h, uint32_t phase) {
    if (!h) return pg_fail<pg_realign>(nullptr, PG_ERR_INVALID_ARG, "pg_realign_set_phase: null handle");
    if (phase >= kPiece) return pg_fail(h, PG_ERR_INVALID_ARG, "pg_realign_set_phase: phase %u (0 to %u)", phase, kPiece - 1);
    h->prm.phase = phase;
    return PG_OK;
}

pg_status pg_realign_kernel_ms(pg_realign *h, double *ms) {
    if (!h) return pg_fail<pg_realign>(nullptr, PG_ERR_INVALID_ARG, "pg_realign_kernel_ms: null handle");
    if (ms) *ms = h->ms;
    h->ms = 0;
    return PG_OK;
}

pg_status pg_realign_set_model(pg_realign *h, const uint32_t *levels, uint32_t k) {
    if (!h) return pg_fail<pg_realign>(nullptr, PG_ERR_INVALID_ARG, "pg_realign_set_model: null handle");
    if (!levels || k < 1 || k > PG_FIT_MAX_K) return pg_fail(h, PG_ERR_INVALID_ARG, "pg_realign_set_model: levels and a kmer_size of 1 to %u are required", PG_FIT_MAX_K);
    const uint64_t ns = 1ull << (2 * k);
    for (uint64_t i = 0; i < ns; i++)
        if (levels[i] >= PG_FIT_MAX_LEVEL) return pg_fail(h, PG_ERR_INVALID_ARG, "pg_realign_set_model: level %u of slot %llu (levels lie below %u)", levels[i], (unsigned long long)i, PG_FIT_MAX_LEVEL);
    PG_HIP_TRY(h, hipSetDevice(h->device));
    PG_HIP_TRY(h, hipStreamSynchronize(h->s));
    PG_HIP_TRY(h, h->d_levels.ensure(ns * sizeof(uint32_t)));
    PG_HIP_TRY(h, h->d_flag.ensure(2 * sizeof(uint32_t)));
    PG_HIP_TRY(h, hipMemcpyAsync(h->d_levels.p, levels, ns * sizeof(uint32_t), hipMemcpyHostToDevice, h->s));
    PG_HIP_TRY(h, hipStreamSynchronize(h->s));
    h->k = k;
    return PG_OK;
}

pg_status pg_realign_submit(pg_realign *h, const pg_batch *b, const uint32_t *status, const double *a, const double *bb, pg_realign_reads *out) {
    if (!h) return pg_fail<pg_realign>(nullptr, PG_ERR_INVALID_ARG, "pg_realign_submit: null handle");
    if (!b || !out) return pg_fail(h, PG_ERR_INVALID_ARG, "pg_realign_submit: null argument");
    if (out->struct_size != sizeof(pg_realign_reads)) return pg_fail(h, PG_ERR_INVALID_ARG, "pg_realign_submit: pg_realign_reads.struct_size %u, this library has %zu", out->struct_size, sizeof(pg_realign_reads));
    memset(out, 0, sizeof *out); out->struct_size = sizeof *out;
    if (!h->k) return pg_fail(h, PG_ERR_STATE, "pg_realign_submit: no model (pg_realign_set_model)");
    if (b->struct_size != sizeof(pg_batch)) return pg_fail(h, PG_ERR_INVALID_ARG, "pg_realign_submit: pg_batch.struct_size %u, this library has %zu", b->struct_size, sizeof(pg_batch));
    if (b->location != PG_LOC_HOST && b->location != PG_LOC_DEVICE) return pg_fail(h, PG_ERR_INVALID_ARG, "pg_realign_submit: location must be PG_LOC_HOST or PG_LOC_DEVICE");
    const bool gapped = (b->flags & PG_BATCH_GAPPED) != 0;
    if (gapped && (b->flags & PG_BATCH_ALL_MATCHES)) return pg_fail(h, PG_ERR_INVALID_ARG, "pg_realign_submit: a batch carries PG_BATCH_GAPPED or PG_BATCH_ALL_MATCHES, not both");
    if (!gapped && !(b->flags & PG_BATCH_ALL_MATCHES)) return pg_fail(h, PG_ERR_INVALID_ARG, "pg_realign_submit: the batch must carry PG_BATCH_ALL_MATCHES (every op a match, as `reform` writes them)");
    const uint64_t n = b->n_reads;
    if (n > 0x7fffffffull) return pg_fail(h, PG_ERR_INVALID_ARG, "pg_realign_submit: batch too large");
    if (!b->sig_off || !b->seq_off || !b->op_off || (n && (!b->query_start || !status || !a || !bb))) return pg_fail(h, PG_ERR_INVALID_ARG, "pg_realign_submit: null array");
    PG_HIP_TRY(h, hipSetDevice(h->device));
    const hipStream_t s = h->s;
    const bool dev = b->location == PG_LOC_DEVICE;
    // the arrays that lay the batch out are looked at on the host: nothing is sized or addressed by an unchecked number
    h->sig_off.resize(n + 1); h->seq_off.resize(n + 1); h->op_off.resize(n + 1); h->qs.resize(n);
    if (dev) {
        const void *must[] = {b->sig_off, b->seq_off, b->op_off, n ? (const void *)b->query_start : nullptr};
        for (const void *q : must)
            if (q && pg_ptr_kind(q, h->device) != PG_PTR_DEVICE) return pg_fail(h, PG_ERR_INVALID_ARG, "pg_realign_submit: PG_LOC_DEVICE arrays must be device memory of device %d", h->device);
        PG_HIP_TRY(h, hipMemcpyAsync(h->sig_off.data(), b->sig_off, (n + 1) * 8, hipMemcpyDeviceToHost, s));
        PG_HIP_TRY(h, hipMemcpyAsync(h->seq_off.data(), b->seq_off, (n + 1) * 8, hipMemcpyDeviceToHost, s));
        PG_HIP_TRY(h, hipMemcpyAsync(h->op_off.data(), b->op_off, (n + 1) * 8, hipMemcpyDeviceToHost, s));
        PG_HIP_TRY(h, hipStreamSynchronize(s));
    } else {
        memcpy(h->sig_off.data(), b->sig_off, (n + 1) * 8); memcpy(h->seq_off.data(), b->seq_off, (n + 1) * 8); memcpy(h->op_off.data(), b->op_off, (n + 1) * 8);
        if (n) memcpy(h->qs.data(), b->query_start, n * 4);
    }
    h->piece_first.resize(n + 1); h->piece_read.clear(); h->part.assign(n, 0); h->ab.assign(2 * n, 0.0);
    for (uint64_t r = 0; r < n; r++) {
        if (h->sig_off[r + 1] < h->sig_off[r] || h->seq_off[r + 1] < h->seq_off[r] || h->op_off[r + 1] < h->op_off[r])
            return pg_fail(h, PG_ERR_INVALID_ARG, "pg_realign_submit: an offset array decreases at read %llu", (unsigned long long)r);
        const uint64_t lb = h->op_off[r + 1] - h->op_off[r];
        if (lb > 0x7fffffffull) return pg_fail(h, PG_ERR_INVALID_ARG, "pg_realign_submit: read %llu has %llu ops (at most 2^31 - 1)", (unsigned long long)r, (unsigned long long)lb);
        if (status[r] == PG_FIT_ST_OK) {
            if (gapped && h->seq_off[r + 1] - h->seq_off[r] > PG_FIT_MAX_SLICE)
                return pg_fail(h, PG_ERR_INVALID_ARG, "pg_realign_submit: read %llu has a reference slice of %llu bases (at most 2^32 - 1)", (unsigned long long)r,
                               (unsigned long long)(h->seq_off[r + 1] - h->seq_off[r]));
            if (!gapped && h->seq_off[r + 1] - h->seq_off[r] < lb)
                return pg_fail(h, PG_ERR_INVALID_ARG, "pg_realign_submit: read %llu has %llu ops and %llu bases (an accepted read has as many bases as ops)", (unsigned long long)r,
                               (unsigned long long)lb, (unsigned long long)(h->seq_off[r + 1] - h->seq_off[r]));
            if (!std::isfinite(a[r]) || !std::isfinite(bb[r]) || !(bb[r] > 0) || !std::isfinite(1.0 / bb[r]))
                return pg_fail(h, PG_ERR_INVALID_ARG, "pg_realign_submit: read %llu has the status ok, but a = %g and b = %g are no fit's", (unsigned long long)r, a[r], bb[r]);
            h->part[r] = 1; h->ab[2 * r] = a[r]; h->ab[2 * r + 1] = 1.0 / bb[r];
        }
        h->piece_first[r] = (uint32_t)h->piece_read.size();
        const uint64_t np = pg_rl_pieces(lb, h->prm.phase);               // every read has pieces: the ops of one that is not refined are copied
        if (h->piece_read.size() + np > 0x7fffffffull) return pg_fail(h, PG_ERR_INVALID_ARG, "pg_realign_submit: batch too large");
        h->piece_read.insert(h->piece_read.end(), np, (uint32_t)r);
    }
    h->piece_first[n] = (uint32_t)h->piece_read.size();
    const size_t n_pieces = h->piece_read.size();
    const uint64_t n_sig = h->sig_off[n], n_seq = h->seq_off[n], n_ops = h->op_off[n];
    if (n_sig - h->sig_off[0] > PG_FIT_BATCH_SAMPLES)
        return pg_fail(h, PG_ERR_UNSUPPORTED, "pg_realign_submit: %llu samples of signal in one batch (at most 2^28: submit fewer reads at a time)", (unsigned long long)(n_sig - h->sig_off[0]));
    if (dev && b->n_ops && b->n_ops != n_ops) return pg_fail(h, PG_ERR_INVALID_ARG, "pg_realign_submit: pg_batch.n_ops is %u, op_off ends at %llu", b->n_ops, (unsigned long long)n_ops);
    if ((n_sig && !b->sig) || (n_seq && !b->seq) || (n_ops && (!b->op_n || !b->op_t))) return pg_fail(h, PG_ERR_INVALID_ARG, "pg_realign_submit: null array");

    RlBatch B{};
    B.n_reads = (uint32_t)n; B.n_pieces = (uint32_t)n_pieces; B.k = h->k; B.m = h->prm.sig_move_offset; B.rna = h->prm.rna ? 1 : 0; B.min_dur = h->prm.min_dur; B.max_dur = h->prm.max_dur;
    B.band = h->prm.band; B.min_len = h->prm.min_len; B.phase = h->prm.phase;
    B.levels = h->d_levels.p;
    auto room = [](size_t bytes) { return bytes + bytes / 4 + 256; };
#define RL_ENSURE(buf, bytes) PG_HIP_TRY(h, (buf).ensure((bytes) ? (bytes) : 1, room(bytes)))
    // (every submit ends behind its last copy: nothing queued earlier still reads the buffers about to be refilled or regrown, unless a
    // submit failed half way)
    if (h->busy) { PG_HIP_TRY(h, hipStreamSynchronize(s)); h->busy = false; }
    const int tgt = h->cur ^ 1;              // the ops go to the array that does not hold the last submit's: the batch's op_n may be that one
    if (dev) {
        const void *must[] = {n_sig ? (const void *)b->sig : nullptr, n_seq ? (const void *)b->seq : nullptr, n_ops ? (const void *)b->op_n : nullptr, n_ops ? (const void *)b->op_t : nullptr};
        for (const void *q : must)
            if (q && pg_ptr_kind(q, h->device) != PG_PTR_DEVICE) return pg_fail(h, PG_ERR_INVALID_ARG, "pg_realign_submit: PG_LOC_DEVICE arrays must be device memory of device %d", h->device);
        if (n_ops && h->d_out[tgt].p && (const void *)b->op_n >= (const void *)h->d_out[tgt].p && (const char *)b->op_n < (const char *)h->d_out[tgt].p + h->d_out[tgt].cap)
            return pg_fail(h, PG_ERR_INVALID_ARG, "pg_realign_submit: op_n is the array of the submit before the last one (a result's op_n is valid until the submit after the next)");
        B.sig = b->sig; B.sig_off = b->sig_off; B.seq = b->seq; B.seq_off = b->seq_off; B.op_n = b->op_n; B.op_t = b->op_t; B.op_off = b->op_off;
        B.qs = b->query_start;
    } else {
        RL_ENSURE(h->d_sig, n_sig * 2); RL_ENSURE(h->d_seq, n_seq); RL_ENSURE(h->d_opn, n_ops * 4); RL_ENSURE(h->d_opt, n_ops);
        RL_ENSURE(h->d_sigoff, (n + 1) * 8); RL_ENSURE(h->d_seqoff, (n + 1) * 8); RL_ENSURE(h->d_opoff, (n + 1) * 8);
        if (n_sig) PG_HIP_TRY(h, hipMemcpyAsync(h->d_sig.p, b->sig, n_sig * 2, hipMemcpyHostToDevice, s));
        if (n_seq) PG_HIP_TRY(h, hipMemcpyAsync(h->d_seq.p, b->seq, n_seq, hipMemcpyHostToDevice, s));
        if (n_ops) {
            PG_HIP_TRY(h, hipMemcpyAsync(h->d_opn.p, b->op_n, n_ops * 4, hipMemcpyHostToDevice, s));
            PG_HIP_TRY(h, hipMemcpyAsync(h->d_opt.p, b->op_t, n_ops, hipMemcpyHostToDevice, s));
        }
        PG_HIP_TRY(h, hipMemcpyAsync(h->d_sigoff.p, h->sig_off.data(), (n + 1) * 8, hipMemcpyHostToDevice, s));
        PG_HIP_TRY(h, hipMemcpyAsync(h->d_seqoff.p, h->seq_off.data(), (n + 1) * 8, hipMemcpyHostToDevice, s));
        PG_HIP_TRY(h, hipMemcpyAsync(h->d_opoff.p, h->op_off.data(), (n + 1) * 8, hipMemcpyHostToDevice, s));
        RL_ENSURE(h->d_qs, n * 4);
        if (n) PG_HIP_TRY(h, hipMemcpyAsync(h->d_qs.p, h->qs.data(), n * 4, hipMemcpyHostToDevice, s));
        B.qs = h->d_qs.p;
        B.sig = h->d_sig.p; B.sig_off = h->d_sigoff.p; B.seq = h->d_seq.p; B.seq_off = h->d_seqoff.p; B.op_n = h->d_opn.p; B.op_t = h->d_opt.p; B.op_off = h->d_opoff.p;
    }
    RL_ENSURE(h->d_pfirst, (n + 1) * 4); RL_ENSURE(h->d_pread, n_pieces * 4); RL_ENSURE(h->d_pstart, n_pieces * 8); RL_ENSURE(h->d_psum, n_pieces * 8);
    if (gapped) { RL_ENSURE(h->d_pcol, n_pieces * 8); RL_ENSURE(h->d_pcsum, n_pieces * 8); }
    RL_ENSURE(h->d_part, n); RL_ENSURE(h->d_ab, n * 16); RL_ENSURE(h->d_out[tgt], n_ops * 4); RL_ENSURE(h->d_pstats, n_pieces * sizeof(RlPiece));
    RL_ENSURE(h->d_reads, n * sizeof(pg_realign_read));
#undef RL_ENSURE
    B.piece_first = h->d_pfirst.p; B.piece_read = h->d_pread.p; B.piece_start = h->d_pstart.p; B.piece_col = h->d_pcol.p; B.part = h->d_part.p; B.ab = h->d_ab.p;
    const uint32_t blocks = (uint32_t)((n_pieces + kWaves - 1) / kWaves);
    (void)hipGetLastError();
    h->reads.assign(n, pg_realign_read{0, 0, 0, 0, 0, 0, 0});
    if (n_pieces) {
        // ---- the spans of the pieces and the look at op_t; every piece's first sample. flag[0]: an op that is no match; flag[1]: the
        // first read that is to be refined and does not lie inside its samples. One copy of both, and the one wait of the submit that is
        // not its end: behind it no kernel indexes the signal of a refused batch.
        uint32_t flag[2] = {0, 0};
        const uint32_t read_blocks = (uint32_t)((n + kWaves - 1) / kWaves);
        h->busy = true;
        PG_HIP_TRY(h, hipMemcpyAsync(h->d_pfirst.p, h->piece_first.data(), (n + 1) * 4, hipMemcpyHostToDevice, s));
        PG_HIP_TRY(h, hipMemcpyAsync(h->d_pread.p, h->piece_read.data(), n_pieces * 4, hipMemcpyHostToDevice, s));
        PG_HIP_TRY(h, hipMemcpyAsync(h->d_part.p, h->part.data(), n, hipMemcpyHostToDevice, s));
        PG_HIP_TRY(h, hipMemcpyAsync(h->d_ab.p, h->ab.data(), n * 16, hipMemcpyHostToDevice, s));
        PG_HIP_TRY(h, hipMemsetAsync(h->d_flag.p, 0, sizeof(uint32_t), s));
        PG_HIP_TRY(h, hipMemsetAsync(h->d_flag.p + 1, 0xff, sizeof(uint32_t), s));
        if (gapped) hipLaunchKernelGGL(k_rl_span<true>, dim3(blocks), dim3(kThreads), 0, s, B, h->d_psum.p, h->d_pcsum.p, h->d_flag.p);
        else hipLaunchKernelGGL(k_rl_span<false>, dim3(blocks), dim3(kThreads), 0, s, B, h->d_psum.p, (uint64_t *)nullptr, h->d_flag.p);
        PG_HIP_TRY(h, hipGetLastError());
        if (gapped) hipLaunchKernelGGL(k_rl_starts<true>, dim3(read_blocks), dim3(kThreads), 0, s, B, h->d_psum.p, h->d_pcsum.p, h->d_pstart.p, h->d_pcol.p, h->d_flag.p);
        else hipLaunchKernelGGL(k_rl_starts<false>, dim3(read_blocks), dim3(kThreads), 0, s, B, h->d_psum.p, (const uint64_t *)nullptr, h->d_pstart.p, (uint64_t *)nullptr, h->d_flag.p);
        PG_HIP_TRY(h, hipGetLastError());
        PG_HIP_TRY(h, hipMemcpyAsync(flag, h->d_flag.p, sizeof flag, hipMemcpyDeviceToHost, s));
        PG_HIP_TRY(h, hipStreamSynchronize(s));
        h->busy = false;
        if (gapped && (flag[0] & 2u)) return pg_fail(h, PG_ERR_INVALID_ARG, "pg_realign_submit: the batch carries PG_BATCH_GAPPED but holds an op code above 2 (0 match, 1 I, 2 D)");
        if (gapped && flag[1] != 0xffffffffu)
            return pg_fail(h, PG_ERR_INVALID_ARG, (flag[1] & 1u) ? "pg_realign_submit: read %llu has the status ok, but its reference slice has not as many bases as its ops have columns (the status of another batch?)"
                                                                 : "pg_realign_submit: read %llu has the status ok, but its ops leave its samples (the status of another batch?)",
                           (unsigned long long)(flag[1] >> 1));
        if (!gapped && flag[0]) return pg_fail(h, PG_ERR_INVALID_ARG, "pg_realign_submit: the batch carries PG_BATCH_ALL_MATCHES but holds an op that is no match (an I, a D or an unknown op)");
        if (flag[1] != 0xffffffffu)
            return pg_fail(h, PG_ERR_INVALID_ARG, "pg_realign_submit: read %llu has the status ok, but its ops leave its samples (the status of another batch?)", (unsigned long long)flag[1]);
        // ---- the alignment, and the reads' records
        h->busy = true;
        PG_HIP_TRY(h, hipEventRecord(h->ev[0], s));
        if (gapped) hipLaunchKernelGGL(k_rl_align<true>, dim3(blocks), dim3(kThreads), 0, s, B, h->d_out[tgt].p, h->d_pstats.p);
        else hipLaunchKernelGGL(k_rl_align<false>, dim3(blocks), dim3(kThreads), 0, s, B, h->d_out[tgt].p, h->d_pstats.p);
        PG_HIP_TRY(h, hipGetLastError());
        PG_HIP_TRY(h, hipEventRecord(h->ev[1], s));
        hipLaunchKernelGGL(k_rl_reads, dim3(read_blocks), dim3(kThreads), 0, s, B, h->d_pstats.p, h->d_reads.p);
        PG_HIP_TRY(h, hipGetLastError());
        PG_HIP_TRY(h, hipMemcpyAsync(h->reads.data(), h->d_reads.p, n * sizeof(pg_realign_read), hipMemcpyDeviceToHost, s));
        PG_HIP_TRY(h, hipStreamSynchronize(s));
        h->busy = false;
        float ms = 0; PG_HIP_TRY(h, hipEventElapsedTime(&ms, h->ev[0], h->ev[1])); h->ms += ms;
    }
    h->cur = tgt;
    out->n_reads = n; out->n_ops = n_ops; out->op_n = h->d_out[tgt].p; out->reads = h->reads.data();
    return PG_OK;
}

pg_status pg_realign_walk(const pg_realign_params *p, const uint32_t *levels, uint32_t k, const uint8_t *seq, uint32_t lb, const uint32_t *op_n, int64_t q, const int16_t *sig,
                          uint64_t n_sig, double a, double b, uint32_t *op_out, pg_realign_read *out) {
    if (!p || !levels || !out || (lb && (!seq || !op_n || !op_out)) || (n_sig && !sig) || k < 1 || k > PG_FIT_MAX_K) return PG_ERR_INVALID_ARG;
    if (p->struct_size != sizeof(pg_realign_params) || !pg_rl_params_ok(p->band, p->min_len, p->min_dur, p->max_dur) || p->sig_move_offset > 64 || p->phase >= PG_FIT_PIECE)
        return PG_ERR_INVALID_ARG;
    PgRlRead r;
    if (!pg_rl_walk_host(seq, lb, op_n, q, sig, n_sig, levels, k, p->sig_move_offset, p->rna != 0, p->min_dur, p->max_dur, p->band, p->min_len, p->phase, a, b, op_out, r))
        return PG_ERR_INPUT;
    *out = pg_realign_read{r.n_free, r.n_moved, r.sum_abs_shift, (uint64_t)r.cost_before, (uint64_t)(r.cost_before >> 64), (uint64_t)r.cost_after, (uint64_t)(r.cost_after >> 64)};
    return PG_OK;
}

pg_status pg_realign_walk_gapped(const pg_realign_params *p, const uint32_t *levels, uint32_t k, const uint8_t *seq, uint64_t n_seq, const uint32_t *op_n, const uint8_t *op_t,
                                 uint32_t lb, int64_t q, const int16_t *sig, uint64_t n_sig, double a, double b, uint32_t *op_out, pg_realign_read *out) {
    if (!p || !levels || !out || (lb && (!op_n || !op_t || !op_out)) || (n_seq && !seq) || (n_sig && !sig) || k < 1 || k > PG_FIT_MAX_K) return PG_ERR_INVALID_ARG;
    if (p->struct_size != sizeof(pg_realign_params) || !pg_rl_params_ok(p->band, p->min_len, p->min_dur, p->max_dur) || p->sig_move_offset > 64 || p->phase >= PG_FIT_PIECE)
        return PG_ERR_INVALID_ARG;
    for (uint32_t e = 0; e < lb; e++)
        if (op_t[e] > PG_FIT_OP_D) return PG_ERR_INVALID_ARG;
    if (n_seq > PG_FIT_MAX_SLICE) return PG_ERR_INVALID_ARG;
    static const uint8_t none = 0;
    PgRlRead r;
    if (!pg_rl_walk_any(seq, n_seq, lb ? op_t : &none, lb, op_n, q, sig, n_sig, levels, k, p->sig_move_offset, p->rna != 0, p->min_dur, p->max_dur, p->band, p->min_len, p->phase, a, b, op_out, r))
        return PG_ERR_INPUT;
    *out = pg_realign_read{r.n_free, r.n_moved, r.sum_abs_shift, (uint64_t)r.cost_before, (uint64_t)(r.cost_before >> 64), (uint64_t)r.cost_after, (uint64_t)(r.cost_after >> 64)};
    return PG_OK;
}

} // extern "C"
