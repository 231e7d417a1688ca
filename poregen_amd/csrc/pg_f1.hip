// pg_f1.hip -- `poregen f1_score` on the device: per-signal-point agreement of two ss signal alignments (the reference's
// src/f1_score/f1score.py), counted in O(ss bytes) instead of O(signal points).
//
// A batch holds the ss strings of n pairs, string 2p = side 1 (file 1) and 2p+1 = side 2 of pair p, concatenated, with per-string
// scalars: the first signal index (si[0]) and the first reference position (si[2], side 2 already shifted by --base_shift).
// The rules restated on the bytes (host/f1_cli.cpp cites the reference's lines):
//   * an op ends at a non-digit byte preceded by a digit of the same string; its count is that digit run. ',' maps `count` points
//     to the current ref and then steps the ref by dir; 'I' maps `count` points to -1; 'D' steps the ref by dir * count; any other
//     byte maps nothing. Signal points run contiguously from si[0].
//   * only the overlap of the two contiguous signal ranges is compared. A point with refs (r1, r2) is skipped under a region when
//     START > r1 + 1 or END < r1 + 1; otherwise it is TN if both are -1, FP if only r1 is, FN if only r2 is, and then ALSO TP if
//     |r1 - r2| <= threshold, else FP.
//
// Every point of one op has the same ref, so the merged list of op boundaries of the two sides cuts the overlap into intervals on
// which (r1, r2) is constant: each is classified once, in closed form, and weighted by its length.
//
// Work is cut into pieces of whole pairs of at most kUnit bytes (a host batch is staged piece by piece; a device batch is read in
// place). Per piece:
//   k_f1_tiles   : per tile of kTile bytes, the number of ops and the sums of their points and ref steps (reads the bytes once)
//   k_f1_scan    : exclusive scan of the tile sums (one workgroup); the prefix at the piece end for the strings that start there
//   k_f1_emit    : per op its exclusive prefix of points and ref steps (global over the piece) and its kind; per string the
//                  prefix at its first byte. Per-string values are differences of these (u64 arithmetic, exact modulo 2^64)
//   k_f1_strings : empty ss / ss ending in a digit
//   k_f1_chunks  : per pair the number of workgroups its merge takes (kChunk merge steps each), then scanned (k_f1_scan_u64)
//   k_f1_merge   : one workgroup per chunk of kChunk steps of a pair's merge: a merge-path partition of the two op lists clamped to
//                  the overlap window, every thread classifies its intervals; u64[4] per pair (TP, FP, TN, FN), integer adds only.
// Refusals (PG_ERR_INPUT with the pair): an op count >= 2^32, a byte >= 0x80 in ss, an empty ss, an ss ending in a digit, a side
// that maps no point. Reference positions are carried in 128-bit integers, so no input value can overflow them.
#include "../../include/pgmove.h"
#include <hip/hip_runtime.h>
#include "pg_hip_host.h"

#include <algorithm>
#include <cstring>
#include <string>
#include <vector>

namespace {

constexpr int kThreads = 256;
constexpr int kSpan = 16;                                // bytes per thread
constexpr uint64_t kTile = (uint64_t)kThreads * kSpan;   // 4 KiB per workgroup
constexpr uint64_t kUnit = 32ull << 20;                  // bytes per piece (a single larger pair makes a piece of its own)
constexpr uint32_t kUnitPairs = 1u << 20;                // pairs per piece
constexpr int kMergeItems = 8;                           // merge steps per thread
constexpr uint64_t kChunk = (uint64_t)kThreads * kMergeItems; // merge steps per workgroup: a long pair spreads over many workgroups

enum : uint32_t { kOpOther = 0, kOpMatch = 1, kOpIns = 2, kOpDel = 3 };
// error codes (low bits of the error word; ordered as the reference meets them within a pair)
enum : uint32_t { kErrEmpty = 1, kErrEndsDigit = 2, kErrNonAscii = 3, kErrCount = 4, kErrNoPoints = 5 };
constexpr unsigned long long kNoErr = ~0ull;

__device__ __forceinline__ bool is_digit(uint32_t c) { return c - '0' < 10u; }

__device__ __forceinline__ void flag_error(unsigned long long *err, uint64_t string, uint32_t code) {
    if (!err) return;
    // pair-major, then code, then side: the smallest word is the failure the reference raises first
    atomicMin(err, (unsigned long long)((string >> 1) << 8 | code << 1 | (string & 1)));
}

// the string holding byte g: the last s with off[s] <= g (empty strings share their offset with the next one)
__device__ __forceinline__ uint32_t string_of(const uint64_t *__restrict__ off, uint32_t ns, uint64_t g) {
    uint32_t lo = 0, hi = ns; // answer in [0, ns)
    while (hi - lo > 1) { const uint32_t mid = (lo + hi) >> 1; if (off[mid] <= g) lo = mid; else hi = mid; }
    return lo;
}

struct OpSums { unsigned long long ops, pts, steps; };

// Walks this thread's kSpan bytes [base, base + kSpan) of the piece, calls f(g, kind, count, s) for every op that ends there,
// in byte order, and flags the byte errors when err is set. The digit run an op ends may start in earlier threads' bytes: it is
// read back from global memory.
template <class F>
__device__ __forceinline__ void walk_span(const uint8_t *__restrict__ p, uint64_t n, const uint64_t *__restrict__ off, uint32_t ns,
                                          uint64_t base, unsigned long long *err, F &&f) {
    if (base >= n) return;
    uint32_t w[kSpan / 4]; // the span's bytes in registers (indexed with constants only: no scratch)
    if (((uintptr_t)(p + base) & 15) == 0 && base + kSpan <= n) {
        const uint4 v = *reinterpret_cast<const uint4 *>(p + base);
        w[0] = v.x; w[1] = v.y; w[2] = v.z; w[3] = v.w;
    } else {
#pragma unroll
        for (int i = 0; i < kSpan / 4; i++) {
            uint32_t x = 0;
            for (int k = 0; k < 4; k++) if (base + 4 * i + k < n) x |= (uint32_t)p[base + 4 * i + k] << (8 * k);
            w[i] = x;
        }
    }
    uint32_t s = string_of(off, ns, base);
    uint64_t s_begin = off[s], s_end = off[s + 1];
    // digits of the run open at base
    unsigned long long v = 0;
    bool has = false;
    if (base > s_begin && is_digit(p[base - 1])) {
        uint64_t j = base - 1;
        while (j > s_begin && is_digit(p[j - 1])) j--;
        for (; j < base; j++) v = min(v * 10 + (p[j] - '0'), 1ull << 32);
        has = true;
    }
    const uint64_t end = min(base + kSpan, n);
    for (int i = 0; i < kSpan; i++) {
        const uint64_t g = base + i;
        if (g >= end) break;
        while (g >= s_end) { // next non-empty string: a fresh digit run
            s++; s_begin = s_end; s_end = off[s + 1];
            v = 0; has = false;
        }
        const uint32_t word = i < 8 ? (i < 4 ? w[0] : w[1]) : (i < 12 ? w[2] : w[3]); // selects, not an indexed (scratch) array
        const uint32_t c = (word >> (8 * (i & 3))) & 0xffu;
        if (c >= 0x80u) flag_error(err, s, kErrNonAscii);
        if (is_digit(c)) { v = min(v * 10 + (c - '0'), 1ull << 32); has = true; continue; }
        if (!has) continue;
        if (v >> 32) flag_error(err, s, kErrCount);
        const uint32_t kind = c == ',' ? kOpMatch : c == 'I' ? kOpIns : c == 'D' ? kOpDel : kOpOther;
        f(g, kind, v, s);
        v = 0; has = false;
    }
}

__device__ __forceinline__ void op_add(OpSums &a, uint32_t kind, unsigned long long v) {
    // values selected, not addresses: a selected address puts `a` in scratch
    a.ops += 1;
    a.pts += (kind == kOpMatch || kind == kOpIns) ? v : 0ull;
    a.steps += kind == kOpMatch ? 1ull : kind == kOpDel ? v : 0ull;
}

template <class T>
__device__ __forceinline__ T wave_sum(T x) {
    for (int o = 32; o > 0; o >>= 1) x += __shfl_xor(x, o);
    return x;
}
template <class T>
__device__ __forceinline__ T wave_incl_scan(T x) {
    const int lane = threadIdx.x & 63;
    for (int o = 1; o < 64; o <<= 1) { const T y = __shfl_up(x, o); if (lane >= o) x += y; }
    return x;
}

__global__ __launch_bounds__(kThreads) void k_f1_tiles(const uint8_t *__restrict__ p, uint64_t n, const uint64_t *__restrict__ off,
                                                       uint32_t ns, unsigned long long *__restrict__ t_ops, unsigned long long *__restrict__ t_pts,
                                                       unsigned long long *__restrict__ t_steps, unsigned long long *err) {
    OpSums a{0, 0, 0};
    walk_span(p, n, off, ns, blockIdx.x * kTile + threadIdx.x * (uint64_t)kSpan, err,
              [&](uint64_t, uint32_t kind, unsigned long long v, uint32_t) { op_add(a, kind, v); });
    __shared__ unsigned long long r_ops[kThreads / 64], r_pts[kThreads / 64], r_steps[kThreads / 64];
    a.ops = wave_sum(a.ops); a.pts = wave_sum(a.pts); a.steps = wave_sum(a.steps);
    if ((threadIdx.x & 63) == 0) { r_ops[threadIdx.x >> 6] = a.ops; r_pts[threadIdx.x >> 6] = a.pts; r_steps[threadIdx.x >> 6] = a.steps; }
    __syncthreads();
    if (threadIdx.x == 0) {
        OpSums t{0, 0, 0};
        for (int w = 0; w < kThreads / 64; w++) { t.ops += r_ops[w]; t.pts += r_pts[w]; t.steps += r_steps[w]; }
        t_ops[blockIdx.x] = t.ops; t_pts[blockIdx.x] = t.pts; t_steps[blockIdx.x] = t.steps;
    }
}

struct StrBase { unsigned long long op, pts, steps; }; // exclusive prefixes at a string's first byte

// exclusive scan of the tile sums in place (one workgroup of 1024), then the strings that start at the piece end
__global__ __launch_bounds__(1024) void k_f1_scan(uint32_t n_tiles, unsigned long long *__restrict__ t_ops, unsigned long long *__restrict__ t_pts,
                                                  unsigned long long *__restrict__ t_steps, const uint64_t *__restrict__ off, uint32_t ns,
                                                  StrBase *__restrict__ sb) {
    __shared__ unsigned long long w_ops[16], w_pts[16], w_steps[16];
    __shared__ unsigned long long carry[3];
    if (threadIdx.x == 0) carry[0] = carry[1] = carry[2] = 0;
    __syncthreads();
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    for (uint32_t b0 = 0; b0 < n_tiles; b0 += 1024) {
        const uint32_t i = b0 + threadIdx.x;
        const unsigned long long o = i < n_tiles ? t_ops[i] : 0, pt = i < n_tiles ? t_pts[i] : 0, st = i < n_tiles ? t_steps[i] : 0;
        const unsigned long long io = wave_incl_scan(o), ip = wave_incl_scan(pt), is = wave_incl_scan(st);
        if (lane == 63) { w_ops[wave] = io; w_pts[wave] = ip; w_steps[wave] = is; }
        __syncthreads();
        unsigned long long bo = carry[0], bp = carry[1], bs = carry[2];
        for (int w = 0; w < wave; w++) { bo += w_ops[w]; bp += w_pts[w]; bs += w_steps[w]; }
        if (i < n_tiles) { t_ops[i] = bo + io - o; t_pts[i] = bp + ip - pt; t_steps[i] = bs + is - st; }
        __syncthreads();
        if (threadIdx.x == 1023) { carry[0] = bo + io; carry[1] = bp + ip; carry[2] = bs + is; }
        __syncthreads();
    }
    if (threadIdx.x == 0) { // strings at the piece end (the sentinel ns included): the totals
        const uint64_t n = off[ns];
        for (int64_t s = ns; s >= 0 && off[s] == n; s--) sb[s] = StrBase{carry[0], carry[1], carry[2]};
    }
}

__global__ __launch_bounds__(kThreads) void k_f1_emit(const uint8_t *__restrict__ p, uint64_t n, const uint64_t *__restrict__ off, uint32_t ns,
                                                      const unsigned long long *__restrict__ t_ops, const unsigned long long *__restrict__ t_pts,
                                                      const unsigned long long *__restrict__ t_steps, unsigned long long *__restrict__ op_pts,
                                                      unsigned long long *__restrict__ op_steps, uint8_t *__restrict__ op_kind,
                                                      StrBase *__restrict__ sb, unsigned long long *err) {
    const uint64_t base = blockIdx.x * kTile + threadIdx.x * (uint64_t)kSpan;
    OpSums a{0, 0, 0}; // byte errors were flagged by k_f1_tiles
    walk_span(p, n, off, ns, base, nullptr, [&](uint64_t, uint32_t kind, unsigned long long v, uint32_t) { op_add(a, kind, v); });
    // exclusive prefix of this thread within the piece
    __shared__ unsigned long long w_ops[kThreads / 64], w_pts[kThreads / 64], w_steps[kThreads / 64];
    const unsigned long long io = wave_incl_scan(a.ops), ip = wave_incl_scan(a.pts), is = wave_incl_scan(a.steps);
    const int wave = threadIdx.x >> 6;
    if ((threadIdx.x & 63) == 63) { w_ops[wave] = io; w_pts[wave] = ip; w_steps[wave] = is; }
    __syncthreads();
    unsigned long long c_op = t_ops[blockIdx.x] + io - a.ops, c_pts = t_pts[blockIdx.x] + ip - a.pts, c_steps = t_steps[blockIdx.x] + is - a.steps;
    for (int w = 0; w < wave; w++) { c_op += w_ops[w]; c_pts += w_pts[w]; c_steps += w_steps[w]; }
    if (base >= n) return;
    // strings that start in this span get the prefix at their first byte; ops get theirs
    uint32_t t_next = 0, hi = ns; // the first string starting at or after base: lower bound in [0, ns]
    while (t_next < hi) { const uint32_t mid = (t_next + hi) >> 1; if (off[mid] < base) t_next = mid + 1; else hi = mid; }
    const uint64_t end = min(base + kSpan, n);
    auto starts_upto = [&](uint64_t g_last) { // the bases of the strings that start at or before byte g_last of this span
        for (; t_next < ns && off[t_next] <= g_last; t_next++) sb[t_next] = StrBase{c_op, c_pts, c_steps};
    };
    walk_span(p, n, off, ns, base, nullptr, [&](uint64_t g, uint32_t kind, unsigned long long v, uint32_t) {
        starts_upto(g); // the op at g belongs to a string that started before g: its prefix comes after
        op_pts[c_op] = c_pts; op_steps[c_op] = c_steps; op_kind[c_op] = (uint8_t)kind;
        OpSums d{0, 0, 0}; op_add(d, kind, v);
        c_op += 1; c_pts += d.pts; c_steps += d.steps;
    });
    starts_upto(end - 1);
}

__global__ void k_f1_strings(const uint8_t *__restrict__ p, const uint64_t *__restrict__ off, uint32_t ns, unsigned long long *err) {
    const uint32_t s = blockIdx.x * blockDim.x + threadIdx.x;
    if (s >= ns) return;
    const uint64_t a = off[s], b = off[s + 1];
    if (a == b) flag_error(err, s, kErrEmpty);
    else if (is_digit(p[b - 1])) flag_error(err, s, kErrEndsDigit);
}

struct F1Params { int32_t dir, use_region; long long threshold, region_start, region_end; };

// the ref of an op that bears points: -1 for 'I', else first + dir * (ref steps before it)
__device__ __forceinline__ __int128 op_ref(uint8_t kind, unsigned long long steps, long long first, int32_t dir) {
    if (kind == kOpIns) return -1;
    return dir > 0 ? (__int128)first + (__int128)steps : (__int128)first - (__int128)steps;
}

// workgroups of pair p's merge: one per kChunk merge steps, at least one (it also checks the pair)
__global__ void k_f1_chunks(const StrBase *__restrict__ sb, uint32_t np, unsigned long long *__restrict__ chunk_off) {
    const uint32_t p = blockIdx.x * blockDim.x + threadIdx.x;
    if (p >= np) return;
    const uint64_t total = sb[2 * p + 2].op - sb[2 * p].op;
    chunk_off[p] = total > kChunk ? (total + kChunk - 1) / kChunk : 1;
}

// exclusive scan of a[0, n) in place, a[n] = the total (one workgroup of 1024)
__global__ __launch_bounds__(1024) void k_f1_scan_u64(uint32_t n, unsigned long long *__restrict__ a) {
    __shared__ unsigned long long w_sum[16];
    __shared__ unsigned long long carry;
    if (threadIdx.x == 0) carry = 0;
    __syncthreads();
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    for (uint32_t b0 = 0; b0 < n; b0 += 1024) {
        const uint32_t i = b0 + threadIdx.x;
        const unsigned long long x = i < n ? a[i] : 0, incl = wave_incl_scan(x);
        if (lane == 63) w_sum[wave] = incl;
        __syncthreads();
        unsigned long long base = carry;
        for (int w = 0; w < wave; w++) base += w_sum[w];
        if (i < n) a[i] = base + incl - x;
        __syncthreads();
        if (threadIdx.x == 1023) carry = base + incl;
        __syncthreads();
    }
    if (threadIdx.x == 0) a[n] = carry;
}

__global__ __launch_bounds__(kThreads) void k_f1_merge(const unsigned long long *__restrict__ op_pts, const unsigned long long *__restrict__ op_steps,
                                                       const uint8_t *__restrict__ op_kind, const StrBase *__restrict__ sb,
                                                       const long long *__restrict__ sig_start, const long long *__restrict__ first_ref,
                                                       const unsigned long long *__restrict__ chunk_off, uint32_t np, F1Params prm,
                                                       unsigned long long *__restrict__ pair_counts, unsigned long long *err) {
    // the grid is an upper bound of the chunks; this workgroup's pair: the last p with chunk_off[p] <= blockIdx.x
    if (blockIdx.x >= chunk_off[np]) return;
    uint32_t pr = 0;
    for (uint32_t hi = np; hi - pr > 1;) { const uint32_t mid = (pr + hi) >> 1; if (chunk_off[mid] <= blockIdx.x) pr = mid; else hi = mid; }
    const uint64_t chunk = blockIdx.x - chunk_off[pr];
    const uint32_t sA = 2 * pr, sB = 2 * pr + 1;
    const StrBase a0 = sb[sA], a1 = sb[sA + 1], b1 = sb[sB + 1];
    const StrBase &b0 = a1;
    const unsigned long long PA = a1.pts - a0.pts, PB = b1.pts - b0.pts;
    const uint64_t nA = a1.op - a0.op, nB = b1.op - b0.op;
    unsigned long long tp = 0, fp = 0, tn = 0, fn = 0;
    if (PA == 0 || PB == 0) {
        if (threadIdx.x == 0 && chunk == 0) flag_error(err, PA == 0 ? sA : sB, kErrNoPoints);
    } else {
        const __int128 sa = sig_start[sA], sbg = sig_start[sB];
        const __int128 lo = sa > sbg ? sa : sbg, ea = sa + (__int128)PA, eb = sbg + (__int128)PB, hi = ea < eb ? ea : eb;
        if (hi > lo) {
            const unsigned long long L = (unsigned long long)(hi - lo), offA = (unsigned long long)(lo - sa), offB = (unsigned long long)(lo - sbg);
            // boundary of op i of a side in window coordinates, clamped into [0, L]
            auto bA = [&](uint64_t i) -> unsigned long long {
                const unsigned long long x = op_pts[a0.op + i] - a0.pts;
                return x <= offA ? 0 : min(x - offA, L);
            };
            auto bB = [&](uint64_t i) -> unsigned long long {
                const unsigned long long x = op_pts[b0.op + i] - b0.pts;
                return x <= offB ? 0 : min(x - offB, L);
            };
            const long long fA = first_ref[sA], fB = first_ref[sB];
            const uint64_t total = nA + nB;
            const uint64_t d0 = chunk * kChunk + (uint64_t)threadIdx.x * kMergeItems;
            if (d0 < total) {
                // merge path: i items of A among the first d0 merged (A first on ties)
                uint64_t lo_i = d0 > nB ? d0 - nB : 0, hi_i = min<uint64_t>(d0, nA);
                while (lo_i < hi_i) {
                    const uint64_t mid = (lo_i + hi_i) >> 1;
                    if (bA(mid) <= bB(d0 - 1 - mid)) lo_i = mid + 1; else hi_i = mid;
                }
                uint64_t i = lo_i, j = d0 - lo_i;
                unsigned long long nextA = i < nA ? bA(i) : L, nextB = j < nB ? bB(j) : L;
                const uint64_t d1 = min<uint64_t>(d0 + kMergeItems, total);
                for (uint64_t d = d0; d < d1; d++) {
                    unsigned long long pos;
                    if (i < nA && (j >= nB || nextA <= nextB)) { pos = nextA; i++; nextA = i < nA ? bA(i) : L; }
                    else { pos = nextB; j++; nextB = j < nB ? bB(j) : L; }
                    const unsigned long long nxt = min(nextA, nextB);
                    if (nxt <= pos || i == 0 || j == 0) continue; // empty interval (before both sides started, or a tie)
                    const unsigned long long len = nxt - pos;
                    const __int128 r1 = op_ref(op_kind[a0.op + i - 1], op_steps[a0.op + i - 1] - a0.steps, fA, prm.dir);
                    const __int128 r2 = op_ref(op_kind[b0.op + j - 1], op_steps[b0.op + j - 1] - b0.steps, fB, prm.dir);
                    if (prm.use_region && ((__int128)prm.region_start > r1 + 1 || (__int128)prm.region_end < r1 + 1)) continue;
                    if (r1 == -1 && r2 == -1) tn += len;
                    else if (r1 == -1) fp += len;
                    else if (r2 == -1) fn += len;
                    const __int128 diff = r1 > r2 ? r1 - r2 : r2 - r1;
                    if (diff <= (__int128)prm.threshold) tp += len; else fp += len;
                }
            }
        }
    }
    __shared__ unsigned long long red[4][kThreads / 64];
    tp = wave_sum(tp); fp = wave_sum(fp); tn = wave_sum(tn); fn = wave_sum(fn);
    if ((threadIdx.x & 63) == 0) { red[0][threadIdx.x >> 6] = tp; red[1][threadIdx.x >> 6] = fp; red[2][threadIdx.x >> 6] = tn; red[3][threadIdx.x >> 6] = fn; }
    __syncthreads();
    if (threadIdx.x < 4) {
        unsigned long long t = 0;
        for (int w = 0; w < kThreads / 64; w++) t += red[threadIdx.x][w];
        if (t) atomicAdd(&pair_counts[4 * (uint64_t)pr + threadIdx.x], t); // integer adds: the order does not matter
    }
}

struct Slot { // one piece in flight: its device inputs (host batches), its results and the event that says they are back
    PgEvent done;
    PgDev<uint8_t> dbytes;
    PgPinned<uint8_t> stage; // copy of the bytes (pageable host input)
    PgDev<uint64_t> doff; PgDev<long long> dsig, dref;
    PgPinned<uint64_t> hoff; PgPinned<long long> hsig, href;
    PgDev<unsigned long long> dcounts, derr;
    PgPinned<unsigned long long> hcounts, herr;
    bool busy = false;
    uint64_t first_pair = 0, n_pairs = 0;
};

} // namespace

struct pg_fscore {
    int device = 0;
    F1Params prm{};
    PgStream st;
    Slot slot[2];
    int next = 0;
    // per-piece work space
    PgDev<unsigned long long> t_ops, t_pts, t_steps;
    PgDev<unsigned long long> op_pts, op_steps; PgDev<uint8_t> op_kind;
    PgDev<StrBase> sb;
    PgDev<unsigned long long> chunk_off;
    // results since the last finish
    uint64_t n_pairs = 0;
    std::vector<unsigned long long> counts; // 4 per pair
    uint64_t err_word = kNoErr, err_first_pair = 0; // first device error: err_first_pair + (word >> 8)
    std::string err;
};

// wait for a slot's piece and fold its results in
static pg_status f1_drain(pg_fscore *h, Slot &sl) {
    if (!sl.busy) return PG_OK;
    PG_HIP_TRY(h, hipEventSynchronize(sl.done));
    sl.busy = false;
    memcpy(h->counts.data() + 4 * sl.first_pair, sl.hcounts.p, 4 * sl.n_pairs * sizeof(unsigned long long));
    if (*sl.herr.p != kNoErr && h->err_word == kNoErr) { h->err_word = *sl.herr.p; h->err_first_pair = sl.first_pair; }
    return PG_OK;
}

// one piece: strings [s0, s0 + ns) of the caller's batch (ns even), bytes [off[s0], off[s0 + ns]) at `bytes` (device memory when dev)
static pg_status f1_piece(pg_fscore *h, const uint8_t *bytes, bool dev, bool pinned, const uint64_t *off, const int64_t *sig,
                          const int64_t *ref, uint64_t s0, uint32_t ns) {
    Slot &sl = h->slot[h->next]; h->next ^= 1;
    if (pg_status s = f1_drain(h, sl)) return s;
    const uint64_t b0 = off[s0], n = off[s0 + ns] - b0;
    const uint32_t np = ns / 2;
    // inputs: offsets rebased to the piece, scalars (pinned, then one copy each)
    const uint64_t strs = (uint64_t)ns + 1;
    PG_HIP_TRY(h, sl.hoff.ensure(strs * 8)); PG_HIP_TRY(h, sl.hsig.ensure(strs * 8)); PG_HIP_TRY(h, sl.href.ensure(strs * 8));
    PG_HIP_TRY(h, sl.doff.ensure(strs * 8)); PG_HIP_TRY(h, sl.dsig.ensure(strs * 8)); PG_HIP_TRY(h, sl.dref.ensure(strs * 8));
    PG_HIP_TRY(h, sl.hcounts.ensure(4ull * np * 8)); PG_HIP_TRY(h, sl.dcounts.ensure(4ull * np * 8));
    for (uint32_t i = 0; i <= ns; i++) sl.hoff.p[i] = off[s0 + i] - b0;
    memcpy(sl.hsig.p, sig + s0, ns * sizeof(int64_t));
    memcpy(sl.href.p, ref + s0, ns * sizeof(int64_t));
    *sl.herr.p = kNoErr;
    PG_HIP_TRY(h, hipMemcpyAsync(sl.doff.p, sl.hoff.p, strs * sizeof(uint64_t), hipMemcpyHostToDevice, h->st));
    PG_HIP_TRY(h, hipMemcpyAsync(sl.dsig.p, sl.hsig.p, ns * sizeof(int64_t), hipMemcpyHostToDevice, h->st));
    PG_HIP_TRY(h, hipMemcpyAsync(sl.dref.p, sl.href.p, ns * sizeof(int64_t), hipMemcpyHostToDevice, h->st));
    PG_HIP_TRY(h, hipMemcpyAsync(sl.derr.p, sl.herr.p, sizeof(unsigned long long), hipMemcpyHostToDevice, h->st));
    const uint8_t *p = bytes + b0;
    if (!dev && n) {
        PG_HIP_TRY(h, sl.dbytes.ensure(n));
        const uint8_t *from = p;
        if (!pinned) {
            PG_HIP_TRY(h, sl.stage.ensure(n));
            memcpy(sl.stage.p, p, n);
            from = sl.stage.p;
        }
        PG_HIP_TRY(h, hipMemcpyAsync(sl.dbytes.p, from, n, hipMemcpyHostToDevice, h->st));
        p = sl.dbytes.p;
    }
    // work space
    const uint64_t n_tiles = (n + kTile - 1) / kTile;
    if (n_tiles * 8 > h->t_ops.cap) {
        PG_HIP_TRY(h, hipStreamSynchronize(h->st)); // the other slot's piece may still use the old buffers
        PG_HIP_TRY(h, h->t_ops.ensure(n_tiles * 8)); PG_HIP_TRY(h, h->t_pts.ensure(n_tiles * 8)); PG_HIP_TRY(h, h->t_steps.ensure(n_tiles * 8));
    }
    const uint64_t max_ops = n / 2 + 1; // an op takes a digit and its terminator
    if (max_ops * 8 > h->op_pts.cap) {
        PG_HIP_TRY(h, hipStreamSynchronize(h->st));
        PG_HIP_TRY(h, h->op_pts.ensure(max_ops * 8)); PG_HIP_TRY(h, h->op_steps.ensure(max_ops * 8)); PG_HIP_TRY(h, h->op_kind.ensure(max_ops));
    }
    if (strs * sizeof(StrBase) > h->sb.cap) { PG_HIP_TRY(h, hipStreamSynchronize(h->st)); PG_HIP_TRY(h, h->sb.ensure(strs * sizeof(StrBase))); }
    if ((np + 1ull) * 8 > h->chunk_off.cap) { PG_HIP_TRY(h, hipStreamSynchronize(h->st)); PG_HIP_TRY(h, h->chunk_off.ensure((np + 1ull) * 8)); }
    if (n_tiles) {
        hipLaunchKernelGGL(k_f1_tiles, dim3((uint32_t)n_tiles), dim3(kThreads), 0, h->st, p, n, sl.doff.p, ns, h->t_ops.p, h->t_pts.p, h->t_steps.p, sl.derr.p);
        PG_HIP_TRY(h, hipGetLastError());
    }
    hipLaunchKernelGGL(k_f1_scan, dim3(1), dim3(1024), 0, h->st, (uint32_t)n_tiles, h->t_ops.p, h->t_pts.p, h->t_steps.p, sl.doff.p, ns, h->sb.p);
    PG_HIP_TRY(h, hipGetLastError());
    if (n_tiles) {
        hipLaunchKernelGGL(k_f1_emit, dim3((uint32_t)n_tiles), dim3(kThreads), 0, h->st, p, n, sl.doff.p, ns, h->t_ops.p, h->t_pts.p, h->t_steps.p,
                           h->op_pts.p, h->op_steps.p, h->op_kind.p, h->sb.p, sl.derr.p);
        PG_HIP_TRY(h, hipGetLastError());
    }
    hipLaunchKernelGGL(k_f1_strings, dim3((ns + 255) / 256), dim3(256), 0, h->st, p, sl.doff.p, ns, sl.derr.p);
    PG_HIP_TRY(h, hipGetLastError());
    hipLaunchKernelGGL(k_f1_chunks, dim3((np + 255) / 256), dim3(256), 0, h->st, h->sb.p, np, h->chunk_off.p);
    PG_HIP_TRY(h, hipGetLastError());
    hipLaunchKernelGGL(k_f1_scan_u64, dim3(1), dim3(1024), 0, h->st, np, h->chunk_off.p);
    PG_HIP_TRY(h, hipGetLastError());
    PG_HIP_TRY(h, hipMemsetAsync(sl.dcounts.p, 0, 4ull * np * sizeof(unsigned long long), h->st));
    // chunks <= sum over pairs of (ops / kChunk + 1) <= max_ops / kChunk + np
    const uint64_t grid = max_ops / kChunk + np + 1;
    hipLaunchKernelGGL(k_f1_merge, dim3((uint32_t)grid), dim3(kThreads), 0, h->st, h->op_pts.p, h->op_steps.p, h->op_kind.p, h->sb.p, sl.dsig.p, sl.dref.p,
                       h->chunk_off.p, np, h->prm, sl.dcounts.p, sl.derr.p);
    PG_HIP_TRY(h, hipGetLastError());
    PG_HIP_TRY(h, hipMemcpyAsync(sl.hcounts.p, sl.dcounts.p, 4ull * np * sizeof(unsigned long long), hipMemcpyDeviceToHost, h->st));
    PG_HIP_TRY(h, hipMemcpyAsync(sl.herr.p, sl.derr.p, sizeof(unsigned long long), hipMemcpyDeviceToHost, h->st));
    PG_HIP_TRY(h, hipEventRecord(sl.done, h->st));
    sl.busy = true; sl.first_pair = h->n_pairs; sl.n_pairs = np;
    h->n_pairs += np;
    return PG_OK;
}

extern "C" {

const char *pg_fscore_last_error(const pg_fscore *h) { return h ? h->err.c_str() : pg_create_error<pg_fscore>().c_str(); }

pg_status pg_fscore_create(const pg_fscore_params *params, int32_t device, pg_fscore **out) {
    if (!out || !params) return pg_fail<pg_fscore>(nullptr, PG_ERR_INVALID_ARG, "pg_fscore_create: null argument");
    *out = nullptr;
    if (pg_status st = pg_select_device<pg_fscore>(device)) return st;
    pg_fscore *h = new pg_fscore();
    h->device = device;
    h->prm = F1Params{params->rna ? -1 : 1, params->use_region ? 1 : 0, (long long)params->threshold, (long long)params->region_start,
                      (long long)params->region_end};
    auto init = [&]() -> pg_status {
        PG_HIP_TRY(h, hipStreamCreateWithFlags(&h->st.h, hipStreamNonBlocking));
        for (Slot &sl : h->slot) {
            PG_HIP_TRY(h, hipEventCreateWithFlags(&sl.done.h, hipEventDisableTiming));
            PG_HIP_TRY(h, sl.derr.ensure(sizeof(unsigned long long)));
            PG_HIP_TRY(h, sl.herr.ensure(sizeof(unsigned long long)));
        }
        return PG_OK;
    };
    if (pg_status st = init()) return pg_create_failed(h, st, pg_fscore_destroy);
    *out = h;
    return PG_OK;
}

void pg_fscore_destroy(pg_fscore *h) {
    if (!h) return;
    (void)hipSetDevice(h->device);
    if (h->st) (void)hipStreamSynchronize(h->st);
    delete h;
}

pg_status pg_fscore_submit(pg_fscore *h, const pg_fscore_batch *b) {
    if (!h) return pg_fail<pg_fscore>(nullptr, PG_ERR_INVALID_ARG, "pg_fscore_submit: null handle");
    if (!b) return pg_fail(h, PG_ERR_INVALID_ARG, "pg_fscore_submit: null batch");
    if (!b->n_pairs) return PG_OK;
    if (!b->ss_off || !b->sig_start || !b->first_ref) return pg_fail(h, PG_ERR_INVALID_ARG, "pg_fscore_submit: null array");
    if (b->location != PG_LOC_HOST && b->location != PG_LOC_DEVICE) return pg_fail(h, PG_ERR_INVALID_ARG, "pg_fscore_submit: location must be PG_LOC_HOST or PG_LOC_DEVICE");
    PG_HIP_TRY(h, hipSetDevice(h->device));
    const uint64_t ns = 2 * b->n_pairs;
    const uint64_t *off = b->ss_off;
    for (uint64_t s = 0; s < ns; s++)
        if (off[s + 1] < off[s]) return pg_fail(h, PG_ERR_INVALID_ARG, "pg_fscore_submit: ss_off decreases at string %llu", (unsigned long long)s);
    const uint64_t total = off[ns] - off[0];
    if (total && !b->ss) return pg_fail(h, PG_ERR_INVALID_ARG, "pg_fscore_submit: null ss");
    const bool dev = b->location == PG_LOC_DEVICE;
    bool pinned = false;
    if (total) {
        const PgPtrKind kind = pg_ptr_kind(b->ss + off[0], h->device);
        if (dev && kind != PG_PTR_DEVICE)
            return pg_fail(h, PG_ERR_INVALID_ARG, "pg_fscore_submit: PG_LOC_DEVICE ss is not device memory of device %d", h->device);
        pinned = !dev && kind == PG_PTR_PINNED;
    }
    h->counts.resize(4 * (h->n_pairs + b->n_pairs));
    // pieces of whole pairs: at most kUnit bytes and kUnitPairs pairs, a larger pair alone
    uint64_t p0 = 0;
    while (p0 < b->n_pairs) {
        uint64_t p1 = p0 + 1;
        while (p1 < b->n_pairs && p1 - p0 < kUnitPairs && off[2 * (p1 + 1)] - off[2 * p0] <= kUnit) p1++;
        if (pg_status s = f1_piece(h, b->ss, dev, pinned, off, b->sig_start, b->first_ref, 2 * p0, (uint32_t)(2 * (p1 - p0)))) return s;
        p0 = p1;
    }
    // the caller may reuse its host memory once submit returns: pageable input was staged above, page-locked input is read by the copies
    if (pinned) PG_HIP_TRY(h, hipStreamSynchronize(h->st));
    return PG_OK;
}

pg_status pg_fscore_sync(pg_fscore *h) {
    if (!h) return pg_fail<pg_fscore>(nullptr, PG_ERR_INVALID_ARG, "pg_fscore_sync: null handle");
    PG_HIP_TRY(h, hipSetDevice(h->device));
    for (int k = 0; k < 2; k++) if (pg_status s = f1_drain(h, h->slot[h->next ^ k])) return s; // the older piece first
    return PG_OK;
}

pg_status pg_fscore_finish(pg_fscore *h, pg_fscore_result *out, uint64_t *pair_counts, uint64_t cap_pairs) {
    if (!h) return pg_fail<pg_fscore>(nullptr, PG_ERR_INVALID_ARG, "pg_fscore_finish: null handle");
    if (!out) return pg_fail(h, PG_ERR_INVALID_ARG, "pg_fscore_finish: null result");
    memset(out, 0, sizeof *out);
    pg_status st = pg_fscore_sync(h);
    if (st == PG_OK) {
        out->n_pairs = h->n_pairs;
        out->err_pair = -1;
        if (h->err_word != kNoErr) {
            static const char *what[] = {"", "ss is empty", "ss ends in a digit", "ss holds a byte outside ASCII", "an ss op count is 2^32 or more",
                                         "the alignment maps no signal point"};
            const uint64_t pair = h->err_first_pair + (h->err_word >> 8);
            const uint32_t code = (uint32_t)(h->err_word >> 1) & 127, side = (uint32_t)(h->err_word & 1);
            out->err_pair = (int64_t)pair;
            out->err_code = code;
            out->err_side = side;
            st = pg_fail(h, PG_ERR_INPUT, "pair %llu, file %u: %s", (unsigned long long)pair, side + 1, code < 6 ? what[code] : "?");
        } else {
            for (uint64_t i = 0; i < h->n_pairs; i++)
                for (int c = 0; c < 4; c++) out->totals[c] += h->counts[4 * i + c];
            if (pair_counts) memcpy(pair_counts, h->counts.data(), std::min(cap_pairs, h->n_pairs) * 4 * sizeof(uint64_t));
        }
    }
    // reset for the next run, also after an error
    h->n_pairs = 0; h->counts.clear(); h->err_word = kNoErr; h->err_first_pair = 0;
    return st;
}

} // extern "C"
