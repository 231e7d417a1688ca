// pg_kfreq.hip -- `poregen kmer_freq` on the device: a histogram of every k-byte window of every FASTQ sequence line
// (src/kmer_freq.cpp:160-187 of the reference), with the raw FASTQ bytes as input, delivered in pieces cut at any byte.
//
// The reference's rules, restated on the byte stream (the CLI, host/kmer_freq_cli.cpp, cites the lines):
//   * lines are getline()'s: they end after each '\n'; the last one may be unterminated. Line i is a sequence line iff i % 4 == 1.
//   * the last byte of every line is dropped (the '\n', or a real byte for an unterminated final line), every window of k
//     consecutive bytes of what remains is counted. So a window ending at stream offset e is counted iff its k bytes hold no '\n',
//     its line is a sequence line and e is not the LAST byte of the stream. That last condition is all the unterminated-final-line
//     rule needs: the window ending on a piece's last byte is settled by the next piece, and dropped by finish.
//   * ACGT windows go to a dense u64[4^k] histogram (2-bit codes, first base most significant: the lexicographic order of the
//     reference's generated k-mers); any other window ("odd window") is a key of its own bytes, appended to a device list.
//   * a NUL byte in a sequence line is refused (the reference's std::string(line) truncates there): device flag -> PG_ERR_INPUT.
//
// Work is cut into units of at most kUnit bytes (a host piece is staged unit by unit; a device piece is read in place). Per unit:
//   k_kf_lines : newlines per tile of kTile bytes                                     (reads the unit once)
//   k_kf_count : tile prefix -> line index mod 4 at every thread's first byte, rolling 2-bit code per thread over its kSpan
//                bytes (+ k-1 bytes of warm-up), LDS histogram for k <= 6, global u64 adds above; block 0 also settles the windows
//                that straddle the previous unit (the "seam") and writes the next unit's carried state (line index mod 4, the
//                open line's last <= k bytes) into the other slot of a two-slot state: no host round trip between units.
// Equal codes a thread meets back to back (homopolymers) are added once, as a run.
// The walk of a span and the seam are pg_kfreq_text.h, which the host test shim compiles too; here are their loader and sinks.
//
// Second input form, pg_kfreq_submit_reads: reads as a BAM record stores them, two 4-bit codes per byte (pg_kfreq_codes.h), each read a
// sequence line of its own. No lines to find, so one launch per submit (or per h->unit windows of it):
//   k_kf_reads : one wave per piece of at most `piece` window starts of one read (the host lists the pieces; neighbours overlap by the
//                k - 1 bases a window spans), the piece's windows spread evenly over the 64 lanes, each lane rolling over its share plus
//                k - 1 bases of warm-up with 8-byte loads. A read with the reverse flag is walked as stored and the window formed as
//                `samtools fastq` prints it: codes complemented, newest base most significant. Same histograms, same odd list.
//
// Third input form, pg_kfreq_submit_fasta: FASTA bytes, in pieces cut anywhere, units as for the FASTQ text. A line's kind is its first byte
// and a record's windows cross line ends, so the two facts the FASTQ kernels rest on are replaced (pg_kfreq_fasta.h has the rules and the
// record-tail monoid; DESIGN.md 9.2 the reasoning):
//   k_kf_fa_lines : per tile, the offset behind its last newline and the tile's summary (the last <= 11 sequence bytes in front of its
//                   first newline; behind it, whether a header line lies there and the last <= 11 sequence bytes after the last one)
//   k_kf_fa_count : prefix maximum of the tiles' line starts -> the kind of the line open at every tile's first byte (one byte read) ->
//                   the tiles' summaries resolved and folded in order -> the same again over the tile's 256 spans: every thread starts
//                   with the state a sequential walk holds at its first byte, and walks its span alone. Block 0 writes the carried
//                   state (kind of the open line, the open record's last <= 11 bytes). Nothing is deferred: a window is counted by the
//                   thread that holds its last byte, the stream's last byte included, so finish has nothing to settle.
#include "../../include/pgmove.h"
#include <hip/hip_runtime.h>
#include "pg_hip_host.h"
#include "pg_kfreq_codes.h"
#include "pg_kfreq_fasta.h"
#include "pg_kfreq_text.h"

#include <algorithm>
#include <cstdlib>
#include <cstring>
#include <deque>
#include <string>
#include <unordered_map>
#include <vector>

namespace {

// the geometry of the text kernels and KfState, the state carried across units: pg_kfreq_text.h
constexpr int kThreads = PG_KF_THREADS;
constexpr int kSpan = PG_KF_SPAN;                // bytes per thread
constexpr uint64_t kTile = PG_KF_TILE;           // 32 KiB per workgroup
constexpr uint64_t kUnit = PG_KF_UNIT;           // bytes per unit (512 tiles)
constexpr uint32_t kMaxK = PG_KF_MAX_K;
constexpr uint32_t kLdsMaxK = PG_KF_LDS_MAX_K;   // 4^6 u32 = 16 KiB of LDS
constexpr int kSnapRing = 64;                    // outstanding odd-count snapshots

struct KfFaState {     // the FASTA form's carried state, two slots like KfState; all zero at the start of a stream
    uint32_t kind;     // PG_FA_*: the line open at the unit's first byte (FRESH: it starts there)
    uint32_t pad;
    PgFaSum rec;       // the open record's last <= kFaTail sequence bytes
};
static_assert(kSpan == kFaSpan && kThreads == kFaTileSpans && kMaxK - 1 <= kFaTail, "pg_kfreq_fasta.h describes these spans and tiles");
static_assert(kUnit / kTile <= 2 * kThreads, "k_kf_fa_count folds two tile summaries per thread");

struct KfDev {
    unsigned long long *hist;  // u64[4^k]
    uint4 *odd;                // odd windows, k bytes each, zero padded
    unsigned long long *odd_n; // windows appended since the last drain (may exceed cap: those past it are lost -- never allowed)
    uint32_t *err;             // NUL in a sequence line
    KfState *state;            // [2]
    uint32_t *tile_nl;         // newlines per tile of the current unit
    uint32_t *tile_ls;         // FASTA: per tile, the offset in the unit behind its last newline ("line start"); 0 = the tile holds none
    PgFaSum *fa_tile;          // FASTA: per tile, [2 t] the bytes in front of its first newline, [2 t + 1] the rest (PgFaSpan's fa, pb)
    KfFaState *fa_state;       // [2]
    uint64_t odd_cap;
};

// this thread's kSpan bytes of the unit (or fewer at its end), as four-byte words in registers
template <bool kAligned>
__device__ __forceinline__ void load_span(const uint8_t *__restrict__ p, uint64_t base, uint64_t n, uint32_t (&w)[kSpan / 4]) {
    if (kAligned && base + kSpan <= n) {
        const uint4 *q = reinterpret_cast<const uint4 *>(p + base);
#pragma unroll
        for (int i = 0; i < kSpan / 16; i++) { const uint4 v = q[i]; w[4 * i] = v.x; w[4 * i + 1] = v.y; w[4 * i + 2] = v.z; w[4 * i + 3] = v.w; }
        return;
    }
#pragma unroll
    for (int i = 0; i < kSpan / 4; i++) {
        uint32_t x = 0;
        for (int b = 0; b < 4; b++) { const uint64_t o = base + 4 * i + b; if (o < n) x |= (uint32_t)p[o] << (8 * b); }
        w[i] = x;
    }
}

template <bool kAligned>
__device__ __forceinline__ uint4 load16(const uint8_t *__restrict__ p, uint64_t o, uint64_t n) {
    if (kAligned && o + 16 <= n) return *reinterpret_cast<const uint4 *>(p + o);
    uint32_t x[4] = {0, 0, 0, 0};
    for (int b = 0; b < 16; b++) if (o + b < n) x[b >> 2] |= (uint32_t)p[o + b] << (8 * (b & 3));
    return make_uint4(x[0], x[1], x[2], x[3]);
}

__device__ __forceinline__ uint32_t nl_in_word(uint32_t x) { // bytes equal to '\n'
    const uint32_t y = x ^ 0x0a0a0a0au;
    return __popc(~(((y & 0x7f7f7f7fu) + 0x7f7f7f7fu) | y | 0x7f7f7f7fu));
}

template <bool kAligned>
__global__ __launch_bounds__(kThreads) void k_kf_lines(const uint8_t *__restrict__ p, uint64_t n, uint32_t *__restrict__ tile_nl) {
    const uint64_t base = blockIdx.x * kTile + threadIdx.x * (uint64_t)kSpan;
    uint32_t w[kSpan / 4];
    uint32_t c = 0;
    if (base < n) {
        load_span<kAligned>(p, base, n, w);
#pragma unroll
        for (int i = 0; i < kSpan / 4; i++) c += nl_in_word(w[i]); // zero padding past n is no newline
    }
    __shared__ uint32_t red[kThreads / 64];
    for (int o = 32; o > 0; o >>= 1) c += __shfl_xor(c, o);
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = c;
    __syncthreads();
    if (threadIdx.x == 0) { uint32_t s = 0; for (int i = 0; i < kThreads / 64; i++) s += red[i]; tile_nl[blockIdx.x] = s; }
}

__device__ __forceinline__ uint4 odd_key(uint64_t lo, uint32_t hi, uint32_t k) {
    uint32_t key[4];
    pg_kf_odd_key(lo, hi, k, key);
    return make_uint4(key[0], key[1], key[2], key[3]);
}

__device__ __forceinline__ void emit_odd(const KfDev &d, uint4 key) {
    const unsigned long long i = atomicAdd(d.odd_n, 1ull);
    if (i < d.odd_cap) d.odd[i] = key;
}

// odd windows of a workgroup are gathered in LDS and appended with one global add per workgroup; past kOddLds they go out one by one
constexpr uint32_t kOddLds = PG_KF_ODD_LDS;
__device__ __forceinline__ void stage_odd(const KfDev &d, uint4 *s_odd, uint32_t *s_odd_n, uint4 key) {
    const uint32_t i = atomicAdd(s_odd_n, 1u);
    if (i < kOddLds) s_odd[i] = key;
    else emit_odd(d, key);
}

template <bool kLds>
__device__ __forceinline__ void add_run(const KfDev &d, uint32_t *lds, uint32_t code, uint32_t cnt) {
    if (!cnt) return;
    if (kLds) atomicAdd(&lds[code], cnt);
    else atomicAdd(&d.hist[code], (unsigned long long)cnt);
}

// The end of a text kernel, all threads of the workgroup: the open run of every thread (the wave is converged here) -- where all of a
// wave's runs share one code, a homopolymer, one lane adds their sum, instead of 64 adds to one address -- then the staged odd windows
// and the LDS histogram.
template <bool kLds>
__device__ __forceinline__ void kf_flush(const KfDev &d, uint32_t *lds_hist, uint32_t n_codes, uint32_t run_code, uint32_t run_cnt,
                                         const uint4 *s_odd, const uint32_t *s_odd_n, unsigned long long *s_odd_at) {
    const uint32_t tid = threadIdx.x;
    const uint32_t c0 = __builtin_amdgcn_readfirstlane(run_code);
    const bool lone = __ballot(run_cnt != 0 && run_code != c0) != 0;
    if (lone) {
        add_run<kLds>(d, lds_hist, run_code, run_cnt);
    } else {
        uint32_t sum = run_cnt;
        for (int o = 32; o > 0; o >>= 1) sum += __shfl_xor(sum, o);
        if ((tid & 63) == 0) add_run<kLds>(d, lds_hist, c0, sum);
    }
    __syncthreads();
    const uint32_t n_staged = min(*s_odd_n, kOddLds);
    if (n_staged) {
        if (tid == 0) *s_odd_at = atomicAdd(d.odd_n, (unsigned long long)n_staged);
        __syncthreads();
        for (uint32_t i = tid; i < n_staged; i += kThreads)
            if (*s_odd_at + i < d.odd_cap) d.odd[*s_odd_at + i] = s_odd[i];
    }
    if (kLds) {
        for (uint32_t i = tid; i < n_codes; i += kThreads)
            if (const uint32_t v = lds_hist[i]) atomicAdd(&d.hist[i], (unsigned long long)v);
    }
}

// The sinks of the walks (pg_kfreq_text.h: pg_kf_walk, pg_kf_seam; pg_kfreq_fasta.h: pg_fa_walk) and the loader of a span's 16-byte chunks.
// A thread's sink merges equal codes met back to back into a run (kf_flush adds the open one) and stages its odd windows in LDS.
template <bool kLds>
struct KfSink {
    const KfDev &d;
    uint32_t *lds_hist;
    uint4 *s_odd;
    uint32_t *s_odd_n;
    uint32_t k, run_code, run_cnt;
    __device__ __forceinline__ void dense(uint32_t code) {
        if (code == run_code) run_cnt++;
        else { add_run<kLds>(d, lds_hist, run_code, run_cnt); run_code = code; run_cnt = 1; }
    }
    __device__ __forceinline__ void odd(uint64_t lo, uint32_t hi) { stage_odd(d, s_odd, s_odd_n, odd_key(lo, hi, k)); }
};
struct KfSeamSink { // block 0, thread 0: a handful of windows per unit, added one by one
    const KfDev &d;
    uint32_t k;
    __device__ __forceinline__ void dense(uint32_t code) { atomicAdd(&d.hist[code], 1ull); }
    __device__ __forceinline__ void odd(uint64_t lo, uint32_t hi) { emit_odd(d, odd_key(lo, hi, k)); }
};
template <bool kAligned>
struct KfLoad {
    const uint8_t *p;
    uint64_t base, n;
    __device__ __forceinline__ void operator()(uint32_t ch, uint32_t (&ws)[4]) const {
        const uint4 v = load16<kAligned>(p, base + 16 * ch, n); // second read of the span: served by the cache
        ws[0] = v.x; ws[1] = v.y; ws[2] = v.z; ws[3] = v.w;
    }
};

// block 0, thread 0: windows that start in the carried tail and end in this unit, then the state the next unit starts from
__device__ void kf_seam(const KfDev &d, const uint8_t *__restrict__ p, uint64_t n, uint32_t k, uint32_t par, uint32_t total_nl) {
    const KfState s = d.state[par];
    KfSeamSink sink{d, k};
    d.state[par ^ 1] = pg_kf_seam(s, p, n, k, total_nl, sink);
}

template <bool kAligned, bool kLds>
__global__ __launch_bounds__(kThreads) void k_kf_count(KfDev d, const uint8_t *__restrict__ p, uint64_t n, uint32_t n_tiles, uint32_t k, uint32_t par) {
    extern __shared__ uint32_t lds_hist[];
    __shared__ uint32_t s_scan[kThreads];
    __shared__ uint32_t s_red[kThreads / 64];
    __shared__ uint4 s_odd[kOddLds];
    __shared__ uint32_t s_odd_n;
    __shared__ unsigned long long s_odd_at;
    const uint32_t tid = threadIdx.x;
    if (tid == 0) s_odd_n = 0;
    const uint32_t n_codes = 1u << (2 * k);
    if (kLds) for (uint32_t i = tid; i < n_codes; i += kThreads) lds_hist[i] = 0;

    // newlines in front of this tile (block 0: in front of the whole unit's end, for the next state)
    const uint32_t upto = blockIdx.x == 0 ? n_tiles : blockIdx.x;
    uint32_t pre = 0;
    for (uint32_t i = tid; i < upto; i += kThreads) pre += d.tile_nl[i];
    for (int o = 32; o > 0; o >>= 1) pre += __shfl_xor(pre, o);
    if ((tid & 63) == 0) s_red[tid >> 6] = pre;

    const uint64_t base = blockIdx.x * kTile + tid * (uint64_t)kSpan;
    uint32_t w[kSpan / 4];
    uint32_t my_nl = 0;
    if (base < n) {
        load_span<kAligned>(p, base, n, w);
#pragma unroll
        for (int i = 0; i < kSpan / 4; i++) my_nl += nl_in_word(w[i]);
    }
    s_scan[tid] = my_nl;
    __syncthreads();
    uint32_t tile_pre = 0;
    for (int i = 0; i < kThreads / 64; i++) tile_pre += s_red[i];
    if (blockIdx.x == 0) {
        if (tid == 0) kf_seam(d, p, n, k, par, tile_pre);
        tile_pre = 0;
    }
    // exclusive scan of the per-thread newline counts (mod 4 is all that is needed; plain sums do not overflow)
    for (uint32_t off = 1; off < kThreads; off <<= 1) {
        const uint32_t x = tid >= off ? s_scan[tid - off] : 0;
        __syncthreads();
        s_scan[tid] += x;
        __syncthreads();
    }
    const uint32_t excl = s_scan[tid] - my_nl;
    const KfState st = d.state[par];
    uint32_t mod4 = (st.mod4 + tile_pre + excl) & 3;

    KfSink<kLds> sink{d, lds_hist, s_odd, &s_odd_n, k, 0, 0};
    if (base < n) {
        KfLoad<kAligned> load{p, base, n};
        if (pg_kf_walk(p, base, n, k, mod4, load, sink)) atomicOr(d.err, 1u);
    }
    kf_flush<kLds>(d, lds_hist, n_codes, sink.run_code, sink.run_cnt, s_odd, &s_odd_n, &s_odd_at);
}

// ---- FASTA text ------------------------------------------------------------------------------------------------------------------
__device__ __forceinline__ PgFaSum fa_shfl_up(const PgFaSum &v, int delta) {
    PgFaSum r;
    r.lo = (uint64_t)__shfl_up((uint32_t)(v.lo >> 32), delta) << 32 | __shfl_up((uint32_t)v.lo, delta);
    r.hi = __shfl_up(v.hi, delta);
    r.meta = __shfl_up(v.meta, delta);
    return r;
}

// Scans over the workgroup's threads in thread order (all threads call; s_w: one LDS entry per wave, free again on return).
// The maximum of x over the threads in front of this one (0 if none); *total: over all of them.
__device__ __forceinline__ uint32_t block_max_before(uint32_t x, uint32_t *s_w, uint32_t *total) {
    const uint32_t lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    for (int o = 1; o < 64; o <<= 1) { const uint32_t y = __shfl_up(x, o); if (lane >= (uint32_t)o) x = max(x, y); }
    if (lane == 63) s_w[wave] = x;
    uint32_t before = __shfl_up(x, 1);
    if (lane == 0) before = 0;
    __syncthreads();
    uint32_t all = 0;
    for (uint32_t i = 0; i < kThreads / 64; i++) { if (i == wave) before = max(before, all); all = max(all, s_w[i]); }
    __syncthreads();
    *total = all;
    return before;
}
// The composition of v over the threads in front of this one; *total: over all of them.
__device__ __forceinline__ PgFaSum block_compose_before(PgFaSum v, PgFaSum *s_w, PgFaSum *total) {
    const uint32_t lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    for (int o = 1; o < 64; o <<= 1) { const PgFaSum u = fa_shfl_up(v, o); if (lane >= (uint32_t)o) v = pg_fa_compose(u, v); }
    if (lane == 63) s_w[wave] = v;
    PgFaSum before = fa_shfl_up(v, 1);
    if (lane == 0) before = pg_fa_empty();
    __syncthreads();
    PgFaSum all = pg_fa_empty();
    for (uint32_t i = 0; i < kThreads / 64; i++) { if (i == wave) before = pg_fa_compose(all, before); all = pg_fa_compose(all, s_w[i]); }
    __syncthreads();
    *total = all;
    return before;
}

template <bool kAligned>
__global__ __launch_bounds__(kThreads) void k_kf_fa_lines(const uint8_t *__restrict__ p, uint64_t n, uint32_t *__restrict__ tile_ls, PgFaSum *__restrict__ fa_tile) {
    __shared__ uint32_t s_m[kThreads / 64];
    __shared__ PgFaSum s_w[kThreads / 64];
    const uint64_t tile0 = blockIdx.x * kTile, base = tile0 + threadIdx.x * (uint64_t)kSpan;
    PgFaSpan sp;
    sp.fa = sp.pb = pg_fa_empty(); sp.has_nl = 0; sp.last_nl = 0;
    uint32_t first_byte = 0;
    if (base < n) {
        uint32_t w[kSpan / 4];
        load_span<kAligned>(p, base, n, w);
        pg_fa_span_summary(w, (uint32_t)min<uint64_t>(kSpan, n - base), sp);
        first_byte = w[0] & 0xff;
    }
    // where the line open at this span's first byte starts, if that is inside the tile (a unit has < 2^32 bytes). An offset behind a
    // newline is at least 1, so 0 stands for "no newline" and the maximum needs no flag.
    uint32_t tile_last;
    const uint32_t ls = block_max_before(sp.has_nl ? (uint32_t)base + sp.last_nl + 1 : 0, s_m, &tile_last);
    // the part of the tile behind its first newline: there the kind of every span's first line is known
    PgFaSum e = sp.pb;
    if (ls != 0 && base < n) e = pg_fa_resolve(pg_fa_kind_at(p, ls, base, PG_FA_SEQ), first_byte, sp.fa, sp.pb);
    PgFaSum rest;
    block_compose_before(e, s_w, &rest);
    if (threadIdx.x == 0) { tile_ls[blockIdx.x] = tile_last; fa_tile[2 * blockIdx.x + 1] = rest; }
    // the part in front of it: its last <= kFaTail bytes lie side by side in front of that newline (or of the tile's end)
    const bool owner = tile_last == 0 ? threadIdx.x == 0 : ls == 0 && sp.has_nl;
    if (owner) {
        uint64_t end = min<uint64_t>(n, tile0 + kTile);
        if (sp.has_nl) { uint32_t first = 0; while (p[base + first] != '\n') first++; end = base + first; }
        PgFaSum f = pg_fa_empty();
        for (uint64_t q = end - tile0 > kFaTail ? end - kFaTail : tile0; q < end; q++) pg_fa_append(f, p[q]);
        fa_tile[2 * blockIdx.x] = f;
    }
}

template <bool kAligned, bool kLds>
__global__ __launch_bounds__(kThreads) void k_kf_fa_count(KfDev d, const uint8_t *__restrict__ p, uint64_t n, uint32_t n_tiles, uint32_t k, uint32_t par) {
    extern __shared__ uint32_t lds_hist[];
    __shared__ uint32_t s_m[kThreads / 64];
    __shared__ PgFaSum s_w[kThreads / 64];
    __shared__ uint4 s_odd[kOddLds];
    __shared__ uint32_t s_odd_n;
    __shared__ unsigned long long s_odd_at;
    const uint32_t tid = threadIdx.x;
    if (tid == 0) s_odd_n = 0;
    const uint32_t n_codes = 1u << (2 * k);
    if (kLds) for (uint32_t i = tid; i < n_codes; i += kThreads) lds_hist[i] = 0;
    const KfFaState st = d.fa_state[par];

    // the tiles in front of this one (block 0: all of them, for the next unit's state), two per thread: where the line open at each
    // tile's first byte starts -> its kind -> the tile's effect on the record tail; folded in order
    const uint32_t upto = blockIdx.x == 0 ? n_tiles : blockIdx.x;
    const uint32_t t0 = 2 * tid, t1 = t0 + 1;
    const uint32_t ls0 = t0 < upto ? d.tile_ls[t0] : 0, ls1 = t1 < upto ? d.tile_ls[t1] : 0; // 0: no newline in the tile (a line start is >= 1)
    uint32_t line_in;
    const uint32_t ls_t0 = block_max_before(max(ls0, ls1), s_m, &line_in);
    PgFaSum e = pg_fa_empty();
    if (t0 < upto) e = pg_fa_resolve(pg_fa_kind_at(p, ls_t0, t0 * kTile, st.kind), p[t0 * kTile], d.fa_tile[2 * t0], d.fa_tile[2 * t0 + 1]);
    if (t1 < upto) e = pg_fa_compose(e, pg_fa_resolve(pg_fa_kind_at(p, max(ls_t0, ls0), t1 * kTile, st.kind), p[t1 * kTile], d.fa_tile[2 * t1], d.fa_tile[2 * t1 + 1]));
    PgFaSum rec_in;
    block_compose_before(e, s_w, &rec_in);
    rec_in = pg_fa_compose(st.rec, rec_in);
    if (blockIdx.x == 0) {
        if (tid == 0) { KfFaState o; o.kind = pg_fa_kind_at(p, line_in, n, st.kind); o.pad = 0; o.rec = rec_in; d.fa_state[par ^ 1] = o; }
        line_in = 0; rec_in = st.rec;
    }

    // the same over this tile's spans
    const uint64_t base = blockIdx.x * kTile + tid * (uint64_t)kSpan;
    const uint32_t lim = base < n ? (uint32_t)min<uint64_t>(kSpan, n - base) : 0;
    PgFaSpan sp;
    sp.fa = sp.pb = pg_fa_empty(); sp.has_nl = 0; sp.last_nl = 0;
    uint32_t first_byte = 0;
    if (lim) {
        uint32_t w[kSpan / 4];
        load_span<kAligned>(p, base, n, w);
        pg_fa_span_summary(w, lim, sp);
        first_byte = w[0] & 0xff;
    }
    uint32_t unused;
    const uint32_t ls = max(line_in, block_max_before(sp.has_nl ? (uint32_t)base + sp.last_nl + 1 : 0, s_m, &unused));
    const uint32_t kind = lim ? pg_fa_kind_at(p, ls, base, st.kind) : (uint32_t)PG_FA_SEQ;
    PgFaSum all;
    const PgFaSum rec = pg_fa_compose(rec_in, block_compose_before(lim ? pg_fa_resolve(kind, first_byte, sp.fa, sp.pb) : pg_fa_empty(), s_w, &all));

    KfSink<kLds> sink{d, lds_hist, s_odd, &s_odd_n, k, 0, 0};
    if (lim) {
        KfLoad<kAligned> load{p, base, n};
        if (pg_fa_walk(load, lim, k, kind, rec, sink)) atomicOr(d.err, 1u);
    }
    kf_flush<kLds>(d, lds_hist, n_codes, sink.run_code, sink.run_cnt, s_odd, &s_odd_n, &s_odd_at);
}

// ---- packed reads ---------------------------------------------------------------------------------------------------------------
constexpr uint32_t kReadPiece = 4096;            // window starts per wave of work: 64 per lane
constexpr uint32_t kReadBlocks = 512;            // workgroups of a launch at most (two per CU); waves stride over the pieces
constexpr uint32_t kMaxReadLen = 0x7fffffffu;    // BAM's l_seq is an int32

struct KfReads {
    const uint8_t *seq;      // n_bytes bytes; read r starts at byte off[r], high nibble first
    uint64_t n_bytes;
    const uint64_t *off;
    const uint32_t *len;
    const uint8_t *rev;
    const uint2 *work;       // (read, piece) of every piece of this launch
    uint32_t n_work, piece, n_to_t;
};

template <bool kAligned>
__device__ __forceinline__ uint64_t load8(const uint8_t *__restrict__ p, uint64_t o, uint64_t n) {
    if (kAligned && o + 8 <= n) return *reinterpret_cast<const unsigned long long *>(p + o);
    uint64_t x = 0;
    for (int b = 0; b < 8; b++) if (o + b < n) x |= (uint64_t)p[o + b] << (8 * b);
    return x;
}

__device__ __forceinline__ uint4 odd_key_rev(uint64_t lo, uint32_t hi, uint32_t k) {
    // the window read backwards: byte i of the key is i bytes older than the newest
    uint32_t key[4] = {0, 0, 0, 0};
    for (uint32_t i = 0; i < k; i++) {
        const uint32_t b = i < 8 ? (uint32_t)(lo >> (8 * i)) & 0xff : (hi >> (8 * (i - 8))) & 0xff;
        key[i >> 2] |= b << (8 * (i & 3));
    }
    return make_uint4(key[0], key[1], key[2], key[3]);
}

template <bool kAligned, bool kLds>
__global__ __launch_bounds__(kThreads) void k_kf_reads(KfDev d, KfReads in, uint32_t k) {
    extern __shared__ uint32_t lds_hist[];
    const uint32_t tid = threadIdx.x, lane = tid & 63;
    const uint32_t n_codes = 1u << (2 * k), mask = n_codes - 1, top = 2 * (k - 1);
    if (kLds) {
        for (uint32_t i = tid; i < n_codes; i += kThreads) lds_hist[i] = 0;
        __syncthreads();
    }
    constexpr uint32_t kWaves = kThreads / 64;
    uint32_t run_code = 0, run_cnt = 0; // the open run lives across pieces
    for (uint32_t w = blockIdx.x * kWaves + (tid >> 6); w < in.n_work; w += gridDim.x * kWaves) {
        const uint2 it = in.work[w];
        const uint32_t len = in.len[it.x];
        const bool rev = in.rev[it.x] != 0;
        const uint64_t nib0 = in.off[it.x] * 2; // the read's first base, counted in nibbles from seq
        if (len < k) continue;
        const uint32_t n_win = len - k + 1;
        const uint64_t ws = (uint64_t)it.y * in.piece;
        if (ws >= n_win) continue;
        const uint32_t we = (uint32_t)min<uint64_t>(n_win, ws + in.piece);
        const uint32_t span = (we - (uint32_t)ws + 63) / 64;
        const uint64_t a = ws + (uint64_t)lane * span;           // this lane's window starts: [a, b)
        if (a >= we) continue;
        const uint64_t b = min<uint64_t>(we, a + span);
        uint64_t cur = 0, lo = 0;
        uint32_t hi = 0, run = 0, code = 0;
        for (uint64_t j = a; j < b + k - 1; j++) {               // bases [a, b + k - 1) of the read as stored: below len
            const uint64_t q = nib0 + j;
            if (j == a || (q & 15) == 0) cur = load8<kAligned>(in.seq, (q >> 4) << 3, in.n_bytes);
            uint32_t c = (uint32_t)(cur >> (4 * ((q & 15) ^ 1))) & 15;
            if (rev) c = pg_kf_complement(c);
            if (in.n_to_t && c == 15) c = 8;
            const bool acgt = c != 0 && (c & (c - 1)) == 0;      // exactly one base
            const uint32_t b2 = acgt ? (uint32_t)__ffs((int)c) - 1 : 0;
            run = acgt ? run + 1 : 0;
            code = rev ? (code >> 2) | (b2 << top) : ((code << 2) | b2) & mask;
            hi = (hi << 8) | (uint32_t)(lo >> 56); lo = (lo << 8) | pg_kf_letter(c);
            if (j - a + 1 >= k) {
                if (run >= k) {
                    if (code == run_code) run_cnt++;
                    else { add_run<kLds>(d, lds_hist, run_code, run_cnt); run_code = code; run_cnt = 1; }
                } else {
                    emit_odd(d, rev ? odd_key_rev(lo, hi, k) : odd_key(lo, hi, k));
                }
            }
        }
    }
    // as in k_kf_count: a wave whose open runs all share one code adds their sum from one lane
    const uint32_t c0 = __builtin_amdgcn_readfirstlane(run_code);
    const bool lone = __ballot(run_cnt != 0 && run_code != c0) != 0;
    if (lone) {
        add_run<kLds>(d, lds_hist, run_code, run_cnt);
    } else {
        uint32_t sum = run_cnt;
        for (int o = 32; o > 0; o >>= 1) sum += __shfl_xor(sum, o);
        if (lane == 0) add_run<kLds>(d, lds_hist, c0, sum);
    }
    if (kLds) {
        __syncthreads();
        for (uint32_t i = tid; i < n_codes; i += kThreads)
            if (const uint32_t v = lds_hist[i]) atomicAdd(&d.hist[i], (unsigned long long)v);
    }
}

struct OddKey {
    uint32_t w[4];
    bool operator==(const OddKey &o) const { return memcmp(w, o.w, sizeof w) == 0; }
};
struct OddHash {
    size_t operator()(const OddKey &k) const {
        uint64_t a = ((uint64_t)k.w[1] << 32 | k.w[0]) * 0x9E3779B97F4A7C15ull, b = ((uint64_t)k.w[3] << 32 | k.w[2]) * 0xC2B2AE3D27D4EB4Full;
        return (size_t)(a ^ (b >> 29) ^ (a >> 31));
    }
};

} // namespace

struct pg_kfreq {
    uint32_t k = 0, n_codes = 0;
    int device = 0;
    uint64_t unit = kUnit; // <= odd_cap: a unit never has more windows than the list holds
    PgStream ks, cs; // count stream, copy stream (host input)
    PgEvent copied[2], counted[2], snap_ev[kSnapRing];
    PgDev<> mem[9];  // what d points to, in the order of KfDev's members
    KfDev d{};
    uint32_t par = 0;
    // host input: two pinned staging buffers and their device copies
    PgPinned<uint8_t> stage[2];
    PgDev<uint8_t> dbuf[2];
    int next_buf = 0;
    // odd-list fill: exact counts read back asynchronously, one snapshot per unit
    PgPinned<unsigned long long> snap; // [kSnapRing]
    struct Pending { int slot; uint64_t bound; };
    std::deque<Pending> pending;
    int snap_next = 0;
    uint64_t odd_known = 0;              // exact list fill as of the newest completed snapshot (or drain)
    std::unordered_map<OddKey, uint64_t, OddHash> odd_map;
    std::vector<uint4> drain_buf;
    // finish output
    std::vector<uint8_t> out_keys;
    std::vector<uint64_t> out_counts;
    bool aligned_stage = true;
    // packed reads: what one submit uploads (sequence bytes, offsets, lengths, flags, the piece list) as one block, two in rotation
    int form = 0;              // the stream's input form: 0 none yet, 1 FASTQ text, 2 reads, 3 FASTA text
    uint32_t piece = kReadPiece; // <= unit
    PgPinned<uint8_t> r_stage[2];
    PgDev<uint8_t> r_dev[2];
    std::vector<uint64_t> r_off;   // PG_LOC_DEVICE: the caller's offsets and lengths, brought over to plan the pieces
    std::vector<uint32_t> r_len;
    std::vector<uint2> r_work;
    std::string err;
};

static const char *const kFormName[4] = {"nothing", "FASTQ text", "packed reads", "FASTA text"};

static uint64_t odd_cap_from_env() {
    if (const char *s = getenv("PGKFREQ_ODD_CAP")) { const long long v = atoll(s); if (v >= 1) return (uint64_t)v; }
    return 3 * kUnit; // three units' worth of windows: a unit may be launched while two are still unread (kf_reserve)
}

// Fold the device odd list into the host map and empty it. The count stream must be idle.
static pg_status kf_drain(pg_kfreq *h) {
    unsigned long long n = 0;
    PG_HIP_TRY(h, hipMemcpy(&n, h->d.odd_n, sizeof n, hipMemcpyDeviceToHost));
    if (n > h->d.odd_cap) return pg_fail(h, PG_ERR_STATE, "internal: odd-window list overflowed (%llu > %llu)", n, (unsigned long long)h->d.odd_cap);
    if (n) {
        h->drain_buf.resize(n);
        PG_HIP_TRY(h, hipMemcpy(h->drain_buf.data(), h->d.odd, n * sizeof(uint4), hipMemcpyDeviceToHost));
        for (const uint4 &v : h->drain_buf) { OddKey key{{v.x, v.y, v.z, v.w}}; h->odd_map[key]++; }
        PG_HIP_TRY(h, hipMemsetAsync(h->d.odd_n, 0, sizeof(unsigned long long), h->ks));
        PG_HIP_TRY(h, hipStreamSynchronize(h->ks));
    }
    h->odd_known = 0;
    h->pending.clear();
    return PG_OK;
}

// Before a unit of n bytes is launched: make sure the odd list has room for all its windows. The exact fill is known from the
// snapshots of earlier units that have completed (never waited for while the bound is low); only when the bound says the list
// could overflow does the host wait, and only when the exact fill says so does it drain.
static pg_status kf_reserve(pg_kfreq *h, uint64_t n) {
    while (!h->pending.empty() && hipEventQuery(h->snap_ev[h->pending.front().slot]) == hipSuccess) {
        h->odd_known = h->snap.p[h->pending.front().slot];
        h->pending.pop_front();
    }
    uint64_t bound = h->odd_known + n;
    for (const auto &q : h->pending) bound += q.bound;
    if (bound <= h->d.odd_cap && (int)h->pending.size() < kSnapRing - 1) return PG_OK;
    if (!h->pending.empty()) {
        PG_HIP_TRY(h, hipEventSynchronize(h->snap_ev[h->pending.back().slot]));
        h->odd_known = h->snap.p[h->pending.back().slot];
        h->pending.clear();
    }
    if (h->odd_known + n > h->d.odd_cap) {
        PG_HIP_TRY(h, hipStreamSynchronize(h->ks));
        return kf_drain(h);
    }
    return PG_OK;
}

// behind a launch of at most n windows: the odd list's fill as of its end, on its way to the host
static pg_status kf_snapshot(pg_kfreq *h, uint64_t n) {
    const int slot = h->snap_next; h->snap_next = (h->snap_next + 1) % kSnapRing;
    PG_HIP_TRY(h, hipMemcpyAsync(&h->snap.p[slot], h->d.odd_n, sizeof(unsigned long long), hipMemcpyDeviceToHost, h->ks));
    PG_HIP_TRY(h, hipEventRecord(h->snap_ev[slot], h->ks));
    h->pending.push_back({slot, n});
    return PG_OK;
}

// one unit of at most kUnit bytes, resident on the device, complete on the count stream's side
static pg_status kf_unit(pg_kfreq *h, const uint8_t *p, uint64_t n) {
    if (!n) return PG_OK;
    if (pg_status s = kf_reserve(h, n)) return s;
    const uint32_t n_tiles = (uint32_t)((n + kTile - 1) / kTile);
    const bool al = ((uintptr_t)p & 15) == 0;
    const bool lds = h->k <= kLdsMaxK;
    const size_t lds_bytes = lds ? (size_t)h->n_codes * sizeof(uint32_t) : 0;
    if (h->form == 3) {
        if (al) hipLaunchKernelGGL(k_kf_fa_lines<true>, dim3(n_tiles), dim3(kThreads), 0, h->ks, p, n, h->d.tile_ls, h->d.fa_tile);
        else hipLaunchKernelGGL(k_kf_fa_lines<false>, dim3(n_tiles), dim3(kThreads), 0, h->ks, p, n, h->d.tile_ls, h->d.fa_tile);
        if (al && lds) hipLaunchKernelGGL((k_kf_fa_count<true, true>), dim3(n_tiles), dim3(kThreads), lds_bytes, h->ks, h->d, p, n, n_tiles, h->k, h->par);
        else if (al) hipLaunchKernelGGL((k_kf_fa_count<true, false>), dim3(n_tiles), dim3(kThreads), 0, h->ks, h->d, p, n, n_tiles, h->k, h->par);
        else if (lds) hipLaunchKernelGGL((k_kf_fa_count<false, true>), dim3(n_tiles), dim3(kThreads), lds_bytes, h->ks, h->d, p, n, n_tiles, h->k, h->par);
        else hipLaunchKernelGGL((k_kf_fa_count<false, false>), dim3(n_tiles), dim3(kThreads), 0, h->ks, h->d, p, n, n_tiles, h->k, h->par);
        PG_HIP_TRY(h, hipGetLastError());
        h->par ^= 1;
        return kf_snapshot(h, n);
    }
    if (al) hipLaunchKernelGGL(k_kf_lines<true>, dim3(n_tiles), dim3(kThreads), 0, h->ks, p, n, h->d.tile_nl);
    else hipLaunchKernelGGL(k_kf_lines<false>, dim3(n_tiles), dim3(kThreads), 0, h->ks, p, n, h->d.tile_nl);
    if (al && lds) hipLaunchKernelGGL((k_kf_count<true, true>), dim3(n_tiles), dim3(kThreads), lds_bytes, h->ks, h->d, p, n, n_tiles, h->k, h->par);
    else if (al) hipLaunchKernelGGL((k_kf_count<true, false>), dim3(n_tiles), dim3(kThreads), 0, h->ks, h->d, p, n, n_tiles, h->k, h->par);
    else if (lds) hipLaunchKernelGGL((k_kf_count<false, true>), dim3(n_tiles), dim3(kThreads), lds_bytes, h->ks, h->d, p, n, n_tiles, h->k, h->par);
    else hipLaunchKernelGGL((k_kf_count<false, false>), dim3(n_tiles), dim3(kThreads), 0, h->ks, h->d, p, n, n_tiles, h->k, h->par);
    PG_HIP_TRY(h, hipGetLastError());
    h->par ^= 1;
    return kf_snapshot(h, n);
}

static pg_status kf_reset_device(pg_kfreq *h) {
    PG_HIP_TRY(h, hipMemsetAsync(h->d.hist, 0, (size_t)h->n_codes * sizeof(unsigned long long), h->ks));
    PG_HIP_TRY(h, hipMemsetAsync(h->d.odd_n, 0, sizeof(unsigned long long), h->ks));
    PG_HIP_TRY(h, hipMemsetAsync(h->d.err, 0, sizeof(uint32_t), h->ks));
    PG_HIP_TRY(h, hipMemsetAsync(h->d.state, 0, 2 * sizeof(KfState), h->ks));
    PG_HIP_TRY(h, hipMemsetAsync(h->d.fa_state, 0, 2 * sizeof(KfFaState), h->ks));
    PG_HIP_TRY(h, hipStreamSynchronize(h->ks));
    h->par = 0;
    h->form = 0;
    h->pending.clear();
    h->odd_known = 0;
    h->odd_map.clear();
    return PG_OK;
}

extern "C" {

const char *pg_kfreq_last_error(const pg_kfreq *h) { return h ? h->err.c_str() : pg_create_error<pg_kfreq>().c_str(); }

pg_status pg_kfreq_create(uint32_t kmer_size, int32_t device, pg_kfreq **out) {
    if (!out) return pg_fail<pg_kfreq>(nullptr, PG_ERR_INVALID_ARG, "pg_kfreq_create: null argument");
    *out = nullptr;
    if (kmer_size < 1 || kmer_size > kMaxK) return pg_fail<pg_kfreq>(nullptr, PG_ERR_INVALID_ARG, "kmer_size must be in [1,%u]", kMaxK);
    if (pg_status st = pg_select_device<pg_kfreq>(device)) return st;
    pg_kfreq *h = new pg_kfreq();
    h->k = kmer_size; h->n_codes = 1u << (2 * kmer_size); h->device = device;
    h->d.odd_cap = odd_cap_from_env();
    h->unit = std::min<uint64_t>(kUnit, h->d.odd_cap);
    h->piece = (uint32_t)std::min<uint64_t>(kReadPiece, h->unit);
    auto init = [&]() -> pg_status {
        PG_HIP_TRY(h, hipStreamCreateWithFlags(&h->ks.h, hipStreamNonBlocking));
        PG_HIP_TRY(h, hipStreamCreateWithFlags(&h->cs.h, hipStreamNonBlocking));
        const size_t bytes[9] = {(size_t)h->n_codes * sizeof(unsigned long long), h->d.odd_cap * sizeof(uint4), sizeof(unsigned long long),
                                 sizeof(uint32_t), 2 * sizeof(KfState), (kUnit / kTile) * sizeof(uint32_t), (kUnit / kTile) * sizeof(uint32_t),
                                 2 * (kUnit / kTile) * sizeof(PgFaSum), 2 * sizeof(KfFaState)};
        for (int i = 0; i < 9; i++) PG_HIP_TRY(h, h->mem[i].ensure(bytes[i]));
        h->d.hist = h->mem[0].as<unsigned long long>(); h->d.odd = h->mem[1].as<uint4>(); h->d.odd_n = h->mem[2].as<unsigned long long>();
        h->d.err = h->mem[3].as<uint32_t>(); h->d.state = h->mem[4].as<KfState>(); h->d.tile_nl = h->mem[5].as<uint32_t>();
        h->d.tile_ls = h->mem[6].as<uint32_t>(); h->d.fa_tile = h->mem[7].as<PgFaSum>(); h->d.fa_state = h->mem[8].as<KfFaState>();
        PG_HIP_TRY(h, h->snap.ensure(kSnapRing * sizeof(unsigned long long)));
        for (auto &ev : h->snap_ev) PG_HIP_TRY(h, hipEventCreateWithFlags(&ev.h, hipEventDisableTiming));
        for (int i = 0; i < 2; i++) {
            PG_HIP_TRY(h, hipEventCreateWithFlags(&h->copied[i].h, hipEventDisableTiming));
            PG_HIP_TRY(h, hipEventCreateWithFlags(&h->counted[i].h, hipEventDisableTiming));
        }
        return kf_reset_device(h);
    };
    if (pg_status st = init()) return pg_create_failed(h, st, pg_kfreq_destroy);
    *out = h;
    return PG_OK;
}

void pg_kfreq_destroy(pg_kfreq *h) {
    if (!h) return;
    (void)hipSetDevice(h->device);
    if (h->ks) (void)hipStreamSynchronize(h->ks);
    if (h->cs) (void)hipStreamSynchronize(h->cs);
    delete h;
}

static pg_status kf_submit_text(pg_kfreq *h, const void *data, uint64_t n_bytes, int32_t location, int form, const char *fn) {
    if (!h) return pg_fail<pg_kfreq>(nullptr, PG_ERR_INVALID_ARG, "%s: null handle", fn);
    if (!n_bytes) return PG_OK;
    if (!data) return pg_fail(h, PG_ERR_INVALID_ARG, "%s: null data", fn);
    if (h->form && h->form != form) return pg_fail(h, PG_ERR_INVALID_ARG, "%s: this stream holds %s (one input form per stream)", fn, kFormName[h->form]);
    if (location != PG_LOC_HOST && location != PG_LOC_DEVICE) return pg_fail(h, PG_ERR_INVALID_ARG, "%s: location must be PG_LOC_HOST or PG_LOC_DEVICE", fn);
    h->form = form;
    PG_HIP_TRY(h, hipSetDevice(h->device));
    const uint8_t *src = static_cast<const uint8_t *>(data);
    if (location == PG_LOC_DEVICE) {
        if (pg_ptr_kind(data, h->device) != PG_PTR_DEVICE)
            return pg_fail(h, PG_ERR_INVALID_ARG, "%s: PG_LOC_DEVICE data is not device memory of device %d", fn, h->device);
        for (uint64_t o = 0; o < n_bytes; o += h->unit)
            if (pg_status s = kf_unit(h, src + o, std::min<uint64_t>(h->unit, n_bytes - o))) return s;
        return PG_OK;
    }
    if (location != PG_LOC_HOST) return pg_fail(h, PG_ERR_INVALID_ARG, "%s: location must be PG_LOC_HOST or PG_LOC_DEVICE", fn);
    // page-locked caller memory goes to the device as it is; anything else through the pinned staging buffers
    const bool pinned = pg_ptr_kind(data, h->device) == PG_PTR_PINNED;
    for (uint64_t o = 0; o < n_bytes; o += h->unit) {
        const uint64_t m = std::min<uint64_t>(h->unit, n_bytes - o);
        const int b = h->next_buf; h->next_buf ^= 1;
        if (!h->dbuf[b].p) {
            PG_HIP_TRY(h, h->dbuf[b].ensure(kUnit));
            PG_HIP_TRY(h, hipEventRecord(h->copied[b], h->cs));
            PG_HIP_TRY(h, hipEventRecord(h->counted[b], h->ks));
        }
        const uint8_t *from = src + o;
        if (!pinned) {
            PG_HIP_TRY(h, h->stage[b].ensure(kUnit));
            PG_HIP_TRY(h, hipEventSynchronize(h->copied[b])); // the staging buffer's previous copy is done
            memcpy(h->stage[b].p, from, m);
            from = h->stage[b].p;
        }
        PG_HIP_TRY(h, hipStreamWaitEvent(h->cs, h->counted[b], 0)); // the device buffer's previous unit is counted
        PG_HIP_TRY(h, hipMemcpyAsync(h->dbuf[b].p, from, m, hipMemcpyHostToDevice, h->cs));
        PG_HIP_TRY(h, hipEventRecord(h->copied[b], h->cs));
        PG_HIP_TRY(h, hipStreamWaitEvent(h->ks, h->copied[b], 0));
        if (pg_status s = kf_unit(h, h->dbuf[b].p, m)) return s;
        PG_HIP_TRY(h, hipEventRecord(h->counted[b], h->ks));
    }
    // the caller may reuse its (page-locked) buffer once submit returns
    if (pinned) PG_HIP_TRY(h, hipStreamSynchronize(h->cs));
    return PG_OK;
}

pg_status pg_kfreq_submit(pg_kfreq *h, const void *data, uint64_t n_bytes, int32_t location) {
    return kf_submit_text(h, data, n_bytes, location, 1, "pg_kfreq_submit");
}

pg_status pg_kfreq_submit_fasta(pg_kfreq *h, const void *data, uint64_t n_bytes, int32_t location) {
    return kf_submit_text(h, data, n_bytes, location, 3, "pg_kfreq_submit_fasta");
}

uint32_t pg_kfreq_reads_piece(const pg_kfreq *h) { return h ? h->piece : 0; }

pg_status pg_kfreq_submit_reads(pg_kfreq *h, const uint8_t *seq_bytes, uint64_t n_seq_bytes, const uint64_t *byte_off, const uint32_t *l_seq,
                                const uint8_t *reverse, uint64_t n_reads, uint32_t flags, int32_t location) {
    if (!h) return pg_fail<pg_kfreq>(nullptr, PG_ERR_INVALID_ARG, "pg_kfreq_submit_reads: null handle");
    if (h->form && h->form != 2) return pg_fail(h, PG_ERR_INVALID_ARG, "pg_kfreq_submit_reads: this stream holds %s (one input form per stream)", kFormName[h->form]);
    if (flags & ~(uint32_t)PG_KFREQ_N_TO_T) return pg_fail(h, PG_ERR_INVALID_ARG, "pg_kfreq_submit_reads: unknown flags 0x%x", flags);
    if (location != PG_LOC_HOST && location != PG_LOC_DEVICE) return pg_fail(h, PG_ERR_INVALID_ARG, "pg_kfreq_submit_reads: location must be PG_LOC_HOST or PG_LOC_DEVICE");
    if (!n_reads) return PG_OK;
    if (n_reads > 0xffffffffull) return pg_fail(h, PG_ERR_INVALID_ARG, "pg_kfreq_submit_reads: %llu reads in one call (at most 2^32 - 1)", (unsigned long long)n_reads);
    if (!byte_off || !l_seq || !reverse || (n_seq_bytes && !seq_bytes)) return pg_fail(h, PG_ERR_INVALID_ARG, "pg_kfreq_submit_reads: null array");
    PG_HIP_TRY(h, hipSetDevice(h->device));
    const bool dev = location == PG_LOC_DEVICE;
    const uint64_t *off = byte_off;
    const uint32_t *len = l_seq;
    if (dev) {
        const void *arrs[4] = {byte_off, l_seq, reverse, seq_bytes};
        for (int i = 0; i < 4; i++)
            if ((i < 3 || n_seq_bytes) && pg_ptr_kind(arrs[i], h->device) != PG_PTR_DEVICE)
                return pg_fail(h, PG_ERR_INVALID_ARG, "pg_kfreq_submit_reads: PG_LOC_DEVICE arrays must be device memory of device %d", h->device);
        h->r_off.resize(n_reads); h->r_len.resize(n_reads);
        PG_HIP_TRY(h, hipMemcpy(h->r_off.data(), byte_off, n_reads * sizeof(uint64_t), hipMemcpyDeviceToHost));
        PG_HIP_TRY(h, hipMemcpy(h->r_len.data(), l_seq, n_reads * sizeof(uint32_t), hipMemcpyDeviceToHost));
        off = h->r_off.data(); len = h->r_len.data();
    }
    // every read inside seq_bytes; the pieces of the reads that hold a window, and where the launches are cut (h->unit windows at most)
    const uint32_t k = h->k, piece = h->piece;
    h->r_work.clear();
    std::vector<std::pair<size_t, uint64_t>> cuts; // (end in r_work, windows) per launch
    uint64_t seg = 0;
    for (uint64_t r = 0; r < n_reads; r++) {
        const uint64_t n = len[r];
        if (n > kMaxReadLen) return pg_fail(h, PG_ERR_INVALID_ARG, "pg_kfreq_submit_reads: read %llu has %llu bases (at most 2^31 - 1)", (unsigned long long)r, (unsigned long long)n);
        if (off[r] > n_seq_bytes || (n + 1) / 2 > n_seq_bytes - off[r])
            return pg_fail(h, PG_ERR_INVALID_ARG, "pg_kfreq_submit_reads: read %llu lies outside seq_bytes", (unsigned long long)r);
        if (n < k) continue;
        const uint64_t n_win = n - k + 1;
        for (uint64_t p = 0; p * piece < n_win; p++) {
            const uint64_t m = std::min<uint64_t>(piece, n_win - p * piece);
            if (seg + m > h->unit) { cuts.emplace_back(h->r_work.size(), seg); seg = 0; }
            h->r_work.push_back(make_uint2((uint32_t)r, (uint32_t)p));
            seg += m;
        }
    }
    h->form = 2;
    if (h->r_work.empty()) return PG_OK;
    cuts.emplace_back(h->r_work.size(), seg);
    // the block: [sequence bytes | offsets | piece list | lengths | flags], each part 16-byte aligned; device input uploads the list alone
    auto up16 = [](uint64_t x) { return (x + 15) & ~15ull; };
    const uint64_t o_off = dev ? 0 : up16(n_seq_bytes), o_work = dev ? 0 : o_off + up16(n_reads * sizeof(uint64_t));
    const uint64_t o_len = o_work + up16(h->r_work.size() * sizeof(uint2)), o_rev = dev ? o_len : o_len + up16(n_reads * sizeof(uint32_t));
    const uint64_t total = dev ? o_len : o_rev + up16(n_reads);
    const int b = h->next_buf; h->next_buf ^= 1;
    PG_HIP_TRY(h, hipEventSynchronize(h->copied[b]));  // the staging block's previous copy is done
    PG_HIP_TRY(h, h->r_stage[b].ensure(total, total + total / 4));
    if (total > h->r_dev[b].cap) PG_HIP_TRY(h, hipEventSynchronize(h->counted[b])); // about to be freed: its last launch is over
    PG_HIP_TRY(h, h->r_dev[b].ensure(total, total + total / 4));
    uint8_t *st = h->r_stage[b].p;
    if (!dev) {
        if (n_seq_bytes) memcpy(st, seq_bytes, n_seq_bytes);
        memcpy(st + o_off, byte_off, n_reads * sizeof(uint64_t));
        memcpy(st + o_len, l_seq, n_reads * sizeof(uint32_t));
        memcpy(st + o_rev, reverse, n_reads);
    }
    memcpy(st + o_work, h->r_work.data(), h->r_work.size() * sizeof(uint2));
    PG_HIP_TRY(h, hipStreamWaitEvent(h->cs, h->counted[b], 0)); // the device block's previous launches are over
    PG_HIP_TRY(h, hipMemcpyAsync(h->r_dev[b].p, st, total, hipMemcpyHostToDevice, h->cs));
    PG_HIP_TRY(h, hipEventRecord(h->copied[b], h->cs));
    PG_HIP_TRY(h, hipStreamWaitEvent(h->ks, h->copied[b], 0));
    const uint8_t *base = h->r_dev[b].p;
    KfReads in{};
    in.seq = dev ? seq_bytes : base; in.n_bytes = n_seq_bytes;
    in.off = dev ? byte_off : reinterpret_cast<const uint64_t *>(base + o_off);
    in.len = dev ? l_seq : reinterpret_cast<const uint32_t *>(base + o_len);
    in.rev = dev ? reverse : base + o_rev;
    in.piece = piece; in.n_to_t = flags & PG_KFREQ_N_TO_T ? 1 : 0;
    const bool al = ((uintptr_t)in.seq & 7) == 0;
    const bool lds = k <= kLdsMaxK;
    const size_t lds_bytes = lds ? (size_t)h->n_codes * sizeof(uint32_t) : 0;
    size_t w0 = 0;
    for (const auto &cut : cuts) {
        if (pg_status s = kf_reserve(h, cut.second)) return s;
        in.work = reinterpret_cast<const uint2 *>(base + o_work) + w0;
        in.n_work = (uint32_t)(cut.first - w0);
        const uint32_t grid = std::min<uint32_t>(kReadBlocks, (in.n_work + kThreads / 64 - 1) / (kThreads / 64));
        if (al && lds) hipLaunchKernelGGL((k_kf_reads<true, true>), dim3(grid), dim3(kThreads), lds_bytes, h->ks, h->d, in, k);
        else if (al) hipLaunchKernelGGL((k_kf_reads<true, false>), dim3(grid), dim3(kThreads), 0, h->ks, h->d, in, k);
        else if (lds) hipLaunchKernelGGL((k_kf_reads<false, true>), dim3(grid), dim3(kThreads), lds_bytes, h->ks, h->d, in, k);
        else hipLaunchKernelGGL((k_kf_reads<false, false>), dim3(grid), dim3(kThreads), 0, h->ks, h->d, in, k);
        PG_HIP_TRY(h, hipGetLastError());
        if (pg_status s = kf_snapshot(h, cut.second)) return s;
        w0 = cut.first;
    }
    PG_HIP_TRY(h, hipEventRecord(h->counted[b], h->ks));
    return PG_OK;
}

pg_status pg_kfreq_sync(pg_kfreq *h) {
    if (!h) return pg_fail<pg_kfreq>(nullptr, PG_ERR_INVALID_ARG, "pg_kfreq_sync: null handle");
    PG_HIP_TRY(h, hipSetDevice(h->device));
    PG_HIP_TRY(h, hipStreamSynchronize(h->cs));
    PG_HIP_TRY(h, hipStreamSynchronize(h->ks));
    return PG_OK;
}

pg_status pg_kfreq_finish(pg_kfreq *h, uint64_t *counts_out, pg_kfreq_result *out) {
    if (!h) return pg_fail<pg_kfreq>(nullptr, PG_ERR_INVALID_ARG, "pg_kfreq_finish: null handle");
    if (!counts_out || !out) return pg_fail(h, PG_ERR_INVALID_ARG, "pg_kfreq_finish: null argument");
    memset(out, 0, sizeof *out);
    if (pg_status s = pg_kfreq_sync(h)) return s;
    uint32_t bad = 0;
    PG_HIP_TRY(h, hipMemcpy(&bad, h->d.err, sizeof bad, hipMemcpyDeviceToHost));
    pg_status st = PG_OK;
    if (bad) st = pg_fail(h, PG_ERR_INPUT, "a sequence line holds a NUL byte (the reference truncates the line there: undefined counts)");
    else if ((st = kf_drain(h)) == PG_OK) {
        PG_HIP_TRY(h, hipMemcpy(counts_out, h->d.hist, (size_t)h->n_codes * sizeof(uint64_t), hipMemcpyDeviceToHost));
        std::vector<std::pair<OddKey, uint64_t>> v(h->odd_map.begin(), h->odd_map.end());
        const uint32_t k = h->k;
        std::sort(v.begin(), v.end(), [k](const auto &a, const auto &b) { return memcmp(a.first.w, b.first.w, k) < 0; });
        h->out_keys.resize(v.size() * k);
        h->out_counts.resize(v.size());
        for (size_t i = 0; i < v.size(); i++) { memcpy(&h->out_keys[i * k], v[i].first.w, k); h->out_counts[i] = v[i].second; }
        out->kmer_size = k;
        out->n_odd = v.size();
        out->odd_keys = h->out_keys.data();
        out->odd_counts = h->out_counts.data();
    }
    if (pg_status s = kf_reset_device(h)) return s;
    return st;
}

} // extern "C"
