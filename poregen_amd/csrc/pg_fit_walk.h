// pg_fit_walk.h -- the walk of one piece of a read by one wave, as pg_fit.hip describes it: the device code that `poregen fit`
// (pg_fit.hip) and `poregen eventalign` (pg_evalign.hip) share. Device code only; everything lives in an anonymous namespace, so each
// translation unit that includes it has its own instances. Not installed.
#pragma once
#include <hip/hip_runtime.h>
#include "pg_fit.h"
#include "pg_dev.h"

namespace {

constexpr int kWave = WAVE;
constexpr int kThreads = PG_FIT_THREADS;
constexpr int kWaves = kThreads / kWave;
constexpr uint32_t kPiece = PG_FIT_PIECE;
constexpr uint32_t kUnroll = 4;
typedef unsigned long long u64;
static_assert(PG_FIT_STEP == kWave && sizeof(u64) == 8, "one op per lane");

struct FitBatch {
    const int16_t *sig; const uint64_t *sig_off;
    const uint8_t *seq; const uint64_t *seq_off;
    const uint32_t *op_n; const uint8_t *op_t; const uint64_t *op_off;
    const uint32_t *piece_read, *piece_first; // the read of every piece; the first piece of every read (n_reads + 1)
    const uint64_t *piece_start;              // the first sample of the piece's first op, counted in its read (query_start included)
    const uint64_t *piece_col;                // gapped batches: the reference column in front of the piece's first op
    const uint8_t *part;                      // per read: it takes part in the pass
    const uint32_t *levels;
    const double *ab;                         // pass 2: a and 1 / b of every read
    uint32_t n_reads, n_pieces, k, m, rna, min_dur, max_dur;
};

struct WaveLds { uint32_t cincl[kWave], lvl[kWave]; uint64_t off[kWave]; u64 evd[kWave], evdd[kWave]; };

// LDS written by some lanes of a wave and read by others of the same wave: the wave's LDS operations complete in order, so only the
// compiler has to be kept from moving them across this point
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

struct PieceGeo { uint32_t r, e0, e1, lb, S, col; uint64_t o0, s0, sig0, pos; }; // S, col: gapped walks only (a read that takes part has col <= S < 2^32)
template <bool kGapped = false> __device__ __forceinline__ PieceGeo piece_geo(const FitBatch &B, uint32_t pid, bool with_start) {
    PieceGeo g;
    g.r = B.piece_read[pid];
    g.o0 = B.op_off[g.r];
    g.lb = (uint32_t)(B.op_off[g.r + 1] - g.o0);
    g.e0 = (pid - B.piece_first[g.r]) * kPiece;
    g.e1 = min(g.e0 + kPiece, g.lb);
    g.s0 = B.seq_off[g.r]; g.sig0 = B.sig_off[g.r];
    g.pos = with_start ? B.piece_start[pid] : 0;
    g.S = kGapped ? (uint32_t)(B.seq_off[g.r + 1] - g.s0) : 0u;
    g.col = kGapped && with_start ? (uint32_t)B.piece_col[pid] : 0u;
    return g;
}

// flag: bit 0 an op that is no match, bit 1 an op code above 2. Gapped: pcol gets the piece's reference columns beside its samples.
template <bool kGapped> __global__ __launch_bounds__(kThreads) void k_fit_span(const FitBatch B, uint64_t *__restrict__ psum, uint64_t *__restrict__ pcol, uint32_t *__restrict__ flag) {
    const uint32_t lane = threadIdx.x & (kWave - 1), pid = blockIdx.x * kWaves + threadIdx.x / kWave;
    if (pid >= B.n_pieces) return;                                        // (the whole wave)
    const PieceGeo g = piece_geo(B, pid, false);
    u64 s = 0, c = 0; uint32_t bad = 0;
    for (uint32_t e = g.e0 + lane; e < g.e1; e += kWave) {
        const uint32_t n = B.op_n[g.o0 + e], t = B.op_t[g.o0 + e];
        bad |= t > PG_FIT_OP_D ? 2u : t ? 1u : 0u;
        if (kGapped) { s += pg_fit_op_samples(t, n); c += pg_fit_op_cols(t, n); } else s += n;
    }
    s = wave_sum(s);
    if (kGapped) c = wave_sum(c);
    bad |= __any(bad & 1u) ? 1u : 0u; bad |= __any(bad & 2u) ? 2u : 0u;
    if (bad && lane == 0) atomicOr(flag, bad);
    if (lane == 0) { psum[pid] = s; if (kGapped) pcol[pid] = c; }
}

// One piece by one wave. per_step(counted, start): behind the scans of a step and in front of its samples, in the lane that owns the
// event, start the event's first sample in its read; per_sample(r, l, j): a counted sample with its event's level, j the event's lane;
// per_event(n, code, counted, e, first, start): behind the samples of a step, in the lane that owns the event -- e the op's index in its
// read, first its k-mer's first base in seq. kSamples = false: no sample is read and no LDS touched (per_sample is never called), and a
// piece_geo without its start will do for an all-matches batch.
template <bool kResid, bool kGapped, bool kSamples = true, class PerStep, class PerSample, class PerEvent>
__device__ __forceinline__ void walk_piece(const FitBatch &B, const PieceGeo &g, WaveLds &L, uint32_t lane, PerStep per_step, PerSample per_sample, PerEvent per_event) {
    uint64_t pos = g.pos;
    uint32_t col = g.col;                                                 // gapped: the column in front of the step's first op
    const int16_t *__restrict__ sig = B.sig + g.sig0;
    for (uint32_t es = g.e0; es < g.e1; es += kWave) {                     // (uniform: the scans need every lane)
        const uint32_t e = es + lane;
        const bool valid = e < g.e1;
        const uint32_t n = valid ? B.op_n[g.o0 + e] : 0u;
        uint32_t first = 0, lvl = 0; int32_t code = -1;
        uint64_t incl; bool counted;
        if (kGapped) { // a D takes no samples; a third scan gives the op's column, carried from step to step as pos is
            const uint32_t t = valid ? B.op_t[g.o0 + e] : (uint32_t)PG_FIT_OP_I, cols = pg_fit_op_cols(t, n);
            incl = wave_incl_scan_u64(pg_fit_op_samples(t, n));
            const uint32_t colincl = wave_incl_scan_u32(cols);
            counted = valid && t == PG_FIT_OP_MATCH && pg_fit_dur_ok(n, B.min_dur, B.max_dur) &&
                      pg_fit_gap_kmer_at(B.op_t + g.o0, g.lb, g.S, B.k, B.m, B.rna != 0, e, col + (colincl - cols), first);
            col += (uint32_t)__shfl((int)colincl, kWave - 1, kWave);
        } else {
            incl = wave_incl_scan_u64(n);
            counted = valid && pg_fit_dur_ok(n, B.min_dur, B.max_dur) && pg_fit_kmer_at(g.lb, B.k, B.m, B.rna != 0, e, first);
        }
        if (counted) {
            code = pg_fit_code(B.seq + g.s0, first, B.k);
            lvl = code >= 0 ? B.levels[code] : 0u;
            counted = lvl != 0;
        }
        if (kSamples) {
            const uint32_t cn = counted ? n : 0u;                         // (n <= max_dur <= 2^20: 64 of them fit 32 bits)
            const uint32_t cincl = wave_incl_scan_u32(cn);
            const uint32_t total = (uint32_t)__shfl((int)cincl, kWave - 1, kWave);
            L.cincl[lane] = cincl; L.lvl[lane] = lvl;
            L.off[lane] = pos + (incl - n) - (uint64_t)(cincl - cn);      // virtual index v of this event is sample off + v of the read (read by counted events only: matches)
            if (kResid) { L.evd[lane] = 0; L.evdd[lane] = 0; }
            per_step(counted, pos + (incl - n));
            wave_lds_sync();
            for (uint32_t v0 = lane; v0 < total; v0 += kUnroll * kWave) {  // kUnroll samples per lane and round: their searches and loads are in flight together
                uint32_t ev[kUnroll]; int32_t raw[kUnroll], lev[kUnroll];
#pragma unroll
                for (uint32_t u = 0; u < kUnroll; u++) {
                    const uint32_t v = v0 + u * kWave < total ? v0 + u * kWave : v0; // (behind the end: the lane's first sample again, dropped below)
                    uint32_t j = 0;                                       // the events whose scan value is <= v: the first one behind them holds v
#pragma unroll
                    for (uint32_t s = kWave / 2; s > 0; s >>= 1) if (L.cincl[j + s - 1] <= v) j += s;
                    ev[u] = j; raw[u] = (int32_t)sig[L.off[j] + v]; lev[u] = (int32_t)L.lvl[j];
                }
#pragma unroll
                for (uint32_t u = 0; u < kUnroll; u++) if (v0 + u * kWave < total) per_sample(raw[u], lev[u], ev[u]);
            }
            wave_lds_sync();
        }
        per_event(n, code, counted, e, first, pos + (incl - n));
        pos += __shfl(incl, kWave - 1, kWave);
    }
}

} // namespace
