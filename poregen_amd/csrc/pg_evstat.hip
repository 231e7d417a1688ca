// pg_evstat.hip -- the event table: level (mean) and spread (sample standard deviation) of every event, in 1e-8 units, exact (pg_evstat.h).
//
// The step from samples to per-event statistics is a segmented reduction over the whole arena of values: events are 5 to 70 values, so
// lanes take the arena, not the events. Kernels:
//   k_ev_stats   a lane loads PG_EV_LANE = 2 values (16 bytes, coalesced), a wave a tile of PG_EV_TILE = 128. The wave looks its first value's
//                event up once (a binary search of samp_off, the same addresses in every lane); the starts of the events that follow are
//                read 64 at a time and marked in a 128-bit mask in LDS, from which a lane takes its head flags, its event (a popcount)
//                and the event's first position (the highest mark at or below it). The three sums (sum d, sum d^2 as two words) are
//                scanned by segment with __shfl_up. The lane at the last value of a segment either finishes its event -- it began and
//                ends in this tile -- or leaves the partial sums in the tile's carry: `head` for the event that came in from the tile in
//                front, `tail` for the one that goes on behind. No wave waits for another.
//   k_ev_carry   one thread per tile: the event that begins in the tile and goes on takes the `head` sums of the tiles behind it (at most
//                PG_EV_MAX_LEN / PG_EV_TILE + 1 of them) and is finished here. An event longer than PG_EV_MAX_LEN is flagged, not summed.
//   k_ev_identity  the layouts in which every event is ONE value (samp_off[i] = i, ev_len[i] = 1): with ev_off unchanged, the existing
//                reduction (pg_launch_slot_model_units) then gives the median and sstdev of a file's means and of its spreads.
// The layout's invariants, which both callers keep and on which the marks rest: samp_off[0] = 0 and strictly increasing (every event holds
// a sample: a ';' closes a value in dump text, a kept window of a context is never empty -- pg_model_events looks), samples 16-byte aligned.
// Refusals (one-sample event, too long, a sample 2^41 units from its event's first, a value outside the fixed-point view) are OR-ed into
// the file's flags with a vector atomicOr; the event's file is looked up only then.
#include <hip/hip_runtime.h>
#include "pg_internal.h"
#include "pg_model.h"
#include "pg_evstat.h"

#include <algorithm>

namespace {

constexpr int kThreads = PG_EV_THREADS;
constexpr uint32_t kTile = PG_EV_TILE;
constexpr uint64_t kNone = ~0ull;
static_assert(PG_EV_LANE == 2 && kTile == 128 && kThreads % 64 == 0, "a lane is one 16-byte load of two values, the head marks of a tile are two 64-bit words");

struct __attribute__((aligned(16))) Carry { uint64_t e; int64_t s1; uint64_t s2_lo, s2_hi; }; // 32 bytes; e = kNone: nothing

template <class S> struct EvArgs {
    const uint64_t *ev_off; uint32_t n_files;
    const uint64_t *samp_off; const S *samples;
    uint64_t cap_events, cap_values;
    int64_t *ev_mean, *ev_sd;
    uint32_t *fflags;
    Carry *head, *tail; // [tiles of cap_values]
};

// the file of event e: the last f with ev_off[f] <= e
__device__ __forceinline__ uint32_t file_of_event(const uint64_t *__restrict__ ev_off, uint32_t n_files, uint64_t e) {
    uint32_t lo = 0, hi = n_files;
    while (hi - lo > 1) { const uint32_t mid = lo + (hi - lo) / 2; if (ev_off[mid] <= e) lo = mid; else hi = mid; }
    return lo;
}
template <class S> __device__ __forceinline__ void refuse(const EvArgs<S> &a, uint64_t e, uint32_t code) {
    if (code && a.n_files) atomicOr(&a.fflags[file_of_event(a.ev_off, a.n_files, e)], code);
}
template <class S> __device__ __forceinline__ int64_t first_units(const EvArgs<S> &a, uint64_t at) { bool bad = false; const int64_t v = sample_units(a.samples[at], bad); return bad ? 0 : v; }

__device__ __forceinline__ uint64_t shfl_up64(uint64_t v, int o) { return (uint64_t)__shfl_up((unsigned long long)v, o, 64); }

// events and values of the batch as the device holds them (the host does not): 0 when they do not fit the buffers (never)
template <class S> __device__ __forceinline__ bool totals(const EvArgs<S> &a, uint64_t &ne, uint64_t &nv) {
    ne = a.ev_off[a.n_files];
    if (ne > a.cap_events) { ne = nv = 0; return false; }
    nv = a.samp_off[ne]; // (samp_off[0] = 0)
    if (nv > a.cap_values) { ne = nv = 0; return false; }
    return true;
}

template <class S> __global__ __launch_bounds__(kThreads) void k_ev_stats(EvArgs<S> a) {
    __shared__ uint32_t marks[kThreads / 64][4];
    const uint32_t lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    uint64_t ne, nv;
    (void)totals(a, ne, nv);
    const uint64_t tile = (uint64_t)blockIdx.x * (kThreads / 64) + w, tile_base = tile * kTile;
    const bool active = tile_base < nv; // the same for the whole wave
    const uint32_t tile_len = active ? (uint32_t)min<uint64_t>(kTile, nv - tile_base) : 0;
    if (lane < 4) marks[w][lane] = 0;
    __syncthreads();
    // the event of the tile's first value: the last e with samp_off[e] <= its index
    uint64_t e_first = 0, start_first = 0;
    if (active) {
        uint64_t lo = 0, hi = ne;
        while (hi - lo > 1) { const uint64_t mid = lo + (hi - lo) / 2; if (a.samp_off[mid] <= tile_base) lo = mid; else hi = mid; }
        e_first = lo; start_first = a.samp_off[lo];
        // an event that begins with the tile is marked like the ones behind it, so that "no mark at or below" means "came in from the tile in front"
        if (start_first == tile_base) { if (lane == 0) atomicOr(&marks[w][0], 1u); e_first--; } // (e_first + marks: modulo 2^64)
        // the events that begin inside the tile, 64 per round
        for (uint32_t r = 0; r < kTile / 64; r++) {
            const uint64_t e = e_first + 1 + r * 64 + lane;
            const uint64_t off = e < ne ? a.samp_off[e] : kNone;
            if (off < tile_base + tile_len) { const uint32_t p = (uint32_t)(off - tile_base); atomicOr(&marks[w][p >> 5], 1u << (p & 31)); }
            if (__shfl(off < tile_base + tile_len ? 1 : 0, 63, 64) == 0) break; // (sorted: the last lane's start lies behind the tile, so do all later ones)
        }
    }
    __syncthreads();
    if (!active) return;
    const uint64_t m_lo = (uint64_t)marks[w][0] | ((uint64_t)marks[w][1] << 32), m_hi = (uint64_t)marks[w][2] | ((uint64_t)marks[w][3] << 32);
    const uint32_t p0 = 2 * lane, p1 = p0 + 1;
    const bool valid0 = p0 < tile_len, valid1 = p1 < tile_len;
    // marks at or below p0: their number is the lane's event, the highest its first position
    uint64_t b_lo, b_hi;
    if (p0 < 64) { b_lo = m_lo & ((2ull << p0) - 1); b_hi = 0; } else { b_lo = m_lo; b_hi = m_hi & ((2ull << (p0 - 64)) - 1); }
    const bool h0 = valid0 && (p0 < 64 ? (m_lo >> p0) & 1 : (m_hi >> (p0 - 64)) & 1);
    const bool h1 = valid1 && (p1 < 64 ? (m_lo >> p1) & 1 : (m_hi >> (p1 - 64)) & 1);
    const uint64_t ev0 = e_first + (uint32_t)__popcll(b_lo) + (uint32_t)__popcll(b_hi), ev1 = ev0 + (h1 ? 1 : 0);
    const uint64_t start0 = b_hi ? tile_base + 64 + (63 - (uint32_t)__clzll(b_hi)) : b_lo ? tile_base + (63 - (uint32_t)__clzll(b_lo)) : start_first;

    // the two values, as units (the batch's last value may stand alone)
    S x0{}, x1{};
    const uint64_t g0 = tile_base + p0;
    if (valid1) {
        const uint4 q = *reinterpret_cast<const uint4 *>(a.samples + g0);
        uint64_t r0 = (uint64_t)q.x | ((uint64_t)q.y << 32), r1 = (uint64_t)q.z | ((uint64_t)q.w << 32);
        static_assert(sizeof(S) == 8, "a value is 8 bytes");
        __builtin_memcpy(&x0, &r0, 8); __builtin_memcpy(&x1, &r1, 8);
    } else if (valid0) x0 = a.samples[g0];
    uint32_t code0 = 0, code1 = 0;
    bool bad0 = false, bad1 = false;
    const int64_t u0 = valid0 ? sample_units(x0, bad0) : 0, u1 = valid1 ? sample_units(x1, bad1) : 0;
    if (bad0) code0 |= PG_EV_BAD_VALUE;
    if (bad1) code1 |= PG_EV_BAD_VALUE;
    int64_t first0 = u0;
    if (valid0 && !h0) { bool b = false; first0 = sample_units(a.samples[start0], b); if (b) first0 = u0; } // (a bad first value is flagged by its own lane)
    const int64_t first1 = h1 ? u1 : first0;
    PgEvSums s0{0, 0, 0}, s1{0, 0, 0};
    if (valid0 && !bad0) pg_ev_add(s0, pg_ev_dev(u0, first0, code0));
    if (valid1 && !bad1) pg_ev_add(s1, pg_ev_dev(u1, first1, code1));
    refuse(a, ev0, code0); refuse(a, ev1, code1);

    // segmented inclusive scan of the lanes' sums: a lane stands for the run that is still open at its end
    PgEvSums agg = s1;
    if (!h1) pg_ev_merge(agg, s0);
    uint32_t fl = (h0 || h1) ? 1u : 0u;
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
        PgEvSums up; up.s1 = (int64_t)shfl_up64((uint64_t)agg.s1, o); up.s2_lo = shfl_up64(agg.s2_lo, o); up.s2_hi = shfl_up64(agg.s2_hi, o);
        const uint32_t fu = (uint32_t)__shfl_up((int)fl, o, 64);
        if ((int)lane >= o) { if (!fl) pg_ev_merge(agg, up); fl |= fu; }
    }
    PgEvSums pre; pre.s1 = (int64_t)shfl_up64((uint64_t)agg.s1, 1); pre.s2_lo = shfl_up64(agg.s2_lo, 1); pre.s2_hi = shfl_up64(agg.s2_hi, 1);
    uint32_t pre_fl = (uint32_t)__shfl_up((int)fl, 1, 64);
    if (lane == 0) { pre = PgEvSums{0, 0, 0}; pre_fl = 0; }
    PgEvSums i0 = s0;
    if (!h0) pg_ev_merge(i0, pre);
    PgEvSums i1 = s1;
    if (!h1) pg_ev_merge(i1, i0);
    const bool open0 = !h0 && !pre_fl, open1 = !h1 && open0; // the run came in from the tile in front
    const bool next_h0 = __shfl_down((int)h0, 1, 64) != 0;
    const bool tail0 = valid0 && (!valid1 || h1), tail1 = valid1 && (p1 + 1 == tile_len || (lane < 63 && next_h0));

    bool is_head = false, is_tail = false; // this lane leaves the tile's head / tail partial
#pragma unroll 1
    for (int k = 0; k < 2; k++) {
        const bool t = k ? tail1 : tail0;
        if (!t) continue;
        const uint32_t p = k ? p1 : p0;
        const uint64_t e = k ? ev1 : ev0;
        const PgEvSums &sum = k ? i1 : i0;
        const bool open = k ? open1 : open0;
        const uint64_t start = k ? (h1 ? tile_base + p1 : start0) : start0;
        // behind the tile's last value the event may go on; everywhere else the next value is a head
        const bool closes = p + 1 < tile_len || a.samp_off[e + 1] == tile_base + p + 1;
        if (!open && closes) {
            int64_t m, sd;
            const uint32_t code = pg_ev_finish(k ? first1 : first0, tile_base + p + 1 - start, sum, m, sd);
            a.ev_mean[e] = m; a.ev_sd[e] = sd;
            refuse(a, e, code);
        } else {
            Carry c; c.e = e; c.s1 = sum.s1; c.s2_lo = sum.s2_lo; c.s2_hi = sum.s2_hi;
            if (open) { a.head[tile] = c; is_head = true; } else { a.tail[tile] = c; is_tail = true; }
        }
    }
    const Carry none{kNone, 0, 0, 0};
    if (!__any(is_head) && lane == 0) a.head[tile] = none;
    if (!__any(is_tail) && lane == 0) a.tail[tile] = none;
}

template <class S> __global__ __launch_bounds__(kThreads) void k_ev_carry(EvArgs<S> a) {
    uint64_t ne, nv;
    (void)totals(a, ne, nv);
    const uint64_t n_tiles = (nv + kTile - 1) / kTile;
    for (uint64_t t = (uint64_t)blockIdx.x * kThreads + threadIdx.x; t < n_tiles; t += (uint64_t)gridDim.x * kThreads) {
        const Carry c = a.tail[t];
        if (c.e == kNone) continue;
        const uint64_t e = c.e, start = a.samp_off[e], n = a.samp_off[e + 1] - start;
        int64_t m = 0, sd = 0;
        uint32_t code = PG_EV_TOO_LONG;
        if (n <= PG_EV_MAX_LEN) {
            PgEvSums s{c.s1, c.s2_lo, c.s2_hi};
            for (uint64_t t2 = t + 1; t2 < n_tiles && t2 <= t + PG_EV_MAX_LEN / kTile + 1; t2++) { // (the event's tiles: it ends in one of these)
                const Carry h = a.head[t2];
                if (h.e != e) break;
                pg_ev_merge(s, PgEvSums{h.s1, h.s2_lo, h.s2_hi});
            }
            code = pg_ev_finish(first_units(a, start), n, s, m, sd);
        }
        a.ev_mean[e] = m; a.ev_sd[e] = sd;
        refuse(a, e, code);
    }
}

__global__ __launch_bounds__(kThreads) void k_ev_identity(uint64_t n, uint64_t *__restrict__ id_off, uint32_t *__restrict__ len1) {
    for (uint64_t i = (uint64_t)blockIdx.x * kThreads + threadIdx.x; i <= n; i += (uint64_t)gridDim.x * kThreads) { id_off[i] = i; if (i < n) len1[i] = 1; }
}

template <class S> hipError_t launch_ev_stats(hipStream_t st, uint32_t n_files, const uint64_t *ev_off, const uint64_t *samp_off, const S *samples, uint64_t cap_events,
                                              uint64_t cap_values, int64_t *ev_mean, int64_t *ev_sd, uint32_t *fflags, void *carry) {
    if (!n_files || !cap_values) return hipSuccess;
    if ((uintptr_t)samples & 15) return hipErrorInvalidValue; // (a lane's two values are one 16-byte load)
    (void)hipGetLastError();
    const uint64_t tiles = pg_ev_tiles(cap_values);
    EvArgs<S> a{ev_off, n_files, samp_off, samples, cap_events, cap_values, ev_mean, ev_sd, fflags, static_cast<Carry *>(carry), static_cast<Carry *>(carry) + tiles};
    const uint32_t blocks = (uint32_t)((tiles + kThreads / 64 - 1) / (kThreads / 64));
    hipLaunchKernelGGL(k_ev_stats<S>, dim3(blocks), dim3(kThreads), 0, st, a);
    hipLaunchKernelGGL(k_ev_carry<S>, dim3((uint32_t)std::min<uint64_t>((tiles + kThreads - 1) / kThreads, 4096)), dim3(kThreads), 0, st, a);
    return hipGetLastError();
}

} // namespace

size_t pg_ev_carry_bytes(uint64_t cap_values) { return 2 * (size_t)pg_ev_tiles(cap_values) * sizeof(Carry); }
hipError_t pg_launch_ev_stats_units(hipStream_t st, uint32_t n_files, const uint64_t *ev_off, const uint64_t *samp_off, const int64_t *units, uint64_t cap_events,
                                    uint64_t cap_values, int64_t *ev_mean, int64_t *ev_sd, uint32_t *fflags, void *carry) {
    return launch_ev_stats<int64_t>(st, n_files, ev_off, samp_off, units, cap_events, cap_values, ev_mean, ev_sd, fflags, carry);
}
hipError_t pg_launch_ev_stats(hipStream_t st, uint32_t n_files, const uint64_t *ev_off, const uint64_t *samp_off, const double *samples, uint64_t cap_events,
                              uint64_t cap_values, int64_t *ev_mean, int64_t *ev_sd, uint32_t *fflags, void *carry) {
    return launch_ev_stats<double>(st, n_files, ev_off, samp_off, samples, cap_events, cap_values, ev_mean, ev_sd, fflags, carry);
}
hipError_t pg_launch_ev_identity(hipStream_t st, uint64_t n, uint64_t *id_off, uint32_t *len1) {
    (void)hipGetLastError();
    hipLaunchKernelGGL(k_ev_identity, dim3((uint32_t)std::min<uint64_t>((n + kThreads) / kThreads, 4096)), dim3(kThreads), 0, st, n, id_off, len1);
    return hipGetLastError();
}
