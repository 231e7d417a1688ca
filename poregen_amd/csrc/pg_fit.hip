// pg_fit.hip -- `poregen fit`: a k-mer model scored against the samples of the basecaller's own segmentation (the rule: pg_fit.h).
//
// A batch is laid out as pg_mvops_expand leaves it: per read Lb ops (the events' lengths), Lb bases, a query_start, and the signal as the
// collector takes it. Events are 5 to 70 samples and reads are ragged, 400 to 10^6 samples, so neither an event nor a read is a unit of
// work. A read is cut into pieces of PG_FIT_PIECE = 256 ops, and a WAVE takes a piece, PG_FIT_STEP = 64 ops at a time:
//   - lane j owns op j of the step: its length (4 bytes), its k-mer (k bytes of seq, the neighbours' bytes again from L1), the level (a
//     table of at most 1 MB). A wave scan of the lengths gives every event's first sample; a second scan, of the COUNTED events' lengths
//     only, lays the counted samples of the step out back to back as virtual indices 0 .. T.
//   - then the lanes take the SAMPLES: lane t takes virtual indices t, t + 64, ...; a six-step binary search over the 64 scan values (in
//     LDS) names the event, from which the sample's address and level follow. Neighbouring lanes read neighbouring samples (2 bytes each,
//     128 bytes per wave load), and a skipped event -- a stall of 10^5 samples -- costs nothing: its samples are never indexed. A lane
//     takes four samples per round, so that four searches and four loads are in flight together (measured: pass 1 0.51 -> 0.44 ms,
//     pass 2 at k = 5 1.58 -> 1.18 ms on the configs[1] shape).
// Kernels:
//   k_fit_span   per piece the sum of its ops' lengths, and a look at op_t: a batch with an op that is no match is refused. The host scans
//                the pieces' sums (one number per 256 ops) into every piece's first sample, and refuses a read whose ops leave its samples
//                before any kernel indexes the signal by them.
// Gapped batches (PG_BATCH_GAPPED: I and D among the ops, seq the reference slices; the rule: pg_fit.h) run the same three kernels as
// their <kGapped = true> instances; the all-matches instances compile to what they were. The span kernel writes a second sum per piece, its
// reference columns; the host scans both and settles ref_length beside out_of_signal. In walk_piece lane j reads op_t, a D takes no
// samples, a third wave scan gives every op's column (carried from step to step as pos is; a read that takes part has fewer than 2^32
// columns), and the clean window costs at most k bytes of op_t per lane. Everything behind `counted` is the same code.
//   k_fit_sums   pass 1: every lane keeps the six sums of its samples in registers; one wave reduction per piece, seven 64-bit integer
//                atomics per piece into the read's sums.
//   k_fit_resid  pass 2: a sample's residual d goes into its event's two sums with LDS atomics (the step's 64 events); behind the step
//                lane j adds event j to its slot -- in a table of the workgroup in LDS for k <= PG_FIT_LDS_K (4^5 slots, 32 KiB, flushed
//                once with global atomics), in global memory above. The grid is bounded (PG_FIT_GRID workgroups whose waves loop over the
//                pieces), so that the flush is paid a thousand times and not once per piece.
// Every sum is an integer and every combination an integer add: the results do not depend on the order. No workgroup waits for another;
// the four waves of a workgroup meet only at the two barriers around the LDS table of pass 2.
#include "../../include/pgmove.h"
#include <hip/hip_runtime.h>
#include "pg_fit.h"
#include "pg_dev.h"
#include "pg_fit_walk.h"
#include "pg_hip_host.h"

#include <cstring>
#include <string>
#include <vector>

static_assert(sizeof(pg_fit_sums) == 56 && sizeof(PgFitSums) == 56, "the sums come back as 56 bytes per read");
static_assert(PG_FIT_ST_OK == PG_FIT_OK && PG_FIT_ST_OUT_OF_SIGNAL == PG_FIT_OUT_OF_SIGNAL && PG_FIT_ST_TOO_LONG == PG_FIT_TOO_LONG && PG_FIT_ST_FEW_EVENTS == PG_FIT_FEW_EVENTS &&
              PG_FIT_ST_FLAT == PG_FIT_FLAT && PG_FIT_ST_NEGATIVE_SCALE == PG_FIT_NEGATIVE_SCALE && PG_FIT_ST_REF_LENGTH == PG_FIT_REF_LENGTH && PG_FIT_ST_SKIPPED == PG_FIT_SKIPPED, "the header's statuses are the rule's");

namespace {

constexpr uint32_t kLdsSlots = 1u << (2 * PG_FIT_LDS_K);           // (the batch, the pieces' geometry, k_fit_span and the walk of a piece: pg_fit_walk.h)

template <bool kGapped> __global__ __launch_bounds__(kThreads) void k_fit_sums(const FitBatch B, u64 *__restrict__ rsums) {
    __shared__ WaveLds lds[kWaves];
    const uint32_t lane = threadIdx.x & (kWave - 1), w = threadIdx.x / kWave, pid = blockIdx.x * kWaves + w;
    if (pid >= B.n_pieces) return;                                        // (the whole wave; this kernel has no workgroup barrier)
    const PieceGeo g = piece_geo<kGapped>(B, pid, true);
    if (!B.part[g.r]) return;
    PgFitSums s{0, 0, 0, 0, 0, 0, 0};
    walk_piece<false, kGapped>(B, g, lds[w], lane, [](bool, uint64_t) {}, [&](int32_t r, int32_t l, uint32_t) { pg_fit_add(s, r, l); },
                               [&](uint32_t, int32_t, bool counted, uint32_t, uint32_t, uint64_t) { s.e += counted ? 1 : 0; });
    const u64 v[7] = {wave_sum((u64)s.n), wave_sum((u64)s.sl), wave_sum((u64)s.sll), wave_sum((u64)s.sr), wave_sum((u64)s.srl), wave_sum((u64)s.srr), wave_sum((u64)s.e)};
    if (lane < 7) { // (two's complement: the signed sums add as unsigned ones)
        const u64 mine = lane == 0 ? v[0] : lane == 1 ? v[1] : lane == 2 ? v[2] : lane == 3 ? v[3] : lane == 4 ? v[4] : lane == 5 ? v[5] : v[6];
        if (mine) atomicAdd(rsums + 7ull * g.r + lane, mine);
    }
}

// tab: n_samples, n_events, sum d, sum d^2 of every slot, four arrays of n_slots; counters[0]: clamped samples
template <bool kLdsTable, bool kGapped> __global__ __launch_bounds__(kThreads) void k_fit_resid(const FitBatch B, u64 *__restrict__ tab, uint32_t n_slots, u64 *__restrict__ counters) {
    __shared__ WaveLds lds[kWaves];
    __shared__ u64 ltab[kLdsTable ? 4 * kLdsSlots : 1];
    const uint32_t lane = threadIdx.x & (kWave - 1), w = threadIdx.x / kWave;
    if (kLdsTable) {
        for (uint32_t i = threadIdx.x; i < 4 * kLdsSlots; i += kThreads) ltab[i] = 0;
        __syncthreads();
    }
    u64 clamped = 0;
    WaveLds &L = lds[w];
    for (uint32_t pid = blockIdx.x * kWaves + w; pid < B.n_pieces; pid += gridDim.x * kWaves) { // (uniform in the wave)
        const PieceGeo g = piece_geo<kGapped>(B, pid, true);
        if (!B.part[g.r]) continue;
        const double a = B.ab[2ull * g.r], inv_b = B.ab[2ull * g.r + 1];
        walk_piece<true, kGapped>(B, g, L, lane, [](bool, uint64_t) {},
            [&](int32_t r, int32_t l, uint32_t j) {
                bool c;
                const int32_t d = pg_fit_resid(r, a, inv_b, l, c);
                clamped += c ? 1 : 0;
                atomicAdd(&L.evd[j], (u64)(int64_t)d);
                atomicAdd(&L.evdd[j], (u64)((int64_t)d * d));
            },
            [&](uint32_t n, int32_t code, bool counted, uint32_t, uint32_t, uint64_t) {
                if (!counted) return;
                const u64 sd = L.evd[lane], sdd = L.evdd[lane];
                u64 *t = kLdsTable ? ltab : tab;
                const uint32_t stride = kLdsTable ? kLdsSlots : n_slots;
                if (n) atomicAdd(t + code, (u64)n);
                atomicAdd(t + stride + code, 1ull);
                if (sd) atomicAdd(t + 2ull * stride + code, sd);
                if (sdd) atomicAdd(t + 3ull * stride + code, sdd);
            });
    }
    clamped = wave_sum(clamped);
    if (lane == 0 && clamped) atomicAdd(counters, clamped);
    if (kLdsTable) {
        __syncthreads();
        for (uint32_t i = threadIdx.x; i < 4 * kLdsSlots; i += kThreads) {
            const uint32_t q = i / kLdsSlots, slot = i % kLdsSlots;
            const u64 v = ltab[i];
            if (v && slot < n_slots) atomicAdd(tab + (uint64_t)q * n_slots + slot, v);
        }
    }
}

// pg_fit_calibrate: the solve of every read and the collector's numbers from it (the rule: pg_fit.h), one lane per read. status comes in
// as the host left it behind pass 1 (ok, out_of_signal, ref_length, a skip code) and goes out final; a too_long read keeps its N and E only,
// as on the host.
struct FitSolveOut { uint32_t *status; double *a, *b, *center, *spread; uint8_t *use; };
__global__ __launch_bounds__(kThreads) void k_fit_solve(uint32_t n_reads, uint32_t min_events, PgFitSums *__restrict__ sums, const double *__restrict__ dig,
                                                        const double *__restrict__ off, const double *__restrict__ range, const FitSolveOut O) {
    const uint32_t r = blockIdx.x * kThreads + threadIdx.x;
    if (r >= n_reads) return;
    uint32_t st = O.status[r];
    double a = 0.0, b = 0.0;
    if (st == PG_FIT_OK) {
        const PgFitSums s = sums[r];
        const PgFitSolve v = pg_fit_solve_hd(s, min_events);
        st = v.status;
        if (st == PG_FIT_TOO_LONG) sums[r] = PgFitSums{s.n, 0, 0, 0, 0, 0, s.e};
        if (st == PG_FIT_OK) { a = v.a; b = v.b; }
    }
    const PgFitScale c = pg_fit_scale_rule(st, a, b, dig[r], off[r], range[r]);
    O.status[r] = st; O.a[r] = a; O.b[r] = b; O.center[r] = c.center; O.spread[r] = c.spread; O.use[r] = c.use;
}

// what a calibration reports of its reads without bringing them back: tally[0 .. 6] reads per status, [7] reads with a skip code, [8] reads
// with use set. One workgroup; its threads stride over the reads.
constexpr uint32_t kTally = 9;
__global__ __launch_bounds__(kThreads) void k_fit_tally(uint32_t n_reads, const uint32_t *__restrict__ status, const uint8_t *__restrict__ use, u64 *__restrict__ tally) {
    __shared__ uint32_t cnt[kTally];
    if (threadIdx.x < kTally) cnt[threadIdx.x] = 0;
    __syncthreads();
    uint32_t mine[kTally] = {0, 0, 0, 0, 0, 0, 0, 0, 0};
    for (uint32_t r = threadIdx.x; r < n_reads; r += kThreads) {
        const uint32_t st = status[r], slot = st < 7u ? st : 7u;
#pragma unroll
        for (uint32_t i = 0; i < 8; i++) mine[i] += slot == i ? 1u : 0u;
        mine[8] += use[r] ? 1u : 0u;
    }
#pragma unroll
    for (uint32_t i = 0; i < kTally; i++)
        if (mine[i]) atomicAdd(&cnt[i], mine[i]);
    __syncthreads();
    if (threadIdx.x < kTally) tally[threadIdx.x] = cnt[threadIdx.x];
}

} // namespace

struct pg_fit {
    int device = 0;
    pg_fit_params prm{};
    PgStream own;
    hipStream_t s = nullptr;
    PgEvent ev[4], ev_solve[2];
    uint32_t k = 0;
    uint64_t n_slots = 0;
    bool dirty = false; // a submit since the last finish
    double ms[2] = {0, 0};
    PgDev<uint32_t> d_levels, d_opn, d_pread, d_pfirst;
    PgDev<int16_t> d_sig;
    PgDev<uint64_t> d_sigoff, d_seqoff, d_opoff, d_pstart, d_psum, d_pcol, d_pcsum; // (d_pcol, d_pcsum: gapped batches)
    PgDev<uint8_t> d_seq, d_opt, d_part;
    PgDev<u64> d_rsums, d_tab, d_counters;
    PgDev<double> d_ab;
    PgDev<uint32_t> d_flag;
    // pg_fit_calibrate: the arrays it hands out, the staged calibration of a host batch
    PgDev<uint32_t> d_status;
    PgDev<double> d_a, d_b, d_center, d_spread, d_dig, d_off, d_range;
    PgDev<uint8_t> d_use;
    PgDev<u64> d_tally;
    std::vector<uint64_t> sig_off, seq_off, op_off, psum, pstart, pcsum, pcol, tab;
    std::vector<int32_t> qs;
    std::vector<uint32_t> piece_read, piece_first, status;
    std::vector<uint8_t> part;
    std::vector<pg_fit_sums> sums;
    std::vector<double> a, b, ab;
    // the run so far, and the arrays a finish hands out
    std::vector<uint64_t> acc_n, acc_e, out_lo, out_hi;
    std::vector<int64_t> acc_d;
    std::vector<unsigned __int128> acc_dd;
    uint64_t reads = 0, fitted = 0, clamped = 0;
    std::string err;
};

extern "C" {

const char *pg_fit_last_error(const pg_fit *h) { return h ? h->err.c_str() : pg_create_error<pg_fit>().c_str(); }

pg_status pg_fit_create(const pg_fit_params *p, int32_t device, pg_fit **out) {
    if (!out || !p) return pg_fail<pg_fit>(nullptr, PG_ERR_INVALID_ARG, "pg_fit_create: null argument");
    *out = nullptr;
    if (p->struct_size != sizeof(pg_fit_params)) return pg_fail<pg_fit>(nullptr, PG_ERR_INVALID_ARG, "pg_fit_create: struct_size %u, this library has %zu", p->struct_size, sizeof(pg_fit_params));
    if (p->min_dur > p->max_dur || p->max_dur > PG_FIT_MAX_DUR) return pg_fail<pg_fit>(nullptr, PG_ERR_INVALID_ARG, "pg_fit_create: min_dur <= max_dur <= %u is required (got %u, %u)", PG_FIT_MAX_DUR, p->min_dur, p->max_dur);
    if (p->sig_move_offset > 64) return pg_fail<pg_fit>(nullptr, PG_ERR_INVALID_ARG, "pg_fit_create: sig_move_offset %u (at most 64)", p->sig_move_offset);
    if (pg_status st = pg_select_device<pg_fit>(device)) return st;
    pg_fit *h = new pg_fit();
    h->device = device; h->prm = *p;
    hipError_t e = hipStreamCreateWithFlags(&h->own.h, hipStreamNonBlocking);
    for (int i = 0; i < 4 && e == hipSuccess; i++) e = hipEventCreate(&h->ev[i].h);
    for (int i = 0; i < 2 && e == hipSuccess; i++) e = hipEventCreate(&h->ev_solve[i].h);
    if (e != hipSuccess) {
        pg_fail(h, PG_ERR_HIP, "pg_fit_create: %s", hipGetErrorString(e));
        return pg_create_failed(h, PG_ERR_HIP, pg_fit_destroy);
    }
    h->s = h->own;
    *out = h;
    return PG_OK;
}

void pg_fit_destroy(pg_fit *h) {
    if (!h) return;
    (void)hipSetDevice(h->device);
    if (h->s) (void)hipStreamSynchronize(h->s);
    delete h;
}

pg_status pg_fit_set_stream(pg_fit *h, void *hip_stream) {
    if (!h) return pg_fail<pg_fit>(nullptr, PG_ERR_INVALID_ARG, "pg_fit_set_stream: null handle");
    PG_HIP_TRY(h, hipSetDevice(h->device));
    PG_HIP_TRY(h, hipStreamSynchronize(h->s));
    h->s = hip_stream ? (hipStream_t)hip_stream : (hipStream_t)h->own;
    return PG_OK;
}

pg_status pg_fit_pass_ms(pg_fit *h, double *one, double *two) {
    if (!h) return pg_fail<pg_fit>(nullptr, PG_ERR_INVALID_ARG, "pg_fit_pass_ms: null handle");
    if (one) *one = h->ms[0];
    if (two) *two = h->ms[1];
    h->ms[0] = h->ms[1] = 0;
    return PG_OK;
}

pg_status pg_fit_set_model(pg_fit *h, const uint32_t *levels, uint32_t k) {
    if (!h) return pg_fail<pg_fit>(nullptr, PG_ERR_INVALID_ARG, "pg_fit_set_model: null handle");
    if (!levels || k < 1 || k > PG_FIT_MAX_K) return pg_fail(h, PG_ERR_INVALID_ARG, "pg_fit_set_model: levels and a kmer_size of 1 to %u are required", PG_FIT_MAX_K);
    if (h->dirty) return pg_fail(h, PG_ERR_STATE, "pg_fit_set_model: reads have been submitted; call pg_fit_finish first");
    const uint64_t ns = 1ull << (2 * k);
    for (uint64_t i = 0; i < ns; i++)
        if (levels[i] >= PG_FIT_MAX_LEVEL) return pg_fail(h, PG_ERR_INVALID_ARG, "pg_fit_set_model: level %u of slot %llu (levels lie below %u)", levels[i], (unsigned long long)i, PG_FIT_MAX_LEVEL);
    PG_HIP_TRY(h, hipSetDevice(h->device));
    PG_HIP_TRY(h, hipStreamSynchronize(h->s));
    PG_HIP_TRY(h, h->d_levels.ensure(ns * sizeof(uint32_t)));
    PG_HIP_TRY(h, h->d_tab.ensure(4 * ns * sizeof(u64)));
    PG_HIP_TRY(h, h->d_counters.ensure(sizeof(u64)));
    PG_HIP_TRY(h, h->d_flag.ensure(sizeof(uint32_t)));
    PG_HIP_TRY(h, hipMemcpyAsync(h->d_levels.p, levels, ns * sizeof(uint32_t), hipMemcpyHostToDevice, h->s));
    PG_HIP_TRY(h, hipStreamSynchronize(h->s));
    h->k = k; h->n_slots = ns;
    h->acc_n.assign(ns, 0); h->acc_e.assign(ns, 0); h->acc_d.assign(ns, 0); h->acc_dd.assign(ns, 0);
    return PG_OK;
}

} // extern "C"

// The tail of pg_fit_calibrate, behind pass 1 on the handle's stream: the statuses the host has settled go up, k_fit_solve and k_fit_tally
// run, and nine counters come back.
static pg_status fit_solve_device(pg_fit *h, const pg_batch *b, uint64_t n, pg_fit_scaling *cal) {
    const hipStream_t s = h->s;
    auto room = [](size_t bytes) { return bytes + bytes / 4 + 256; };
#define CAL_ENSURE(buf, bytes) PG_HIP_TRY(h, (buf).ensure((bytes) ? (bytes) : 1, room(bytes)))
    CAL_ENSURE(h->d_status, n * 4); CAL_ENSURE(h->d_a, n * 8); CAL_ENSURE(h->d_b, n * 8); CAL_ENSURE(h->d_center, n * 8); CAL_ENSURE(h->d_spread, n * 8); CAL_ENSURE(h->d_use, n);
    PG_HIP_TRY(h, h->d_tally.ensure(kTally * sizeof(u64)));
    const double *dig = b->digitisation, *off = b->offset, *range = b->range;
    if (n && b->location == PG_LOC_DEVICE) {
        for (const void *q : {(const void *)dig, (const void *)off, (const void *)range})
            if (pg_ptr_kind(q, h->device) != PG_PTR_DEVICE) return pg_fail(h, PG_ERR_INVALID_ARG, "pg_fit_calibrate: PG_LOC_DEVICE arrays must be device memory of device %d", h->device);
    } else if (n) {
        CAL_ENSURE(h->d_dig, n * 8); CAL_ENSURE(h->d_off, n * 8); CAL_ENSURE(h->d_range, n * 8);
        PG_HIP_TRY(h, hipMemcpyAsync(h->d_dig.p, dig, n * 8, hipMemcpyHostToDevice, s));
        PG_HIP_TRY(h, hipMemcpyAsync(h->d_off.p, off, n * 8, hipMemcpyHostToDevice, s));
        PG_HIP_TRY(h, hipMemcpyAsync(h->d_range.p, range, n * 8, hipMemcpyHostToDevice, s));
        dig = h->d_dig.p; off = h->d_off.p; range = h->d_range.p;
    }
#undef CAL_ENSURE
    u64 tally[kTally] = {0, 0, 0, 0, 0, 0, 0, 0, 0};
    if (n) {
        PG_HIP_TRY(h, hipMemcpyAsync(h->d_status.p, h->status.data(), n * 4, hipMemcpyHostToDevice, s));
        PG_HIP_TRY(h, hipEventRecord(h->ev_solve[0], s));
        const FitSolveOut O{h->d_status.p, h->d_a.p, h->d_b.p, h->d_center.p, h->d_spread.p, h->d_use.p};
        hipLaunchKernelGGL(k_fit_solve, dim3((uint32_t)((n + kThreads - 1) / kThreads)), dim3(kThreads), 0, s, (uint32_t)n, h->prm.min_events, reinterpret_cast<PgFitSums *>(h->d_rsums.p),
                           dig, off, range, O);
        PG_HIP_TRY(h, hipGetLastError());
        hipLaunchKernelGGL(k_fit_tally, dim3(1), dim3(kThreads), 0, s, (uint32_t)n, h->d_status.p, h->d_use.p, h->d_tally.p);
        PG_HIP_TRY(h, hipGetLastError());
        PG_HIP_TRY(h, hipEventRecord(h->ev_solve[1], s));
        PG_HIP_TRY(h, hipMemcpyAsync(tally, h->d_tally.p, sizeof tally, hipMemcpyDeviceToHost, s));
        PG_HIP_TRY(h, hipStreamSynchronize(s));
        float ms = 0; PG_HIP_TRY(h, hipEventElapsedTime(&ms, h->ev_solve[0], h->ev_solve[1])); cal->solve_ms = ms;
    }
    cal->n_reads = n; cal->n_ok = tally[8];
    for (uint32_t i = 0; i < 8; i++) cal->n_status[i] = tally[i];
    cal->d_sums = reinterpret_cast<const pg_fit_sums *>(h->d_rsums.p); cal->d_status = h->d_status.p; cal->d_a = h->d_a.p; cal->d_b = h->d_b.p;
    cal->d_center = h->d_center.p; cal->d_spread = h->d_spread.p; cal->d_use = h->d_use.p;
    return PG_OK;
}

// pg_fit_submit (out) and pg_fit_calibrate (cal): one of the two. Both check the batch, lay out its pieces and run pass 1; the submit then
// solves on the host and runs pass 2, the calibration leaves the sums where they are and solves on the device (k_fit_solve).
#define FIT_FAIL(st, fmt, ...) pg_fail(h, st, "%s: " fmt, who, ##__VA_ARGS__)
static pg_status fit_run(pg_fit *h, const pg_batch *b, const uint32_t *skip, pg_fit_reads *out, pg_fit_scaling *cal) {
    const char *who = cal ? "pg_fit_calibrate" : "pg_fit_submit";
    if (!h->k) return FIT_FAIL(PG_ERR_STATE, "no model (pg_fit_set_model)");
    if (b->struct_size != sizeof(pg_batch)) return FIT_FAIL(PG_ERR_INVALID_ARG, "pg_batch.struct_size %u, this library has %zu", b->struct_size, sizeof(pg_batch));
    if (b->location != PG_LOC_HOST && b->location != PG_LOC_DEVICE) return FIT_FAIL(PG_ERR_INVALID_ARG, "location must be PG_LOC_HOST or PG_LOC_DEVICE");
    const bool gapped = (b->flags & PG_BATCH_GAPPED) != 0;
    if (gapped && (b->flags & PG_BATCH_ALL_MATCHES)) return FIT_FAIL(PG_ERR_INVALID_ARG, "a batch carries PG_BATCH_GAPPED or PG_BATCH_ALL_MATCHES, not both");
    if (!gapped && !(b->flags & PG_BATCH_ALL_MATCHES)) return FIT_FAIL(PG_ERR_INVALID_ARG, "the batch must carry PG_BATCH_ALL_MATCHES (every op a match, as `reform` writes them)");
    const uint64_t n = b->n_reads;
    if (!b->sig_off || !b->seq_off || !b->op_off || (n && !b->query_start)) return FIT_FAIL(PG_ERR_INVALID_ARG, "null array");
    PG_HIP_TRY(h, hipSetDevice(h->device));
    const hipStream_t s = h->s;
    const bool dev = b->location == PG_LOC_DEVICE;
    // the arrays that lay the batch out are looked at on the host: nothing is sized or addressed by an unchecked number
    h->sig_off.resize(n + 1); h->seq_off.resize(n + 1); h->op_off.resize(n + 1); h->qs.resize(n);
    if (dev) {
        const void *must[] = {b->sig_off, b->seq_off, b->op_off, n ? (const void *)b->query_start : nullptr};
        for (const void *q : must)
            if (q && pg_ptr_kind(q, h->device) != PG_PTR_DEVICE) return FIT_FAIL(PG_ERR_INVALID_ARG, "PG_LOC_DEVICE arrays must be device memory of device %d", h->device);
        PG_HIP_TRY(h, hipMemcpyAsync(h->sig_off.data(), b->sig_off, (n + 1) * 8, hipMemcpyDeviceToHost, s));
        PG_HIP_TRY(h, hipMemcpyAsync(h->seq_off.data(), b->seq_off, (n + 1) * 8, hipMemcpyDeviceToHost, s));
        PG_HIP_TRY(h, hipMemcpyAsync(h->op_off.data(), b->op_off, (n + 1) * 8, hipMemcpyDeviceToHost, s));
        if (n) PG_HIP_TRY(h, hipMemcpyAsync(h->qs.data(), b->query_start, n * 4, hipMemcpyDeviceToHost, s));
        PG_HIP_TRY(h, hipStreamSynchronize(s));
    } else {
        memcpy(h->sig_off.data(), b->sig_off, (n + 1) * 8); memcpy(h->seq_off.data(), b->seq_off, (n + 1) * 8); memcpy(h->op_off.data(), b->op_off, (n + 1) * 8);
        if (n) memcpy(h->qs.data(), b->query_start, n * 4);
    }
    h->piece_first.resize(n + 1); h->piece_read.clear();
    for (uint64_t r = 0; r < n; r++) {
        if (h->sig_off[r + 1] < h->sig_off[r] || h->seq_off[r + 1] < h->seq_off[r] || h->op_off[r + 1] < h->op_off[r])
            return FIT_FAIL(PG_ERR_INVALID_ARG, "an offset array decreases at read %llu", (unsigned long long)r);
        const uint64_t lb = h->op_off[r + 1] - h->op_off[r];
        const bool skipped = skip && skip[r];
        if (skipped && skip[r] >= (1u << 16)) return FIT_FAIL(PG_ERR_INVALID_ARG, "skip code %u of read %llu (below 2^16)", skip[r], (unsigned long long)r);
        if (lb > 0x7fffffffull) return FIT_FAIL(PG_ERR_INVALID_ARG, "read %llu has %llu ops (at most 2^31 - 1)", (unsigned long long)r, (unsigned long long)lb);
        if (gapped && h->seq_off[r + 1] - h->seq_off[r] > PG_FIT_MAX_SLICE)
            return FIT_FAIL(PG_ERR_INVALID_ARG, "read %llu has a reference slice of %llu bases (at most 2^32 - 1)", (unsigned long long)r,
                           (unsigned long long)(h->seq_off[r + 1] - h->seq_off[r]));
        if (!gapped && !skipped && h->seq_off[r + 1] - h->seq_off[r] < lb)
            return FIT_FAIL(PG_ERR_INVALID_ARG, "read %llu has %llu ops and %llu bases (an accepted read has as many bases as ops)", (unsigned long long)r,
                           (unsigned long long)lb, (unsigned long long)(h->seq_off[r + 1] - h->seq_off[r]));
        h->piece_first[r] = (uint32_t)h->piece_read.size();
        const uint64_t np = skipped ? 0 : (lb + kPiece - 1) / kPiece;
        if (h->piece_read.size() + np > 0x7fffffffull) return FIT_FAIL(PG_ERR_INVALID_ARG, "batch too large");
        h->piece_read.insert(h->piece_read.end(), np, (uint32_t)r);
    }
    h->piece_first[n] = (uint32_t)h->piece_read.size();
    const size_t n_pieces = h->piece_read.size();
    const uint64_t n_sig = h->sig_off[n], n_seq = h->seq_off[n], n_ops = h->op_off[n];
    if (n_sig - h->sig_off[0] > PG_FIT_BATCH_SAMPLES)
        return FIT_FAIL(PG_ERR_UNSUPPORTED, "%llu samples of signal in one batch (at most 2^28: submit fewer reads at a time)", (unsigned long long)(n_sig - h->sig_off[0]));
    if (dev && b->n_ops && b->n_ops != n_ops) return FIT_FAIL(PG_ERR_INVALID_ARG, "pg_batch.n_ops is %u, op_off ends at %llu", b->n_ops, (unsigned long long)n_ops);
    if ((n_sig && !b->sig) || (n_seq && !b->seq) || (n_ops && (!b->op_n || !b->op_t))) return FIT_FAIL(PG_ERR_INVALID_ARG, "null array");

    FitBatch B{};
    B.n_reads = (uint32_t)n; B.n_pieces = (uint32_t)n_pieces; B.k = h->k; B.m = h->prm.sig_move_offset; B.rna = h->prm.rna ? 1 : 0; B.min_dur = h->prm.min_dur; B.max_dur = h->prm.max_dur;
    B.levels = h->d_levels.p;
    auto room = [](size_t bytes) { return bytes + bytes / 4 + 256; };
#define FIT_ENSURE(buf, bytes) PG_HIP_TRY(h, (buf).ensure((bytes) ? (bytes) : 1, room(bytes)))
    PG_HIP_TRY(h, hipStreamSynchronize(s)); // (nothing queued earlier still reads the buffers about to be refilled or regrown)
    if (dev) {
        const void *must[] = {n_sig ? (const void *)b->sig : nullptr, n_seq ? (const void *)b->seq : nullptr, n_ops ? (const void *)b->op_n : nullptr, n_ops ? (const void *)b->op_t : nullptr};
        for (const void *q : must)
            if (q && pg_ptr_kind(q, h->device) != PG_PTR_DEVICE) return FIT_FAIL(PG_ERR_INVALID_ARG, "PG_LOC_DEVICE arrays must be device memory of device %d", h->device);
        B.sig = b->sig; B.sig_off = b->sig_off; B.seq = b->seq; B.seq_off = b->seq_off; B.op_n = b->op_n; B.op_t = b->op_t; B.op_off = b->op_off;
    } else {
        FIT_ENSURE(h->d_sig, n_sig * 2); FIT_ENSURE(h->d_seq, n_seq); FIT_ENSURE(h->d_opn, n_ops * 4); FIT_ENSURE(h->d_opt, n_ops);
        FIT_ENSURE(h->d_sigoff, (n + 1) * 8); FIT_ENSURE(h->d_seqoff, (n + 1) * 8); FIT_ENSURE(h->d_opoff, (n + 1) * 8);
        if (n_sig) PG_HIP_TRY(h, hipMemcpyAsync(h->d_sig.p, b->sig, n_sig * 2, hipMemcpyHostToDevice, s));
        if (n_seq) PG_HIP_TRY(h, hipMemcpyAsync(h->d_seq.p, b->seq, n_seq, hipMemcpyHostToDevice, s));
        if (n_ops) {
            PG_HIP_TRY(h, hipMemcpyAsync(h->d_opn.p, b->op_n, n_ops * 4, hipMemcpyHostToDevice, s));
            PG_HIP_TRY(h, hipMemcpyAsync(h->d_opt.p, b->op_t, n_ops, hipMemcpyHostToDevice, s));
        }
        PG_HIP_TRY(h, hipMemcpyAsync(h->d_sigoff.p, h->sig_off.data(), (n + 1) * 8, hipMemcpyHostToDevice, s));
        PG_HIP_TRY(h, hipMemcpyAsync(h->d_seqoff.p, h->seq_off.data(), (n + 1) * 8, hipMemcpyHostToDevice, s));
        PG_HIP_TRY(h, hipMemcpyAsync(h->d_opoff.p, h->op_off.data(), (n + 1) * 8, hipMemcpyHostToDevice, s));
        B.sig = h->d_sig.p; B.sig_off = h->d_sigoff.p; B.seq = h->d_seq.p; B.seq_off = h->d_seqoff.p; B.op_n = h->d_opn.p; B.op_t = h->d_opt.p; B.op_off = h->d_opoff.p;
    }
    FIT_ENSURE(h->d_pfirst, (n + 1) * 4); FIT_ENSURE(h->d_pread, n_pieces * 4); FIT_ENSURE(h->d_pstart, n_pieces * 8); FIT_ENSURE(h->d_psum, n_pieces * 8);
    if (gapped) { FIT_ENSURE(h->d_pcol, n_pieces * 8); FIT_ENSURE(h->d_pcsum, n_pieces * 8); }
    FIT_ENSURE(h->d_part, n); FIT_ENSURE(h->d_rsums, n * sizeof(pg_fit_sums)); FIT_ENSURE(h->d_ab, n * 16);
#undef FIT_ENSURE
    B.piece_first = h->d_pfirst.p; B.piece_read = h->d_pread.p; B.piece_start = h->d_pstart.p; B.piece_col = h->d_pcol.p; B.part = h->d_part.p; B.ab = h->d_ab.p;
    const uint32_t blocks = (uint32_t)((n_pieces + kWaves - 1) / kWaves);
    (void)hipGetLastError();

    // ---- the spans of the pieces, and the look at op_t
    h->psum.assign(n_pieces, 0); h->pcsum.assign(gapped ? n_pieces : 0, 0);
    if (n_pieces) {
        uint32_t flag = 0;
        PG_HIP_TRY(h, hipMemcpyAsync(h->d_pfirst.p, h->piece_first.data(), (n + 1) * 4, hipMemcpyHostToDevice, s));
        PG_HIP_TRY(h, hipMemcpyAsync(h->d_pread.p, h->piece_read.data(), n_pieces * 4, hipMemcpyHostToDevice, s));
        PG_HIP_TRY(h, hipMemsetAsync(h->d_flag.p, 0, sizeof(uint32_t), s));
        if (gapped) hipLaunchKernelGGL(k_fit_span<true>, dim3(blocks), dim3(kThreads), 0, s, B, h->d_psum.p, h->d_pcsum.p, h->d_flag.p);
        else hipLaunchKernelGGL(k_fit_span<false>, dim3(blocks), dim3(kThreads), 0, s, B, h->d_psum.p, (uint64_t *)nullptr, h->d_flag.p);
        PG_HIP_TRY(h, hipGetLastError());
        PG_HIP_TRY(h, hipMemcpyAsync(h->psum.data(), h->d_psum.p, n_pieces * 8, hipMemcpyDeviceToHost, s));
        if (gapped) PG_HIP_TRY(h, hipMemcpyAsync(h->pcsum.data(), h->d_pcsum.p, n_pieces * 8, hipMemcpyDeviceToHost, s));
        PG_HIP_TRY(h, hipMemcpyAsync(&flag, h->d_flag.p, sizeof flag, hipMemcpyDeviceToHost, s));
        PG_HIP_TRY(h, hipStreamSynchronize(s));
        if (gapped && (flag & 2u)) return FIT_FAIL(PG_ERR_INVALID_ARG, "the batch carries PG_BATCH_GAPPED but holds an op code above 2 (0 match, 1 I, 2 D)");
        if (!gapped && flag) return FIT_FAIL(PG_ERR_INVALID_ARG, "the batch carries PG_BATCH_ALL_MATCHES but holds an op that is no match (an I, a D or an unknown op)");
    }
    // ---- every piece's first sample (gapped: and first column); a read whose ops leave its samples takes no part, nor does a gapped read
    // whose slice has not as many bases as its ops have columns: no kernel reads its seq
    h->status.assign(n, PG_FIT_ST_OK); h->part.assign(n, 0); h->pstart.resize(n_pieces); h->pcol.resize(gapped ? n_pieces : 0);
    for (uint64_t r = 0; r < n; r++) {
        if (skip && skip[r]) { h->status[r] = PG_FIT_ST_SKIPPED + skip[r]; continue; }
        const uint64_t len = h->sig_off[r + 1] - h->sig_off[r];
        uint64_t at = h->qs[r] < 0 ? 0 : (uint64_t)h->qs[r];
        uint64_t col = 0;
        for (uint32_t p = h->piece_first[r]; p < h->piece_first[r + 1]; p++) {
            h->pstart[p] = at; at += h->psum[p];
            if (gapped) { h->pcol[p] = col; col += h->pcsum[p]; }
        }
        if (h->qs[r] < 0 || at > len) h->status[r] = PG_FIT_ST_OUT_OF_SIGNAL;
        else if (gapped && col != h->seq_off[r + 1] - h->seq_off[r]) h->status[r] = PG_FIT_ST_REF_LENGTH;
        else h->part[r] = 1;
    }
    // ---- pass 1
    h->sums.assign(n, pg_fit_sums{0, 0, 0, 0, 0, 0, 0});
    if (n_pieces) {
        PG_HIP_TRY(h, hipMemcpyAsync(h->d_pstart.p, h->pstart.data(), n_pieces * 8, hipMemcpyHostToDevice, s));
        if (gapped) PG_HIP_TRY(h, hipMemcpyAsync(h->d_pcol.p, h->pcol.data(), n_pieces * 8, hipMemcpyHostToDevice, s));
        PG_HIP_TRY(h, hipMemcpyAsync(h->d_part.p, h->part.data(), n, hipMemcpyHostToDevice, s));
        PG_HIP_TRY(h, hipMemsetAsync(h->d_rsums.p, 0, n * sizeof(pg_fit_sums), s));
        PG_HIP_TRY(h, hipEventRecord(h->ev[0], s));
        if (gapped) hipLaunchKernelGGL(k_fit_sums<true>, dim3(blocks), dim3(kThreads), 0, s, B, h->d_rsums.p);
        else hipLaunchKernelGGL(k_fit_sums<false>, dim3(blocks), dim3(kThreads), 0, s, B, h->d_rsums.p);
        PG_HIP_TRY(h, hipGetLastError());
        PG_HIP_TRY(h, hipEventRecord(h->ev[1], s));
        if (!cal) {
            PG_HIP_TRY(h, hipMemcpyAsync(h->sums.data(), h->d_rsums.p, n * sizeof(pg_fit_sums), hipMemcpyDeviceToHost, s));
            PG_HIP_TRY(h, hipStreamSynchronize(s));
            float ms = 0; PG_HIP_TRY(h, hipEventElapsedTime(&ms, h->ev[0], h->ev[1])); h->ms[0] += ms;
        }
    } else if (cal && n) PG_HIP_TRY(h, hipMemsetAsync(h->d_rsums.p, 0, n * sizeof(pg_fit_sums), s));
    if (cal) return fit_solve_device(h, b, n, cal);
    // ---- the solve
    h->a.assign(n, 0.0); h->b.assign(n, 0.0); h->ab.assign(2 * n, 0.0);
    uint64_t fitted = 0;
    for (uint64_t r = 0; r < n; r++) {
        h->part[r] = 0;
        if (h->status[r] != PG_FIT_ST_OK) continue;
        const pg_fit_sums &q = h->sums[r];
        const PgFitSolve sv = pg_fit_solve(PgFitSums{q.n, q.sl, q.sll, q.sr, q.srl, q.srr, q.e}, h->prm.min_events);
        h->status[r] = sv.status;
        if (sv.status == PG_FIT_TOO_LONG) h->sums[r] = pg_fit_sums{q.n, 0, 0, 0, 0, 0, q.e};
        if (sv.status != PG_FIT_OK) continue;
        h->a[r] = sv.a; h->b[r] = sv.b; h->ab[2 * r] = sv.a; h->ab[2 * r + 1] = sv.inv_b; h->part[r] = 1;
        fitted++;
    }
    // ---- pass 2
    if (fitted) {
        h->tab.resize(4 * h->n_slots);
        u64 clamped = 0;
        PG_HIP_TRY(h, hipMemcpyAsync(h->d_part.p, h->part.data(), n, hipMemcpyHostToDevice, s));
        PG_HIP_TRY(h, hipMemcpyAsync(h->d_ab.p, h->ab.data(), n * 16, hipMemcpyHostToDevice, s));
        PG_HIP_TRY(h, hipMemsetAsync(h->d_tab.p, 0, 4 * h->n_slots * sizeof(u64), s));
        PG_HIP_TRY(h, hipMemsetAsync(h->d_counters.p, 0, sizeof(u64), s));
        const uint32_t grid = blocks < PG_FIT_GRID ? blocks : PG_FIT_GRID;
        PG_HIP_TRY(h, hipEventRecord(h->ev[2], s));
        const bool lds_tab = h->k <= PG_FIT_LDS_K;
        if (lds_tab && !gapped) hipLaunchKernelGGL((k_fit_resid<true, false>), dim3(grid), dim3(kThreads), 0, s, B, h->d_tab.p, (uint32_t)h->n_slots, h->d_counters.p);
        else if (!gapped) hipLaunchKernelGGL((k_fit_resid<false, false>), dim3(grid), dim3(kThreads), 0, s, B, h->d_tab.p, (uint32_t)h->n_slots, h->d_counters.p);
        else if (lds_tab) hipLaunchKernelGGL((k_fit_resid<true, true>), dim3(grid), dim3(kThreads), 0, s, B, h->d_tab.p, (uint32_t)h->n_slots, h->d_counters.p);
        else hipLaunchKernelGGL((k_fit_resid<false, true>), dim3(grid), dim3(kThreads), 0, s, B, h->d_tab.p, (uint32_t)h->n_slots, h->d_counters.p);
        PG_HIP_TRY(h, hipGetLastError());
        PG_HIP_TRY(h, hipEventRecord(h->ev[3], s));
        PG_HIP_TRY(h, hipMemcpyAsync(h->tab.data(), h->d_tab.p, 4 * h->n_slots * sizeof(u64), hipMemcpyDeviceToHost, s));
        PG_HIP_TRY(h, hipMemcpyAsync(&clamped, h->d_counters.p, sizeof clamped, hipMemcpyDeviceToHost, s));
        PG_HIP_TRY(h, hipStreamSynchronize(s));
        float ms = 0; PG_HIP_TRY(h, hipEventElapsedTime(&ms, h->ev[2], h->ev[3])); h->ms[1] += ms;
        const uint64_t ns = h->n_slots;
        for (uint64_t i = 0; i < ns; i++) {
            h->acc_n[i] += h->tab[i]; h->acc_e[i] += h->tab[ns + i]; h->acc_d[i] += (int64_t)h->tab[2 * ns + i]; h->acc_dd[i] += h->tab[3 * ns + i];
        }
        h->clamped += clamped;
    }
    h->reads += n; h->fitted += fitted; h->dirty = true;
    out->n_reads = n; out->sums = h->sums.data(); out->status = h->status.data(); out->a = h->a.data(); out->b = h->b.data();
    return PG_OK;
}
#undef FIT_FAIL

extern "C" {

pg_status pg_fit_submit(pg_fit *h, const pg_batch *b, const uint32_t *skip, pg_fit_reads *out) {
    if (!h) return pg_fail<pg_fit>(nullptr, PG_ERR_INVALID_ARG, "pg_fit_submit: null handle");
    if (!b || !out) return pg_fail(h, PG_ERR_INVALID_ARG, "pg_fit_submit: null argument");
    memset(out, 0, sizeof *out);
    return fit_run(h, b, skip, out, nullptr);
}

pg_status pg_fit_calibrate(pg_fit *h, const pg_batch *b, const uint32_t *skip, pg_fit_scaling *out) {
    if (!h) return pg_fail<pg_fit>(nullptr, PG_ERR_INVALID_ARG, "pg_fit_calibrate: null handle");
    if (!b || !out) return pg_fail(h, PG_ERR_INVALID_ARG, "pg_fit_calibrate: null argument");
    memset(out, 0, sizeof *out);
    if (b->struct_size == sizeof(pg_batch) && b->n_reads && (!b->digitisation || !b->offset || !b->range))
        return pg_fail(h, PG_ERR_INVALID_ARG, "pg_fit_calibrate: digitisation, offset and range are required");
    return fit_run(h, b, skip, nullptr, out);
}

pg_status pg_fit_finish(pg_fit *h, pg_fit_result *out) {
    if (!h) return pg_fail<pg_fit>(nullptr, PG_ERR_INVALID_ARG, "pg_fit_finish: null handle");
    if (!out) return pg_fail(h, PG_ERR_INVALID_ARG, "pg_fit_finish: null argument");
    memset(out, 0, sizeof *out);
    if (!h->k) return pg_fail(h, PG_ERR_STATE, "pg_fit_finish: no model (pg_fit_set_model)");
    const uint64_t ns = h->n_slots;
    // the arrays handed out are copies: the accumulators start the next run at zero
    h->tab.assign(3 * ns, 0); h->out_lo.assign(ns, 0); h->out_hi.assign(ns, 0);
    uint64_t events = 0, samples = 0;
    for (uint64_t i = 0; i < ns; i++) {
        h->tab[i] = h->acc_n[i]; h->tab[ns + i] = h->acc_e[i]; h->tab[2 * ns + i] = (uint64_t)h->acc_d[i];
        h->out_lo[i] = (uint64_t)h->acc_dd[i]; h->out_hi[i] = (uint64_t)(h->acc_dd[i] >> 64);
        samples += h->acc_n[i]; events += h->acc_e[i];
    }
    out->kmer_size = h->k; out->n_slots = ns;
    out->n_samples = h->tab.data(); out->n_events = h->tab.data() + ns; out->sum_d = reinterpret_cast<const int64_t *>(h->tab.data() + 2 * ns);
    out->sum_dd_lo = h->out_lo.data(); out->sum_dd_hi = h->out_hi.data();
    out->reads = h->reads; out->fitted = h->fitted; out->events = events; out->samples = samples; out->clamped = h->clamped;
    h->acc_n.assign(ns, 0); h->acc_e.assign(ns, 0); h->acc_d.assign(ns, 0); h->acc_dd.assign(ns, 0);
    h->reads = h->fitted = h->clamped = 0; h->dirty = false;
    return PG_OK;
}

pg_status pg_fit_parse_model(const char *text, size_t n, uint32_t want_k, uint32_t *k_out, uint32_t *levels_out, size_t cap_slots, int32_t *uses_u, char *err, size_t err_cap) {
    auto say = [&](const std::string &m) { if (err && err_cap) snprintf(err, err_cap, "%s", m.c_str()); };
    if (err && err_cap) err[0] = 0;
    if ((!text && n) || !k_out || !levels_out) { say("null argument"); return PG_ERR_INVALID_ARG; }
    if (want_k > PG_FIT_MAX_K) { say("a k-mer has 1 to 9 letters"); return PG_ERR_INVALID_ARG; }
    PgFitModel md; std::string why;
    if (!pg_fit_parse_model_text(text, n, want_k, md, why)) { say(why); return PG_ERR_INPUT; }
    if (md.levels.size() > cap_slots) { say("levels_out is too small for the model's k"); return PG_ERR_INVALID_ARG; }
    memcpy(levels_out, md.levels.data(), md.levels.size() * sizeof(uint32_t));
    *k_out = md.k;
    if (uses_u) *uses_u = md.uses_u ? 1 : 0;
    return PG_OK;
}

pg_status pg_fit_residuals(uint64_t n, int64_t sum_d, uint64_t dd_lo, uint64_t dd_hi, int64_t *mean, int64_t *rms) {
    if (!n || !mean || !rms || (((unsigned __int128)dd_hi << 64) | dd_lo) > ((unsigned __int128)n << 36)) return PG_ERR_INVALID_ARG; // (d^2 < 2^36 for every sample)
    pg_fit_slot_resid(n, sum_d, dd_lo, dd_hi, *mean, *rms);
    return PG_OK;
}

} // extern "C"
