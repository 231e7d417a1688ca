// pg_sim.hip -- `poregen simulate`: raw signal and its true alignment drawn from a k-mer model (the rule: pg_sim.h).
//
// The unit of work is fit's: a read is cut into pieces of PG_SIM_PIECE = 256 ops, a WAVE takes a piece, a workgroup is four waves.
//   k_sim_ops    lane j owns op j of a step of 64: it packs the op's k-mer from the sequence bytes, looks the slot up and draws the dwell
//                (one Philox block, stream 1). Per op the dwell and the slot, per piece the samples and what refuses the read (a letter
//                outside ACGTU, a k-mer without a level). The host reads the pieces' sums back, decides every read's status and scans:
//                every piece's first sample and first op in the result, sig_off, op_off and the total, which sizes the signal.
//   k_sim_emit   one piece of an accepted read by one wave: the starts of its 256 events by DPP wave scans into the wave's LDS together
//                with every event's level and stdv; then the piece's samples IN ORDER. A lane owns PG_SIM_LANE = 8 consecutive samples:
//                it finds the event of the first by binary search over the starts and steps on from there, draws one Philox block per
//                sample (stream 2) and stores 16 bytes at a 16-byte aligned address; the samples in front of the first aligned address
//                and behind the last are stored one per lane. The lead of a read is written by its first piece. The tables are read
//                from global memory (3 MiB at k = 9: they live in L2).
// No atomics, no wave waits for another, the four waves of a workgroup never meet; the inner loop is integer only and holds no 64-bit
// division. Every value is addressed by (read, stream, index): the result does not depend on the order of execution or on the batching.
#include "../../include/pgmove.h"
#include <hip/hip_runtime.h>
#include "pg_sim.h"
#include "pg_dev.h"
#include "pg_hip_host.h"

#include <cstring>
#include <string>
#include <vector>

static_assert(sizeof(pg_sim_params) == 64, "pg_sim_params is 64 bytes");
static_assert(PG_SIM_ST_TOO_SHORT == PG_SIM_TOO_SHORT && PG_SIM_ST_BAD_BASE == PG_SIM_BAD_BASE && PG_SIM_ST_NO_LEVEL == PG_SIM_NO_LEVEL, "the statuses of pgmove.h are the rule's");

namespace {

constexpr int kWave = WAVE;
constexpr int kThreads = PG_SIM_THREADS;
constexpr int kWaves = kThreads / kWave;
constexpr uint32_t kPiece = PG_SIM_PIECE;
constexpr uint32_t kSteps = kPiece / kWave;
constexpr uint32_t kLane = PG_SIM_LANE;
constexpr uint32_t kVec = 8;              // samples of one 16-byte store
static_assert(kSteps * kWave == kPiece && (kLane == 8 || kLane == 16), "four steps of one op per lane; a lane's samples are one or two 16-byte stores");

struct SimBatch {
    const uint8_t *seq; const uint64_t *seq_off;
    const uint32_t *piece_read, *piece_first; // the read of every piece; the first piece of every read (n_reads + 1)
    const uint32_t *levels, *stdvs, *dwells;
    uint64_t seed, first_read; int64_t Q;
    uint32_t n_reads, n_pieces, k, m, rna, spread_pct, lead, lead_level, lead_stdv;
};
struct SimPlace {                             // where an accepted read's pieces go, from the host's scan
    const uint8_t *ok;                        // per read: accepted
    const int32_t *off_r;                     // per read
    const uint64_t *piece_sig;                // the piece's first sample in the signal buffer (the first piece of a read: its lead's)
    const uint32_t *piece_j0;                 // ... counted in its read
    const uint64_t *piece_op;                 // the piece's first op in the result's op_n
};

struct SimLds {
    uint32_t start[kPiece + 1];               // the first sample of every event, counted in the piece; [ops of the piece ..] = the piece's samples
    uint32_t lvl[kPiece], sd[kPiece];
};

// LDS written by some lanes of a wave and read by others of the same wave (as in pg_fit.hip)
__device__ __forceinline__ void wave_lds_sync() {
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}
__device__ __forceinline__ uint32_t uni(uint32_t v) { return (uint32_t)__builtin_amdgcn_readfirstlane((int)v); }
__device__ __forceinline__ uint64_t uni64(uint64_t v) { return (uint64_t)uni((uint32_t)v) | ((uint64_t)uni((uint32_t)(v >> 32)) << 32); }

struct SimGeo { uint32_t r, e0, cnt, lb; uint64_t s0; };
__device__ __forceinline__ SimGeo sim_geo(const SimBatch &B, uint32_t pid) {
    SimGeo g;
    g.r = uni(B.piece_read[pid]);
    g.s0 = uni64(B.seq_off[g.r]);
    g.lb = (uint32_t)(uni64(B.seq_off[g.r + 1]) - g.s0);
    g.e0 = (pid - uni(B.piece_first[g.r])) * kPiece;
    g.cnt = min(kPiece, g.lb - g.e0);
    return g;
}

// tmp_n, tmp_slot: indexed as the sequence bytes are (op e of read r at seq_off[r] + e)
__global__ __launch_bounds__(kThreads) void k_sim_ops(const SimBatch B, uint32_t *__restrict__ tmp_n, uint32_t *__restrict__ tmp_slot, uint32_t *__restrict__ psum,
                                                     uint32_t *__restrict__ pflag) {
    const uint32_t lane = threadIdx.x & (kWave - 1), pid = uni(blockIdx.x * kWaves + threadIdx.x / kWave);
    if (pid >= B.n_pieces) return;                                        // (the whole wave)
    const SimGeo g = sim_geo(B, pid);
    const uint8_t *__restrict__ seq = B.seq + g.s0;
    const uint64_t read = B.first_read + g.r;
    uint32_t sum = 0, flag = 0;
    for (uint32_t i = lane; i < g.cnt; i += kWave) {
        const uint32_t e = g.e0 + i;
        if (pg_sim_base(seq[e]) < 0) flag |= PG_SIM_FLAG_BAD_BASE;        // every base of the read is some op's own
        const int32_t code = pg_sim_code(seq, pg_sim_kmer_first(g.lb, B.k, B.m, B.rna != 0, e), B.k);
        uint32_t n = 0, slot = 0;
        if (code < 0) flag |= PG_SIM_FLAG_BAD_BASE;
        else if (!B.levels[code]) flag |= PG_SIM_FLAG_NO_LEVEL;
        else { slot = (uint32_t)code; n = pg_sim_dwell(B.seed, read, e, B.dwells[code], B.spread_pct); }
        tmp_n[g.s0 + e] = n; tmp_slot[g.s0 + e] = slot;
        sum += n;
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) { sum += __shfl_xor(sum, o, kWave); flag |= __shfl_xor(flag, o, kWave); }
    if (lane == 0) { psum[pid] = sum; pflag[pid] = flag; }
}

__global__ __launch_bounds__(kThreads) void k_sim_emit(const SimBatch B, const SimPlace P, const uint32_t *__restrict__ tmp_n, const uint32_t *__restrict__ tmp_slot,
                                                      int16_t *__restrict__ sig, uint32_t *__restrict__ op_n) {
    __shared__ SimLds lds[kWaves];
    const uint32_t lane = threadIdx.x & (kWave - 1), w = threadIdx.x / kWave, pid = uni(blockIdx.x * kWaves + w);
    if (pid >= B.n_pieces) return;                                        // (the whole wave; this kernel has no workgroup barrier)
    const SimGeo g = sim_geo(B, pid);
    if (!P.ok[g.r]) return;                                               // a refused read has no ops and no samples
    SimLds &L = lds[w];
    const uint64_t read = B.first_read + g.r;
    const int32_t off_r = (int32_t)uni((uint32_t)P.off_r[g.r]);
    const uint32_t lead0 = g.e0 == 0 ? B.lead : 0u, j0 = uni(P.piece_j0[pid]);
    const uint64_t base = uni64(P.piece_sig[pid]);
    uint32_t *__restrict__ out_n = op_n + uni64(P.piece_op[pid]);

    // ---- the starts of the piece's events, their levels and stdvs
    uint32_t pos = lead0;
#pragma unroll
    for (uint32_t st = 0; st < kSteps; st++) {
        const uint32_t i = st * kWave + lane;
        const bool valid = i < g.cnt;
        const uint32_t n = valid ? tmp_n[g.s0 + g.e0 + i] : 0u, slot = valid ? tmp_slot[g.s0 + g.e0 + i] : 0u;
        const uint32_t incl = wave_incl_scan_u32(n);
        L.start[i] = pos + (incl - n); L.lvl[i] = valid ? B.levels[slot] : 0u; L.sd[i] = valid ? B.stdvs[slot] : 0u;
        if (valid) out_n[i] = n;
        pos += (uint32_t)__shfl((int)incl, kWave - 1, kWave);
    }
    const uint32_t total = pos;                                           // the piece's samples, its read's lead included (uniform)
    if (lane == 0) L.start[kPiece] = total;
    wave_lds_sync();

    // the event of sample t >= lead0 of the piece: the last one that starts at or in front of t
    auto find = [&](uint32_t t) {
        uint32_t lo = 0, hi = kPiece;
#pragma unroll
        for (uint32_t s = 0; s < 8; s++) { const uint32_t mid = (lo + hi) >> 1; if (L.start[mid] <= t) lo = mid; else hi = mid; }
        return lo;
    };
    auto one = [&](uint32_t t, uint32_t ev) {                             // ev: the event of t (not read for a sample of the lead)
        const bool in_lead = t < lead0;
        const int32_t l = (int32_t)(in_lead ? B.lead_level : L.lvl[ev]), s = (int32_t)(in_lead ? B.lead_stdv : L.sd[ev]);
        return pg_sim_sample(B.seed, read, j0 + t, l, s, B.Q, off_r);
    };
    // ---- the samples in front of the first 16-byte aligned address, one per lane (fewer than 8)
    const uint32_t head = min(total, (uint32_t)((kVec - (base & (kVec - 1))) & (kVec - 1)));
    if (lane < head) sig[base + lane] = (int16_t)one(lane, lane < lead0 ? 0u : find(lane));
    // ---- kLane samples per lane, 512 (or 1024) per wave and round
    const uint32_t n_vec = (total - head) / kLane;
    for (uint32_t v = lane; v < n_vec; v += kWave) {
        const uint32_t t0 = head + v * kLane;
        uint32_t ev = t0 < lead0 ? 0u : find(t0);
        uint32_t q[kLane / 2];
#pragma unroll
        for (uint32_t u = 0; u < kLane; u++) {
            const uint32_t t = t0 + u;
            if (t >= lead0) while (L.start[ev + 1] <= t) ev++;           // (start[256] = total > t ends it)
            const uint32_t x = (uint32_t)one(t, ev) & 0xffffu;
            if (u & 1u) q[u >> 1] |= x << 16; else q[u >> 1] = x;
        }
#pragma unroll
        for (uint32_t c = 0; c < kLane / kVec; c++) *reinterpret_cast<uint4 *>(sig + base + t0 + c * kVec) = make_uint4(q[4 * c], q[4 * c + 1], q[4 * c + 2], q[4 * c + 3]);
    }
    // ---- the samples behind the last whole vector (fewer than kLane), one per lane
    const uint32_t t = head + n_vec * kLane + lane;
    if (t < total) sig[base + t] = (int16_t)one(t, t < lead0 ? 0u : find(t));
}

} // namespace

struct pg_sim {
    int device = 0;
    pg_sim_params prm{};
    uint64_t Q = 0;
    PgStream own;
    hipStream_t s = nullptr;
    PgEvent ev[3];
    uint32_t k = 0;
    double ops_ms = 0, emit_ms = 0;
    PgDev<uint32_t> d_levels, d_stdvs, d_dwells, d_pread, d_pfirst, d_tmpn, d_tmpslot, d_psum, d_pflag, d_pj0, d_opn, d_status;
    PgDev<uint64_t> d_seqoff, d_psig, d_pop, d_sigoff, d_opoff;
    PgDev<uint8_t> d_seq, d_ok, d_opt;
    PgDev<int32_t> d_offr, d_qs, d_t0, d_t1;
    PgDev<double> d_dig, d_off, d_range;
    PgDev<int16_t> d_sig;
    std::vector<uint64_t> seq_off, sig_off, op_off, psig, pop;
    std::vector<uint32_t> piece_read, piece_first, psum, pflag, pj0, status;
    std::vector<uint8_t> ok;
    std::vector<int32_t> offr, qs, t0, t1;
    std::vector<double> dig, off, range;
    std::string err;
};

static pg_status sim_check_params(pg_sim *h, const pg_sim_params *p, const char *who) {
    if (p->struct_size != sizeof(pg_sim_params)) return pg_fail(h, PG_ERR_INVALID_ARG, "%s: struct_size %u, this library has %zu", who, p->struct_size, sizeof(pg_sim_params));
    if (const char *why = pg_sim_rule_error(p->kmer_size, p->sig_move_offset, p->digitisation, p->range_e4, p->offset, p->off_spread, p->spread_pct, p->lead, p->lead_level, p->lead_stdv))
        return pg_fail(h, PG_ERR_INVALID_ARG, "%s: %s", who, why);
    return PG_OK;
}
static PgSimRule sim_rule(const pg_sim_params *p) {
    return PgSimRule{p->kmer_size, p->sig_move_offset, p->rna != 0, p->seed, pg_sim_q(p->digitisation, p->range_e4), p->offset, p->off_spread, p->spread_pct, p->lead, p->lead_level,
                     p->lead_stdv};
}

extern "C" {

const char *pg_sim_last_error(const pg_sim *h) { return h ? h->err.c_str() : pg_create_error<pg_sim>().c_str(); }

pg_status pg_sim_create(const pg_sim_params *p, int32_t device, pg_sim **out) {
    if (!out || !p) return pg_fail<pg_sim>(nullptr, PG_ERR_INVALID_ARG, "pg_sim_create: null argument");
    *out = nullptr;
    if (pg_status st = sim_check_params(nullptr, p, "pg_sim_create")) return st;
    if (pg_status st = pg_select_device<pg_sim>(device)) return st;
    pg_sim *h = new pg_sim();
    h->device = device; h->prm = *p; h->Q = pg_sim_q(p->digitisation, p->range_e4);
    hipError_t e = hipStreamCreateWithFlags(&h->own.h, hipStreamNonBlocking);
    for (int i = 0; i < 3 && e == hipSuccess; i++) e = hipEventCreate(&h->ev[i].h);
    if (e != hipSuccess) {
        pg_fail(h, PG_ERR_HIP, "pg_sim_create: %s", hipGetErrorString(e));
        return pg_create_failed(h, PG_ERR_HIP, pg_sim_destroy);
    }
    h->s = h->own;
    *out = h;
    return PG_OK;
}

void pg_sim_destroy(pg_sim *h) {
    if (!h) return;
    (void)hipSetDevice(h->device);
    if (h->s) (void)hipStreamSynchronize(h->s);
    delete h;
}

pg_status pg_sim_set_stream(pg_sim *h, void *hip_stream) {
    if (!h) return pg_fail<pg_sim>(nullptr, PG_ERR_INVALID_ARG, "pg_sim_set_stream: null handle");
    PG_HIP_TRY(h, hipSetDevice(h->device));
    PG_HIP_TRY(h, hipStreamSynchronize(h->s));
    h->s = hip_stream ? (hipStream_t)hip_stream : (hipStream_t)h->own;
    return PG_OK;
}

void *pg_sim_stream(const pg_sim *h) { return h ? (void *)h->s : nullptr; }

pg_status pg_sim_kernel_ms(pg_sim *h, double *ops_ms, double *emit_ms) {
    if (!h) return pg_fail<pg_sim>(nullptr, PG_ERR_INVALID_ARG, "pg_sim_kernel_ms: null handle");
    if (ops_ms) *ops_ms = h->ops_ms;
    if (emit_ms) *emit_ms = h->emit_ms;
    h->ops_ms = h->emit_ms = 0;
    return PG_OK;
}

pg_status pg_sim_set_model(pg_sim *h, const uint32_t *levels, const uint32_t *stdvs, const uint32_t *dwells, uint32_t k) {
    if (!h) return pg_fail<pg_sim>(nullptr, PG_ERR_INVALID_ARG, "pg_sim_set_model: null handle");
    if (!levels || !stdvs || !dwells || k != h->prm.kmer_size) return pg_fail(h, PG_ERR_INVALID_ARG, "pg_sim_set_model: levels, stdvs, dwells and the handle's kmer_size %u are required", h->prm.kmer_size);
    uint64_t slot = 0;
    if (const char *why = pg_sim_tables_error(levels, stdvs, dwells, k, slot))
        return pg_fail(h, PG_ERR_INVALID_ARG, "pg_sim_set_model: slot %llu has level %u, stdv %u, dwell %u (%s)", (unsigned long long)slot, levels[slot], stdvs[slot], dwells[slot], why);
    const uint64_t ns = 1ull << (2 * k);
    PG_HIP_TRY(h, hipSetDevice(h->device));
    PG_HIP_TRY(h, hipStreamSynchronize(h->s));
    PG_HIP_TRY(h, h->d_levels.ensure(ns * 4)); PG_HIP_TRY(h, h->d_stdvs.ensure(ns * 4)); PG_HIP_TRY(h, h->d_dwells.ensure(ns * 4));
    PG_HIP_TRY(h, hipMemcpyAsync(h->d_levels.p, levels, ns * 4, hipMemcpyHostToDevice, h->s));
    PG_HIP_TRY(h, hipMemcpyAsync(h->d_stdvs.p, stdvs, ns * 4, hipMemcpyHostToDevice, h->s));
    PG_HIP_TRY(h, hipMemcpyAsync(h->d_dwells.p, dwells, ns * 4, hipMemcpyHostToDevice, h->s));
    PG_HIP_TRY(h, hipStreamSynchronize(h->s));
    h->k = k;
    return PG_OK;
}

pg_status pg_sim_generate(pg_sim *h, const pg_sim_batch *b, pg_sim_result *out) {
    if (!h) return pg_fail<pg_sim>(nullptr, PG_ERR_INVALID_ARG, "pg_sim_generate: null handle");
    if (!b || !out) return pg_fail(h, PG_ERR_INVALID_ARG, "pg_sim_generate: null argument");
    if (out->struct_size != sizeof(pg_sim_result)) return pg_fail(h, PG_ERR_INVALID_ARG, "pg_sim_generate: pg_sim_result.struct_size %u, this library has %zu", out->struct_size, sizeof(pg_sim_result));
    memset(out, 0, sizeof *out); out->struct_size = sizeof *out;
    if (!h->k) return pg_fail(h, PG_ERR_STATE, "pg_sim_generate: no model (pg_sim_set_model)");
    if (b->struct_size != sizeof(pg_sim_batch)) return pg_fail(h, PG_ERR_INVALID_ARG, "pg_sim_generate: pg_sim_batch.struct_size %u, this library has %zu", b->struct_size, sizeof(pg_sim_batch));
    if (b->location != PG_LOC_HOST && b->location != PG_LOC_DEVICE) return pg_fail(h, PG_ERR_INVALID_ARG, "pg_sim_generate: location must be PG_LOC_HOST or PG_LOC_DEVICE");
    if (!b->seq_off) return pg_fail(h, PG_ERR_INVALID_ARG, "pg_sim_generate: null array");
    const uint64_t n = b->n_reads;
    const pg_sim_params &prm = h->prm;
    PG_HIP_TRY(h, hipSetDevice(h->device));
    const hipStream_t s = h->s;
    const bool dev = b->location == PG_LOC_DEVICE;
    PG_HIP_TRY(h, hipStreamSynchronize(s)); // (nothing queued earlier still reads the buffers about to be refilled or regrown)
    // the offsets are looked at on the host: nothing is sized or addressed by an unchecked number
    h->seq_off.resize(n + 1);
    if (dev) {
        if (pg_ptr_kind(b->seq_off, h->device) != PG_PTR_DEVICE) return pg_fail(h, PG_ERR_INVALID_ARG, "pg_sim_generate: PG_LOC_DEVICE arrays must be device memory of device %d", h->device);
        PG_HIP_TRY(h, hipMemcpyAsync(h->seq_off.data(), b->seq_off, (n + 1) * 8, hipMemcpyDeviceToHost, s));
        PG_HIP_TRY(h, hipStreamSynchronize(s));
    } else memcpy(h->seq_off.data(), b->seq_off, (n + 1) * 8);
    h->piece_first.resize(n + 1); h->piece_read.clear();
    for (uint64_t r = 0; r < n; r++) {
        if (h->seq_off[r + 1] < h->seq_off[r]) return pg_fail(h, PG_ERR_INVALID_ARG, "pg_sim_generate: seq_off decreases at read %llu", (unsigned long long)r);
        const uint64_t lb = h->seq_off[r + 1] - h->seq_off[r];
        if (lb > 0x7fffffffull) return pg_fail(h, PG_ERR_INVALID_ARG, "pg_sim_generate: read %llu has %llu bases (at most 2^31 - 1)", (unsigned long long)r, (unsigned long long)lb);
        h->piece_first[r] = (uint32_t)h->piece_read.size();
        const uint64_t np = lb < h->k ? 0 : (lb + kPiece - 1) / kPiece;   // a read that is too short has no piece
        if (h->piece_read.size() + np > 0x7fffffffull) return pg_fail(h, PG_ERR_INVALID_ARG, "pg_sim_generate: batch too large");
        h->piece_read.insert(h->piece_read.end(), np, (uint32_t)r);
    }
    h->piece_first[n] = (uint32_t)h->piece_read.size();
    const size_t n_pieces = h->piece_read.size();
    const uint64_t n_seq = h->seq_off[n];
    if (n_seq > (1ull << 32)) return pg_fail(h, PG_ERR_UNSUPPORTED, "pg_sim_generate: %llu bases in one batch (at most 2^32)", (unsigned long long)n_seq);
    if (n_seq && !b->seq) return pg_fail(h, PG_ERR_INVALID_ARG, "pg_sim_generate: null array");

    SimBatch B{};
    B.n_reads = (uint32_t)n; B.n_pieces = (uint32_t)n_pieces; B.k = h->k; B.m = prm.sig_move_offset; B.rna = prm.rna ? 1 : 0; B.spread_pct = prm.spread_pct;
    B.lead = prm.lead; B.lead_level = prm.lead_level; B.lead_stdv = prm.lead_stdv; B.seed = prm.seed; B.first_read = b->first_read; B.Q = (int64_t)h->Q;
    B.levels = h->d_levels.p; B.stdvs = h->d_stdvs.p; B.dwells = h->d_dwells.p;
    auto room = [](size_t bytes) { return bytes + bytes / 4 + 256; };
#define SIM_ENSURE(buf, bytes) PG_HIP_TRY(h, (buf).ensure((bytes) ? (bytes) : 1, room(bytes)))
    if (dev) {
        if (n_seq && pg_ptr_kind(b->seq, h->device) != PG_PTR_DEVICE) return pg_fail(h, PG_ERR_INVALID_ARG, "pg_sim_generate: PG_LOC_DEVICE arrays must be device memory of device %d", h->device);
        B.seq = b->seq; B.seq_off = b->seq_off;
    } else {
        SIM_ENSURE(h->d_seq, n_seq); SIM_ENSURE(h->d_seqoff, (n + 1) * 8);
        if (n_seq) PG_HIP_TRY(h, hipMemcpyAsync(h->d_seq.p, b->seq, n_seq, hipMemcpyHostToDevice, s));
        PG_HIP_TRY(h, hipMemcpyAsync(h->d_seqoff.p, h->seq_off.data(), (n + 1) * 8, hipMemcpyHostToDevice, s));
        B.seq = h->d_seq.p; B.seq_off = h->d_seqoff.p;
    }
    SIM_ENSURE(h->d_pfirst, (n + 1) * 4); SIM_ENSURE(h->d_pread, n_pieces * 4); SIM_ENSURE(h->d_psum, n_pieces * 4); SIM_ENSURE(h->d_pflag, n_pieces * 4);
    SIM_ENSURE(h->d_tmpn, n_seq * 4); SIM_ENSURE(h->d_tmpslot, n_seq * 4);
    B.piece_first = h->d_pfirst.p; B.piece_read = h->d_pread.p;
    const uint32_t blocks = (uint32_t)((n_pieces + kWaves - 1) / kWaves);
    (void)hipGetLastError();

    // ---- the ops: dwells, slots, the pieces' samples and refusals
    h->psum.assign(n_pieces, 0); h->pflag.assign(n_pieces, 0);
    if (n_pieces) {
        PG_HIP_TRY(h, hipMemcpyAsync(h->d_pfirst.p, h->piece_first.data(), (n + 1) * 4, hipMemcpyHostToDevice, s));
        PG_HIP_TRY(h, hipMemcpyAsync(h->d_pread.p, h->piece_read.data(), n_pieces * 4, hipMemcpyHostToDevice, s));
        PG_HIP_TRY(h, hipEventRecord(h->ev[0], s));
        hipLaunchKernelGGL(k_sim_ops, dim3(blocks), dim3(kThreads), 0, s, B, h->d_tmpn.p, h->d_tmpslot.p, h->d_psum.p, h->d_pflag.p);
        PG_HIP_TRY(h, hipGetLastError());
        PG_HIP_TRY(h, hipEventRecord(h->ev[1], s));
        PG_HIP_TRY(h, hipMemcpyAsync(h->psum.data(), h->d_psum.p, n_pieces * 4, hipMemcpyDeviceToHost, s));
        PG_HIP_TRY(h, hipMemcpyAsync(h->pflag.data(), h->d_pflag.p, n_pieces * 4, hipMemcpyDeviceToHost, s));
        PG_HIP_TRY(h, hipStreamSynchronize(s));
        float ms = 0; PG_HIP_TRY(h, hipEventElapsedTime(&ms, h->ev[0], h->ev[1])); h->ops_ms += ms;
    }

    // ---- the statuses and the scan: where every accepted read's samples and ops go
    h->status.assign(n, PG_SIM_OK); h->ok.assign(n, 0); h->sig_off.resize(n + 1); h->op_off.resize(n + 1);
    h->psig.assign(n_pieces, 0); h->pop.assign(n_pieces, 0); h->pj0.assign(n_pieces, 0);
    h->offr.resize(n); h->qs.resize(n); h->t0.resize(n); h->t1.resize(n); h->dig.resize(n); h->off.resize(n); h->range.resize(n);
    uint64_t at_sig = 0, at_op = 0, n_refused = 0;
    for (uint64_t r = 0; r < n; r++) {
        const uint64_t lb = h->seq_off[r + 1] - h->seq_off[r];
        uint32_t flag = 0;
        for (uint32_t p = h->piece_first[r]; p < h->piece_first[r + 1]; p++) flag |= h->pflag[p];
        const uint32_t st = lb < h->k ? PG_SIM_TOO_SHORT : (flag & PG_SIM_FLAG_BAD_BASE) ? PG_SIM_BAD_BASE : (flag & PG_SIM_FLAG_NO_LEVEL) ? PG_SIM_NO_LEVEL : PG_SIM_OK;
        h->status[r] = st; h->ok[r] = st == PG_SIM_OK;
        h->sig_off[r] = at_sig; h->op_off[r] = at_op;
        h->offr[r] = pg_sim_off_r(prm.seed, b->first_read + r, prm.offset, prm.off_spread);
        h->dig[r] = (double)prm.digitisation; h->off[r] = (double)h->offr[r]; h->range[r] = (double)prm.range_e4 / 10000.0;
        h->qs[r] = st == PG_SIM_OK ? (int32_t)prm.lead : 0;
        h->t0[r] = prm.rna ? (int32_t)lb : 0; h->t1[r] = prm.rna ? 0 : (int32_t)lb;
        if (st != PG_SIM_OK) { n_refused++; continue; }
        uint64_t in_read = 0;
        for (uint32_t p = h->piece_first[r]; p < h->piece_first[r + 1]; p++) {
            h->psig[p] = at_sig + in_read; h->pj0[p] = (uint32_t)in_read; h->pop[p] = at_op + (uint64_t)(p - h->piece_first[r]) * kPiece;
            in_read += h->psum[p] + (p == h->piece_first[r] ? prm.lead : 0u);
            if (in_read > PG_SIM_BATCH_SAMPLES) break;
        }
        at_sig += in_read; at_op += lb;
        if (at_sig > PG_SIM_BATCH_SAMPLES)
            return pg_fail(h, PG_ERR_UNSUPPORTED, "pg_sim_generate: more than 2^28 samples of signal in one batch (reached at read %llu: generate fewer reads at a time)", (unsigned long long)r);
    }
    h->sig_off[n] = at_sig; h->op_off[n] = at_op;
    const uint64_t n_sig = at_sig, n_ops = at_op;

    SIM_ENSURE(h->d_sig, n_sig * 2 + 16);                                 // (16 bytes of slack: the collector's tail vector of the last read)
    SIM_ENSURE(h->d_opn, n_ops * 4); SIM_ENSURE(h->d_opt, n_ops); SIM_ENSURE(h->d_sigoff, (n + 1) * 8); SIM_ENSURE(h->d_opoff, (n + 1) * 8);
    SIM_ENSURE(h->d_psig, n_pieces * 8); SIM_ENSURE(h->d_pop, n_pieces * 8); SIM_ENSURE(h->d_pj0, n_pieces * 4); SIM_ENSURE(h->d_ok, n); SIM_ENSURE(h->d_offr, n * 4);
    SIM_ENSURE(h->d_status, n * 4); SIM_ENSURE(h->d_qs, n * 4); SIM_ENSURE(h->d_t0, n * 4); SIM_ENSURE(h->d_t1, n * 4);
    SIM_ENSURE(h->d_dig, n * 8); SIM_ENSURE(h->d_off, n * 8); SIM_ENSURE(h->d_range, n * 8);
#undef SIM_ENSURE
    PG_HIP_TRY(h, hipMemcpyAsync(h->d_sigoff.p, h->sig_off.data(), (n + 1) * 8, hipMemcpyHostToDevice, s));
    PG_HIP_TRY(h, hipMemcpyAsync(h->d_opoff.p, h->op_off.data(), (n + 1) * 8, hipMemcpyHostToDevice, s));
    if (n_ops) PG_HIP_TRY(h, hipMemsetAsync(h->d_opt.p, 0, n_ops, s));
    PG_HIP_TRY(h, hipMemsetAsync((char *)h->d_sig.p + n_sig * 2, 0, 16, s));
    if (n) {
        PG_HIP_TRY(h, hipMemcpyAsync(h->d_ok.p, h->ok.data(), n, hipMemcpyHostToDevice, s));
        PG_HIP_TRY(h, hipMemcpyAsync(h->d_offr.p, h->offr.data(), n * 4, hipMemcpyHostToDevice, s));
        PG_HIP_TRY(h, hipMemcpyAsync(h->d_status.p, h->status.data(), n * 4, hipMemcpyHostToDevice, s));
        PG_HIP_TRY(h, hipMemcpyAsync(h->d_qs.p, h->qs.data(), n * 4, hipMemcpyHostToDevice, s));
        PG_HIP_TRY(h, hipMemcpyAsync(h->d_t0.p, h->t0.data(), n * 4, hipMemcpyHostToDevice, s));
        PG_HIP_TRY(h, hipMemcpyAsync(h->d_t1.p, h->t1.data(), n * 4, hipMemcpyHostToDevice, s));
        PG_HIP_TRY(h, hipMemcpyAsync(h->d_dig.p, h->dig.data(), n * 8, hipMemcpyHostToDevice, s));
        PG_HIP_TRY(h, hipMemcpyAsync(h->d_off.p, h->off.data(), n * 8, hipMemcpyHostToDevice, s));
        PG_HIP_TRY(h, hipMemcpyAsync(h->d_range.p, h->range.data(), n * 8, hipMemcpyHostToDevice, s));
    }
    // ---- the samples
    if (n_pieces) {
        PG_HIP_TRY(h, hipMemcpyAsync(h->d_psig.p, h->psig.data(), n_pieces * 8, hipMemcpyHostToDevice, s));
        PG_HIP_TRY(h, hipMemcpyAsync(h->d_pop.p, h->pop.data(), n_pieces * 8, hipMemcpyHostToDevice, s));
        PG_HIP_TRY(h, hipMemcpyAsync(h->d_pj0.p, h->pj0.data(), n_pieces * 4, hipMemcpyHostToDevice, s));
        const SimPlace P{h->d_ok.p, h->d_offr.p, h->d_psig.p, h->d_pj0.p, h->d_pop.p};
        PG_HIP_TRY(h, hipEventRecord(h->ev[1], s));
        hipLaunchKernelGGL(k_sim_emit, dim3(blocks), dim3(kThreads), 0, s, B, P, h->d_tmpn.p, h->d_tmpslot.p, h->d_sig.p, h->d_opn.p);
        PG_HIP_TRY(h, hipGetLastError());
        PG_HIP_TRY(h, hipEventRecord(h->ev[2], s));
    }
    PG_HIP_TRY(h, hipStreamSynchronize(s));
    if (n_pieces) { float ms = 0; PG_HIP_TRY(h, hipEventElapsedTime(&ms, h->ev[1], h->ev[2])); h->emit_ms += ms; }

    out->n_reads = n; out->n_ops = n_ops; out->n_samples = n_sig; out->n_seq = n_seq; out->n_refused = n_refused;
    out->sig = h->d_sig.p; out->sig_off = h->d_sigoff.p; out->digitisation = h->d_dig.p; out->offset = h->d_off.p; out->range = h->d_range.p;
    out->query_start = h->d_qs.p; out->target_start = h->d_t0.p; out->target_end = h->d_t1.p; out->seq = B.seq; out->seq_off = B.seq_off;
    out->op_n = h->d_opn.p; out->op_t = h->d_opt.p; out->op_off = h->d_opoff.p; out->status = h->d_status.p; out->status_host = h->status.data();
    return PG_OK;
}

pg_status pg_sim_walk(const pg_sim_params *p, const uint32_t *levels, const uint32_t *stdvs, const uint32_t *dwells, const uint8_t *seq, uint32_t lb, uint64_t read, uint32_t *op_out,
                      int16_t *sig_out, uint64_t sig_cap, uint64_t *n_samples, uint32_t *status, int32_t *off_r) {
    if (!p || !levels || !stdvs || !dwells || !n_samples || !status || (lb && (!seq || !op_out)) || (sig_cap && !sig_out)) return PG_ERR_INVALID_ARG;
    if (p->struct_size != sizeof(pg_sim_params) ||
        pg_sim_rule_error(p->kmer_size, p->sig_move_offset, p->digitisation, p->range_e4, p->offset, p->off_spread, p->spread_pct, p->lead, p->lead_level, p->lead_stdv))
        return PG_ERR_INVALID_ARG;
    uint64_t slot = 0;
    if (pg_sim_tables_error(levels, stdvs, dwells, p->kmer_size, slot)) return PG_ERR_INVALID_ARG;
    std::vector<uint32_t> ops; std::vector<int16_t> sig;
    *status = pg_sim_walk_host(sim_rule(p), levels, stdvs, dwells, seq, lb, read, ops, sig, off_r);
    *n_samples = sig.size();
    if (!ops.empty()) memcpy(op_out, ops.data(), ops.size() * 4);
    if (!sig.empty() && sig.size() <= sig_cap) memcpy(sig_out, sig.data(), sig.size() * 2);
    return PG_OK;
}

pg_status pg_sim_parse_model(const char *text, size_t n, uint32_t want_k, uint32_t *kmer_size_out, uint32_t *levels_out, uint32_t *stdvs_out, size_t cap_slots, int32_t *uses_u,
                             char *err, size_t err_cap) {
    if (!text || !kmer_size_out || !levels_out || !stdvs_out) return PG_ERR_INVALID_ARG;
    PgFitModel md; std::vector<uint32_t> sd; std::string why;
    if (!pg_fit_parse_model_text(text, n, want_k, md, why, &sd)) { if (err && err_cap) snprintf(err, err_cap, "%s", why.c_str()); return PG_ERR_INPUT; }
    if (md.levels.size() > cap_slots) return PG_ERR_INVALID_ARG;
    memcpy(levels_out, md.levels.data(), md.levels.size() * 4); memcpy(stdvs_out, sd.data(), sd.size() * 4);
    *kmer_size_out = md.k;
    if (uses_u) *uses_u = md.uses_u ? 1 : 0;
    return PG_OK;
}

pg_status pg_sim_parse_dwell(const char *text, size_t n, uint32_t want_k, uint32_t *kmer_size_out, uint32_t *dwells_out, size_t cap_slots, char *err, size_t err_cap) {
    if (!text || !kmer_size_out || !dwells_out) return PG_ERR_INVALID_ARG;
    std::vector<uint32_t> dw; std::string why; uint32_t k = 0;
    if (!pg_sim_parse_dwell_text(text, n, want_k, k, dw, why)) { if (err && err_cap) snprintf(err, err_cap, "%s", why.c_str()); return PG_ERR_INPUT; }
    if (dw.size() > cap_slots) return PG_ERR_INVALID_ARG;
    memcpy(dwells_out, dw.data(), dw.size() * 4);
    *kmer_size_out = k;
    return PG_OK;
}

} // extern "C"
