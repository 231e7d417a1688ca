// pg_evalign.hip -- `poregen eventalign`: one row per event that fit counts, against the k-mer model (the rule: pg_evalign.h).
//
// A batch is laid out as for pg_fit.hip and cut the same way: pieces of PG_FIT_PIECE = 256 ops, one WAVE per piece, 64 ops a step; only
// the reads whose fit is ok have pieces. The walk of a piece is pg_fit.hip's own (pg_fit_walk.h), instantiated three times here:
//   k_fit_span   per piece the sum of its ops' lengths (gapped: and of its columns) and the look at op_t. The host scans them into every
//                piece's first sample and refuses a fitted read whose ops leave its samples before any kernel indexes the signal.
//   k_ea_count   per piece the number of its counted events: the walk without its samples (no sample is read, no LDS used). The HOST
//                scans the counts into every piece's first row and every read's row offset: it is one number per 256 ops, the host must
//                size the row and text buffers from the total before the next kernel anyway, and the per-read offsets are handed out as a
//                host array -- a device scan would save nothing of that round trip. (fit scans its piece sums the same way.)
//   k_ea_rows    the walk with its samples: a sample adds u - u_first and its square to its event's two sums with LDS atomics (the step's
//                64 events, the evd / evdd of k_fit_resid; both fit 64 bits: pg_evalign.h). Behind the step lane j finishes event j --
//                pg_evstat.h's integer mean and spread, the two conversions, z -- and writes its 40-byte record at the piece's first row
//                plus the event's rank among the step's counted events (a ballot, carried from step to step). A row's place is a function
//                of the batch alone: nothing depends on the order in which waves run, and there is no atomic on global memory.
//   k_ea_lens / k_ea_write   the text, in the pattern of k_text_lens / k_text_write: one row per lane -- its length by pg_ea_row_len, an
//                exclusive device scan of the lengths to 64-bit offsets (pg_launch_scan_u32_u64), then its bytes by pg_ea_row_write at
//                its offset behind the header line -- through the wave's LDS, so that a wave stores whole 16-byte pieces (k_ea_write).
//                The per-read strings come from two device string tables uploaded with the batch.
// No workgroup waits for another; the four waves of a workgroup never meet.
#include "../../include/pgmove.h"
#include <hip/hip_runtime.h>
#include "pg_evalign.h"
#include "pg_dev.h"
#include "pg_fit_walk.h"
#include "pg_hip_host.h"

#include <cmath>
#include <cstring>
#include <string>
#include <vector>

static_assert(sizeof(pg_evalign_row) == sizeof(PgEaRow) && offsetof(pg_evalign_row, start) == offsetof(PgEaRow, start) && offsetof(pg_evalign_row, n) == offsetof(PgEaRow, n) &&
              offsetof(pg_evalign_row, first) == offsetof(PgEaRow, first) && offsetof(pg_evalign_row, mean_u) == offsetof(PgEaRow, mean_u) &&
              offsetof(pg_evalign_row, z_c) == offsetof(PgEaRow, z_c), "pg_evalign_row is the rule's row");

namespace {

template <bool kGapped> __global__ __launch_bounds__(kThreads) void k_ea_count(const FitBatch B, uint32_t *__restrict__ pcount) {
    __shared__ WaveLds unused;                                            // (the walk without samples touches no LDS: nothing is allocated)
    const uint32_t lane = threadIdx.x & (kWave - 1), pid = blockIdx.x * kWaves + threadIdx.x / kWave;
    if (pid >= B.n_pieces) return;                                        // (the whole wave)
    const PieceGeo g = piece_geo<kGapped>(B, pid, true);
    u64 c = 0;
    walk_piece<false, kGapped, false>(B, g, unused, lane, [](bool, uint64_t) {}, [](int32_t, int32_t, uint32_t) {},
                                      [&](uint32_t, int32_t, bool counted, uint32_t, uint32_t, uint64_t) { c += counted ? 1 : 0; });
    c = wave_sum(c);
    if (lane == 0) pcount[pid] = (uint32_t)c;                             // (at most 256)
}

// ag: A and G of every read; piece_row: every piece's first row
template <bool kGapped> __global__ __launch_bounds__(kThreads) void k_ea_rows(const FitBatch B, const uint32_t *__restrict__ stdvs, const double *__restrict__ ag,
                                                                               const uint64_t *__restrict__ piece_row, PgEaRow *__restrict__ rows) {
    __shared__ WaveLds lds[kWaves];
    __shared__ int32_t first_raw[kWaves][kWave];                          // the first sample of the step's events
    const uint32_t lane = threadIdx.x & (kWave - 1), w = threadIdx.x / kWave, pid = blockIdx.x * kWaves + w;
    if (pid >= B.n_pieces) return;                                        // (the whole wave; this kernel has no workgroup barrier)
    const PieceGeo g = piece_geo<kGapped>(B, pid, true);
    WaveLds &L = lds[w];
    int32_t *fr = first_raw[w];
    const int16_t *__restrict__ sig = B.sig + g.sig0;
    const double A = ag[2ull * g.r], G = ag[2ull * g.r + 1];
    uint64_t row = piece_row[pid];
    walk_piece<true, kGapped>(B, g, L, lane,
        [&](bool counted, uint64_t start) { fr[lane] = counted ? (int32_t)sig[start] : 0; }, // (a counted event has min_dur >= 1 samples, inside the read's)
        [&](int32_t r, int32_t, uint32_t j) {
            const int64_t d = 1000ll * (r - fr[j]);                       // u - u_first, |d| < 2^26
            atomicAdd(&L.evd[j], (u64)d);
            atomicAdd(&L.evdd[j], (u64)(d * d));
        },
        [&](uint32_t n, int32_t code, bool counted, uint32_t e, uint32_t first, uint64_t start) {
            const uint64_t mask = __ballot(counted);
            if (counted) {
                PgEaRow o{g.r, e, start, n, (uint32_t)code, first, 0, 0, 0};
                pg_ea_event(fr[lane], n, (int64_t)L.evd[lane], L.evdd[lane], A, G, L.lvl[lane], stdvs[code], o.mean_u, o.stdv_u, o.z_c);
                rows[row + (uint32_t)__popcll(mask & lanemask_lt())] = o;
            }
            row += (uint32_t)__popcll(mask);
        });
}

struct EaText {
    const PgEaRow *rows; uint64_t n_rows;
    const uint8_t *seq; const uint64_t *seq_off;
    const uint32_t *levels, *stdvs;
    const uint8_t *contig; const uint64_t *contig_off;
    const uint8_t *label; const uint64_t *label_off;
    const int64_t *ref_start; const uint8_t *reverse;
    uint32_t k, sample_rate;
};
__device__ __forceinline__ PgEaText ea_text_of(const EaText &C, const PgEaRow &o) {
    PgEaText t;
    const uint64_t c0 = C.contig_off[o.read], l0 = C.label_off[o.read], s0 = C.seq_off[o.read];
    t.contig = C.contig + c0; t.contig_len = (uint32_t)(C.contig_off[o.read + 1] - c0);
    t.label = C.label + l0; t.label_len = (uint32_t)(C.label_off[o.read + 1] - l0);
    t.kmer = C.seq + s0 + o.first; t.k = C.k; t.S = (uint32_t)(C.seq_off[o.read + 1] - s0); t.first = o.first; t.reverse = C.reverse[o.read];
    t.event = o.event; t.n = o.n; t.sample_rate = C.sample_rate; t.L = C.levels[o.slot]; t.SD = C.stdvs[o.slot];
    t.mean_u = o.mean_u; t.stdv_u = o.stdv_u; t.z_c = o.z_c; t.ref_start = C.ref_start[o.read]; t.start = o.start;
    return t;
}
__global__ __launch_bounds__(256) void k_ea_lens(const EaText C, uint32_t *__restrict__ tlen) {
    const uint64_t i = (uint64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= C.n_rows) return;
    tlen[i] = pg_ea_row_len(ea_text_of(C, C.rows[i]));
}
// text: the first byte behind the header line; toff[n_rows] is the end of the last row, so no lane writes past the buffer sized by it.
// A wave's 64 rows are one run of bytes, [toff[i0], toff[i1]). Up to kStage bytes of it the lanes write their rows into the wave's LDS --
// placed so that an LDS byte and its byte of the text have the same address modulo 16 -- and the wave then stores the run as whole
// 16-byte pieces, neighbouring lanes neighbouring pieces; the run's first and last piece, which it shares with the waves beside it, go
// out byte by byte. (Measured on the configs[1] shape, DESIGN.md section 27.6: one row per lane storing its ~72 bytes one at a time, 64
// lanes on 64 different lines per store, made the text stage five times the rows stage.) A longer run -- names of hundreds of bytes --
// is written by its lanes directly.
constexpr uint32_t kStage = 8192;
__global__ __launch_bounds__(256) void k_ea_write(const EaText C, const uint64_t *__restrict__ toff, char *__restrict__ text) {
    __shared__ uint4 stage[kWaves][kStage / 16 + 1];
    const uint32_t lane = threadIdx.x & (kWave - 1), w = threadIdx.x / kWave;
    const uint64_t i0 = (uint64_t)blockIdx.x * 256 + w * kWave, i = i0 + lane;
    if (i0 >= C.n_rows) return;                                           // (the whole wave; this kernel has no workgroup barrier)
    const uint64_t i1 = i0 + kWave < C.n_rows ? i0 + kWave : C.n_rows, t0 = toff[i0], run = toff[i1] - t0;
    if (run > kStage) {
        if (i < C.n_rows) pg_ea_row_write(text + toff[i], ea_text_of(C, C.rows[i]));
        return;
    }
    char *const g = text + t0, *const lds = reinterpret_cast<char *>(stage[w]);
    const uint32_t skew = (uint32_t)(reinterpret_cast<uintptr_t>(g) & 15u), end = skew + (uint32_t)run; // the run is the LDS bytes [skew, end), end <= kStage + 15
    if (i < C.n_rows) pg_ea_row_write(lds + skew + (uint32_t)(toff[i] - t0), ea_text_of(C, C.rows[i]));
    wave_lds_sync();
    char *const gbase = g - skew;                                         // 16-byte aligned; piece c is gbase[16 c, 16 c + 16)
    for (uint32_t c = lane; 16 * c < end; c += kWave) {
        const uint32_t lo = 16 * c, hi = lo + 16;
        if (lo >= skew && hi <= end) *reinterpret_cast<uint4 *>(gbase + lo) = stage[w][c];
        else for (uint32_t j = lo < skew ? skew : lo; j < (hi < end ? hi : end); j++) gbase[j] = lds[j];
    }
}

const char kHeader[] = PG_EA_HEADER;
constexpr size_t kHeaderLen = sizeof(kHeader) - 1;

} // namespace

struct pg_evalign {
    int device = 0;
    pg_evalign_params prm{};
    PgStream own;
    hipStream_t s = nullptr;
    PgEvent ev[6];
    uint32_t k = 0;
    bool bad_model = false;        // the last pg_evalign_set_model was refused for a level without a spread
    double ms[3] = {0, 0, 0};
    PgDev<uint32_t> d_levels, d_stdvs, d_opn, d_pread, d_pfirst, d_flag, d_pcount, d_tlen;
    PgDev<int16_t> d_sig;
    PgDev<uint64_t> d_sigoff, d_seqoff, d_opoff, d_pstart, d_psum, d_pcol, d_pcsum, d_prow, d_toff, d_scan, d_coff, d_loff;
    PgDev<int64_t> d_refstart;
    PgDev<uint8_t> d_seq, d_opt, d_part, d_reverse, d_contig, d_label;
    PgDev<double> d_ag;
    PgDev<PgEaRow> d_rows;
    PgDev<char> d_text;
    std::vector<uint64_t> sig_off, seq_off, op_off, psum, pcsum, pstart, pcol, prow, row_off, coff, loff;
    std::vector<int32_t> qs;
    std::vector<uint32_t> piece_read, piece_first, pcount;
    std::vector<uint8_t> part, reverse, labels;
    std::vector<int64_t> ref_start;
    std::vector<double> ag;
    std::vector<pg_evalign_row> rows_host;
    uint64_t text_bytes = 0;
    std::string err;
};

static pg_status ea_check_params(pg_evalign *h, const pg_evalign_params *p, const char *who) {
    if (p->struct_size != sizeof(pg_evalign_params)) return pg_fail(h, PG_ERR_INVALID_ARG, "%s: struct_size %u, this library has %zu", who, p->struct_size, sizeof(pg_evalign_params));
    if (!pg_ea_params_ok(p->min_dur, p->max_dur, p->sample_rate))
        return pg_fail(h, PG_ERR_INVALID_ARG, "%s: 1 <= min_dur <= max_dur <= %u and sample_rate <= %u are required (got min_dur %u, max_dur %u, sample_rate %u)", who, PG_EA_MAX_DUR,
                       PG_EA_MAX_RATE, p->min_dur, p->max_dur, p->sample_rate);
    if (p->sig_move_offset > 64) return pg_fail(h, PG_ERR_INVALID_ARG, "%s: sig_move_offset %u (at most 64)", who, p->sig_move_offset);
    if (p->flags & ~(uint32_t)(PG_EVALIGN_TEXT | PG_EVALIGN_HOST_ROWS)) return pg_fail(h, PG_ERR_INVALID_ARG, "%s: unknown flags 0x%x", who, p->flags);
    return PG_OK;
}

extern "C" {

const char *pg_evalign_last_error(const pg_evalign *h) { return h ? h->err.c_str() : pg_create_error<pg_evalign>().c_str(); }

pg_status pg_evalign_create(const pg_evalign_params *p, int32_t device, pg_evalign **out) {
    if (!out || !p) return pg_fail<pg_evalign>(nullptr, PG_ERR_INVALID_ARG, "pg_evalign_create: null argument");
    *out = nullptr;
    if (pg_status st = ea_check_params(nullptr, p, "pg_evalign_create")) return st;
    if (pg_status st = pg_select_device<pg_evalign>(device)) return st;
    pg_evalign *h = new pg_evalign();
    h->device = device; h->prm = *p;
    hipError_t e = hipStreamCreateWithFlags(&h->own.h, hipStreamNonBlocking);
    for (int i = 0; i < 6 && e == hipSuccess; i++) e = hipEventCreate(&h->ev[i].h);
    if (e != hipSuccess) {
        pg_fail(h, PG_ERR_HIP, "pg_evalign_create: %s", hipGetErrorString(e));
        return pg_create_failed(h, PG_ERR_HIP, pg_evalign_destroy);
    }
    h->s = h->own;
    *out = h;
    return PG_OK;
}

void pg_evalign_destroy(pg_evalign *h) {
    if (!h) return;
    (void)hipSetDevice(h->device);
    if (h->s) (void)hipStreamSynchronize(h->s);
    delete h;
}

pg_status pg_evalign_set_stream(pg_evalign *h, void *hip_stream) {
    if (!h) return pg_fail<pg_evalign>(nullptr, PG_ERR_INVALID_ARG, "pg_evalign_set_stream: null handle");
    PG_HIP_TRY(h, hipSetDevice(h->device));
    PG_HIP_TRY(h, hipStreamSynchronize(h->s));
    h->s = hip_stream ? (hipStream_t)hip_stream : (hipStream_t)h->own;
    return PG_OK;
}

pg_status pg_evalign_kernel_ms(pg_evalign *h, double *ms) {
    if (!h) return pg_fail<pg_evalign>(nullptr, PG_ERR_INVALID_ARG, "pg_evalign_kernel_ms: null handle");
    for (int i = 0; i < 3; i++) { if (ms) ms[i] = h->ms[i]; h->ms[i] = 0; }
    return PG_OK;
}

pg_status pg_evalign_set_model(pg_evalign *h, const uint32_t *levels, const uint32_t *stdvs, uint32_t k) {
    if (!h) return pg_fail<pg_evalign>(nullptr, PG_ERR_INVALID_ARG, "pg_evalign_set_model: null handle");
    if (!levels || !stdvs || k < 1 || k > PG_FIT_MAX_K) return pg_fail(h, PG_ERR_INVALID_ARG, "pg_evalign_set_model: levels, stdvs and a kmer_size of 1 to %u are required", PG_FIT_MAX_K);
    const uint64_t ns = 1ull << (2 * k);
    for (uint64_t i = 0; i < ns; i++)
        if (levels[i] >= PG_FIT_MAX_LEVEL || stdvs[i] >= PG_FIT_MAX_LEVEL)
            return pg_fail(h, PG_ERR_INVALID_ARG, "pg_evalign_set_model: level %u, level_stdv %u of slot %llu (both lie below %u)", levels[i], stdvs[i], (unsigned long long)i, PG_FIT_MAX_LEVEL);
    for (uint64_t i = 0; i < ns; i++)
        if (levels[i] && !stdvs[i]) {
            h->k = 0; h->bad_model = true;
            return pg_fail(h, PG_ERR_INPUT, "pg_evalign_set_model: slot %llu has a level and a level_stdv of 0 (after rounding to 1e-3 pA): no standardized level", (unsigned long long)i);
        }
    PG_HIP_TRY(h, hipSetDevice(h->device));
    PG_HIP_TRY(h, hipStreamSynchronize(h->s));
    PG_HIP_TRY(h, h->d_levels.ensure(ns * sizeof(uint32_t)));
    PG_HIP_TRY(h, h->d_stdvs.ensure(ns * sizeof(uint32_t)));
    PG_HIP_TRY(h, h->d_flag.ensure(sizeof(uint32_t)));
    PG_HIP_TRY(h, hipMemcpyAsync(h->d_levels.p, levels, ns * sizeof(uint32_t), hipMemcpyHostToDevice, h->s));
    PG_HIP_TRY(h, hipMemcpyAsync(h->d_stdvs.p, stdvs, ns * sizeof(uint32_t), hipMemcpyHostToDevice, h->s));
    PG_HIP_TRY(h, hipStreamSynchronize(h->s));
    h->k = k; h->bad_model = false;
    return PG_OK;
}

pg_status pg_evalign_submit(pg_evalign *h, const pg_batch *b, const uint32_t *status, const double *a, const double *bb, const pg_evalign_meta *meta, pg_evalign_out *out) {
    if (!h) return pg_fail<pg_evalign>(nullptr, PG_ERR_INVALID_ARG, "pg_evalign_submit: null handle");
    if (!b || !out) return pg_fail(h, PG_ERR_INVALID_ARG, "pg_evalign_submit: null argument");
    if (out->struct_size != sizeof(pg_evalign_out)) return pg_fail(h, PG_ERR_INVALID_ARG, "pg_evalign_submit: pg_evalign_out.struct_size %u, this library has %zu", out->struct_size, sizeof(pg_evalign_out));
    memset(out, 0, sizeof *out); out->struct_size = sizeof *out;
    h->text_bytes = 0;
    if (h->bad_model) return pg_fail(h, PG_ERR_INPUT, "pg_evalign_submit: the model was refused: a k-mer with a level has a level_stdv of 0 (pg_evalign_set_model)");
    if (!h->k) return pg_fail(h, PG_ERR_STATE, "pg_evalign_submit: no model (pg_evalign_set_model)");
    if (b->struct_size != sizeof(pg_batch)) return pg_fail(h, PG_ERR_INVALID_ARG, "pg_evalign_submit: pg_batch.struct_size %u, this library has %zu", b->struct_size, sizeof(pg_batch));
    if (b->location != PG_LOC_HOST && b->location != PG_LOC_DEVICE) return pg_fail(h, PG_ERR_INVALID_ARG, "pg_evalign_submit: location must be PG_LOC_HOST or PG_LOC_DEVICE");
    const bool gapped = (b->flags & PG_BATCH_GAPPED) != 0;
    if (gapped && (b->flags & PG_BATCH_ALL_MATCHES)) return pg_fail(h, PG_ERR_INVALID_ARG, "pg_evalign_submit: a batch carries PG_BATCH_GAPPED or PG_BATCH_ALL_MATCHES, not both");
    if (!gapped && !(b->flags & PG_BATCH_ALL_MATCHES)) return pg_fail(h, PG_ERR_INVALID_ARG, "pg_evalign_submit: the batch must carry PG_BATCH_ALL_MATCHES (every op a match, as `reform` writes them) or PG_BATCH_GAPPED");
    const uint64_t n = b->n_reads;
    if (n > 0x7fffffffull) return pg_fail(h, PG_ERR_INVALID_ARG, "pg_evalign_submit: batch too large");
    if (!b->sig_off || !b->seq_off || !b->op_off || (n && (!b->query_start || !status || !a || !bb))) return pg_fail(h, PG_ERR_INVALID_ARG, "pg_evalign_submit: null array");
    if (meta && ((meta->contig && !meta->contig_off) || (meta->label && !meta->label_off))) return pg_fail(h, PG_ERR_INVALID_ARG, "pg_evalign_submit: a string table needs its offsets");
    PG_HIP_TRY(h, hipSetDevice(h->device));
    const hipStream_t s = h->s;
    const bool dev = b->location == PG_LOC_DEVICE;
    const bool want_text = (h->prm.flags & PG_EVALIGN_TEXT) != 0, want_rows = (h->prm.flags & PG_EVALIGN_HOST_ROWS) != 0;
    PG_HIP_TRY(h, hipStreamSynchronize(s)); // (a submit that failed half way may have left work queued: nothing still reads the buffers about to be refilled)
    // the arrays that lay the batch out are looked at on the host: nothing is sized or addressed by an unchecked number
    h->sig_off.resize(n + 1); h->seq_off.resize(n + 1); h->op_off.resize(n + 1); h->qs.resize(n);
    if (dev) {
        const void *must[] = {b->sig_off, b->seq_off, b->op_off, n ? (const void *)b->query_start : nullptr};
        for (const void *q : must)
            if (q && pg_ptr_kind(q, h->device) != PG_PTR_DEVICE) return pg_fail(h, PG_ERR_INVALID_ARG, "pg_evalign_submit: PG_LOC_DEVICE arrays must be device memory of device %d", h->device);
        PG_HIP_TRY(h, hipMemcpyAsync(h->sig_off.data(), b->sig_off, (n + 1) * 8, hipMemcpyDeviceToHost, s));
        PG_HIP_TRY(h, hipMemcpyAsync(h->seq_off.data(), b->seq_off, (n + 1) * 8, hipMemcpyDeviceToHost, s));
        PG_HIP_TRY(h, hipMemcpyAsync(h->op_off.data(), b->op_off, (n + 1) * 8, hipMemcpyDeviceToHost, s));
        if (n) PG_HIP_TRY(h, hipMemcpyAsync(h->qs.data(), b->query_start, n * 4, hipMemcpyDeviceToHost, s));
        PG_HIP_TRY(h, hipStreamSynchronize(s));
    } else {
        memcpy(h->sig_off.data(), b->sig_off, (n + 1) * 8); memcpy(h->seq_off.data(), b->seq_off, (n + 1) * 8); memcpy(h->op_off.data(), b->op_off, (n + 1) * 8);
        if (n) memcpy(h->qs.data(), b->query_start, n * 4);
    }
    // only the fitted reads have pieces
    h->piece_first.resize(n + 1); h->piece_read.clear(); h->part.assign(n, 0); h->ag.assign(2 * n, 0.0);
    for (uint64_t r = 0; r < n; r++) {
        if (h->sig_off[r + 1] < h->sig_off[r] || h->seq_off[r + 1] < h->seq_off[r] || h->op_off[r + 1] < h->op_off[r])
            return pg_fail(h, PG_ERR_INVALID_ARG, "pg_evalign_submit: an offset array decreases at read %llu", (unsigned long long)r);
        const uint64_t lb = h->op_off[r + 1] - h->op_off[r], S = h->seq_off[r + 1] - h->seq_off[r];
        if (lb > 0x7fffffffull) return pg_fail(h, PG_ERR_INVALID_ARG, "pg_evalign_submit: read %llu has %llu ops (at most 2^31 - 1)", (unsigned long long)r, (unsigned long long)lb);
        h->piece_first[r] = (uint32_t)h->piece_read.size();
        if (status[r] != PG_FIT_ST_OK) continue;
        if (S > PG_FIT_MAX_SLICE) return pg_fail(h, PG_ERR_INVALID_ARG, "pg_evalign_submit: read %llu has %llu bases (at most 2^32 - 1)", (unsigned long long)r, (unsigned long long)S);
        if (!gapped && S < lb)
            return pg_fail(h, PG_ERR_INVALID_ARG, "pg_evalign_submit: read %llu has %llu ops and %llu bases (an accepted read has as many bases as ops)", (unsigned long long)r,
                           (unsigned long long)lb, (unsigned long long)S);
        if (!std::isfinite(a[r]) || !std::isfinite(bb[r]) || !pg_ea_read_scale(a[r], bb[r], h->ag[2 * r], h->ag[2 * r + 1]))
            return pg_fail(h, PG_ERR_INVALID_ARG, "pg_evalign_submit: read %llu has the status ok, but a = %g and b = %g are no fit's", (unsigned long long)r, a[r], bb[r]);
        h->part[r] = 1;
        const uint64_t np = (lb + kPiece - 1) / kPiece;
        if (h->piece_read.size() + np > 0x7fffffffull) return pg_fail(h, PG_ERR_INVALID_ARG, "pg_evalign_submit: batch too large");
        h->piece_read.insert(h->piece_read.end(), np, (uint32_t)r);
    }
    h->piece_first[n] = (uint32_t)h->piece_read.size();
    const size_t n_pieces = h->piece_read.size();
    const uint64_t n_sig = h->sig_off[n], n_seq = h->seq_off[n], n_ops = h->op_off[n];
    if (n_sig - h->sig_off[0] > PG_FIT_BATCH_SAMPLES)
        return pg_fail(h, PG_ERR_UNSUPPORTED, "pg_evalign_submit: %llu samples of signal in one batch (at most 2^28: submit fewer reads at a time)", (unsigned long long)(n_sig - h->sig_off[0]));
    if (dev && b->n_ops && b->n_ops != n_ops) return pg_fail(h, PG_ERR_INVALID_ARG, "pg_evalign_submit: pg_batch.n_ops is %u, op_off ends at %llu", b->n_ops, (unsigned long long)n_ops);
    if ((n_sig && !b->sig) || (n_seq && !b->seq) || (n_ops && (!b->op_n || !b->op_t))) return pg_fail(h, PG_ERR_INVALID_ARG, "pg_evalign_submit: null array");
    // the per-read columns of the text: defaults where meta gives none
    h->ref_start.assign(n, 0); h->reverse.assign(n, 0); h->coff.assign(n + 1, 0); h->loff.assign(n + 1, 0); h->labels.clear();
    const uint8_t *contig_bytes = nullptr, *label_bytes = nullptr;
    if (want_text) {
        if (meta && meta->ref_start) memcpy(h->ref_start.data(), meta->ref_start, n * 8);
        if (meta && meta->reverse) for (uint64_t r = 0; r < n; r++) h->reverse[r] = meta->reverse[r] ? 1 : 0;
        if (meta && meta->contig_off) { memcpy(h->coff.data(), meta->contig_off, (n + 1) * 8); contig_bytes = meta->contig; }
        if (meta && meta->label_off) { memcpy(h->loff.data(), meta->label_off, (n + 1) * 8); label_bytes = meta->label; }
        else {
            for (uint64_t r = 0; r < n; r++) { const std::string t = std::to_string(r); h->loff[r] = h->labels.size(); h->labels.insert(h->labels.end(), t.begin(), t.end()); }
            h->loff[n] = h->labels.size(); label_bytes = h->labels.data();
        }
        for (uint64_t r = 0; r < n; r++)
            if (h->coff[r + 1] < h->coff[r] || h->loff[r + 1] < h->loff[r] || h->coff[r + 1] - h->coff[r] > 0xffffffffull || h->loff[r + 1] - h->loff[r] > 0xffffffffull)
                return pg_fail(h, PG_ERR_INVALID_ARG, "pg_evalign_submit: a string table's offsets decrease at read %llu", (unsigned long long)r);
        if ((h->coff[n] > h->coff[0] && !contig_bytes) || (h->loff[n] > h->loff[0] && !label_bytes)) return pg_fail(h, PG_ERR_INVALID_ARG, "pg_evalign_submit: a string table needs its bytes");
    }

    FitBatch B{};
    B.n_reads = (uint32_t)n; B.n_pieces = (uint32_t)n_pieces; B.k = h->k; B.m = h->prm.sig_move_offset; B.rna = h->prm.rna ? 1 : 0; B.min_dur = h->prm.min_dur; B.max_dur = h->prm.max_dur;
    B.levels = h->d_levels.p;
    auto room = [](size_t bytes) { return bytes + bytes / 4 + 256; };
#define EA_ENSURE(buf, bytes) PG_HIP_TRY(h, (buf).ensure((bytes) ? (bytes) : 1, room(bytes)))
    if (dev) {
        const void *must[] = {n_sig ? (const void *)b->sig : nullptr, n_seq ? (const void *)b->seq : nullptr, n_ops ? (const void *)b->op_n : nullptr, n_ops ? (const void *)b->op_t : nullptr};
        for (const void *q : must)
            if (q && pg_ptr_kind(q, h->device) != PG_PTR_DEVICE) return pg_fail(h, PG_ERR_INVALID_ARG, "pg_evalign_submit: PG_LOC_DEVICE arrays must be device memory of device %d", h->device);
        B.sig = b->sig; B.sig_off = b->sig_off; B.seq = b->seq; B.seq_off = b->seq_off; B.op_n = b->op_n; B.op_t = b->op_t; B.op_off = b->op_off;
    } else {
        EA_ENSURE(h->d_sig, n_sig * 2); EA_ENSURE(h->d_seq, n_seq); EA_ENSURE(h->d_opn, n_ops * 4); EA_ENSURE(h->d_opt, n_ops);
        EA_ENSURE(h->d_sigoff, (n + 1) * 8); EA_ENSURE(h->d_seqoff, (n + 1) * 8); EA_ENSURE(h->d_opoff, (n + 1) * 8);
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
    EA_ENSURE(h->d_pfirst, (n + 1) * 4); EA_ENSURE(h->d_pread, n_pieces * 4); EA_ENSURE(h->d_pstart, n_pieces * 8); EA_ENSURE(h->d_psum, n_pieces * 8);
    EA_ENSURE(h->d_pcol, n_pieces * 8); EA_ENSURE(h->d_pcsum, n_pieces * 8); EA_ENSURE(h->d_pcount, n_pieces * 4); EA_ENSURE(h->d_prow, n_pieces * 8);
    EA_ENSURE(h->d_part, n); EA_ENSURE(h->d_ag, n * 16);
    B.piece_first = h->d_pfirst.p; B.piece_read = h->d_pread.p; B.piece_start = h->d_pstart.p; B.piece_col = h->d_pcol.p; B.part = h->d_part.p; B.ab = h->d_ag.p;
    const uint32_t blocks = (uint32_t)((n_pieces + kWaves - 1) / kWaves);
    (void)hipGetLastError();

    h->row_off.assign(n + 1, 0);
    uint64_t n_rows = 0;
    if (n_pieces) {
        // ---- the spans of the pieces and the look at op_t; every piece's first sample (and column) on the host
        uint32_t flag = 0;
        h->psum.assign(n_pieces, 0); h->pcsum.assign(gapped ? n_pieces : 0, 0);
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
        if (gapped && (flag & 2u)) return pg_fail(h, PG_ERR_INVALID_ARG, "pg_evalign_submit: the batch carries PG_BATCH_GAPPED but holds an op code above 2 (0 match, 1 I, 2 D)");
        if (!gapped && flag) return pg_fail(h, PG_ERR_INVALID_ARG, "pg_evalign_submit: the batch carries PG_BATCH_ALL_MATCHES but holds an op that is no match (an I, a D or an unknown op)");
        h->pstart.resize(n_pieces); h->pcol.assign(n_pieces, 0);
        for (uint64_t r = 0; r < n; r++) {
            if (!h->part[r]) continue;
            const uint64_t len = h->sig_off[r + 1] - h->sig_off[r];
            uint64_t at = h->qs[r] < 0 ? 0 : (uint64_t)h->qs[r], col = 0;
            for (uint32_t p = h->piece_first[r]; p < h->piece_first[r + 1]; p++) {
                h->pstart[p] = at; at += h->psum[p];
                if (gapped) { h->pcol[p] = col; col += h->pcsum[p]; }
            }
            if (h->qs[r] < 0 || at > len)
                return pg_fail(h, PG_ERR_INVALID_ARG, "pg_evalign_submit: read %llu has the status ok, but its ops leave its samples (the status of another batch?)", (unsigned long long)r);
            if (gapped && col != h->seq_off[r + 1] - h->seq_off[r])
                return pg_fail(h, PG_ERR_INVALID_ARG, "pg_evalign_submit: read %llu has the status ok, but its reference slice has not as many bases as its ops have columns (the status of another batch?)",
                               (unsigned long long)r);
        }
        // ---- count: every piece's counted events; rows of every piece and read by a scan on the host
        h->pcount.assign(n_pieces, 0);
        PG_HIP_TRY(h, hipMemcpyAsync(h->d_pstart.p, h->pstart.data(), n_pieces * 8, hipMemcpyHostToDevice, s));
        PG_HIP_TRY(h, hipMemcpyAsync(h->d_pcol.p, h->pcol.data(), n_pieces * 8, hipMemcpyHostToDevice, s));
        PG_HIP_TRY(h, hipMemcpyAsync(h->d_part.p, h->part.data(), n, hipMemcpyHostToDevice, s));
        PG_HIP_TRY(h, hipMemcpyAsync(h->d_ag.p, h->ag.data(), n * 16, hipMemcpyHostToDevice, s));
        PG_HIP_TRY(h, hipEventRecord(h->ev[0], s));
        if (gapped) hipLaunchKernelGGL(k_ea_count<true>, dim3(blocks), dim3(kThreads), 0, s, B, h->d_pcount.p);
        else hipLaunchKernelGGL(k_ea_count<false>, dim3(blocks), dim3(kThreads), 0, s, B, h->d_pcount.p);
        PG_HIP_TRY(h, hipGetLastError());
        PG_HIP_TRY(h, hipEventRecord(h->ev[1], s));
        PG_HIP_TRY(h, hipMemcpyAsync(h->pcount.data(), h->d_pcount.p, n_pieces * 4, hipMemcpyDeviceToHost, s));
        PG_HIP_TRY(h, hipStreamSynchronize(s));
        float ms = 0; PG_HIP_TRY(h, hipEventElapsedTime(&ms, h->ev[0], h->ev[1])); h->ms[0] += ms;
        h->prow.resize(n_pieces);
        for (uint64_t r = 0; r < n; r++) {
            h->row_off[r] = n_rows;
            for (uint32_t p = h->piece_first[r]; p < h->piece_first[r + 1]; p++) {
                if (h->pcount[p] > kPiece) return pg_fail(h, PG_ERR_HIP, "pg_evalign_submit: a piece reports %u counted events", h->pcount[p]);
                h->prow[p] = n_rows; n_rows += h->pcount[p];
            }
        }
    }
    h->row_off[n] = n_rows;
    // ---- rows
    EA_ENSURE(h->d_rows, n_rows * sizeof(PgEaRow));
    if (n_rows) {
        PG_HIP_TRY(h, hipMemcpyAsync(h->d_prow.p, h->prow.data(), n_pieces * 8, hipMemcpyHostToDevice, s));
        PG_HIP_TRY(h, hipEventRecord(h->ev[2], s));
        if (gapped) hipLaunchKernelGGL(k_ea_rows<true>, dim3(blocks), dim3(kThreads), 0, s, B, h->d_stdvs.p, h->d_ag.p, h->d_prow.p, h->d_rows.p);
        else hipLaunchKernelGGL(k_ea_rows<false>, dim3(blocks), dim3(kThreads), 0, s, B, h->d_stdvs.p, h->d_ag.p, h->d_prow.p, h->d_rows.p);
        PG_HIP_TRY(h, hipGetLastError());
        PG_HIP_TRY(h, hipEventRecord(h->ev[3], s));
    }
    h->rows_host.clear();
    if (want_rows && n_rows) {
        h->rows_host.resize(n_rows);
        PG_HIP_TRY(h, hipMemcpyAsync(h->rows_host.data(), h->d_rows.p, n_rows * sizeof(PgEaRow), hipMemcpyDeviceToHost, s));
    }
    // ---- text: the header line, then the rows at the offsets a device scan of their lengths gives
    uint64_t text_rows = 0;
    if (want_text) {
        EaText C{};
        C.rows = h->d_rows.p; C.n_rows = n_rows; C.seq = B.seq; C.seq_off = B.seq_off; C.levels = h->d_levels.p; C.stdvs = h->d_stdvs.p; C.k = h->k; C.sample_rate = h->prm.sample_rate;
        if (n_rows) {
            const uint64_t cbytes = h->coff[n], lbytes = h->loff[n], scan_words = (n_rows + 4095) / 4096 + 80;
            EA_ENSURE(h->d_refstart, n * 8); EA_ENSURE(h->d_reverse, n); EA_ENSURE(h->d_coff, (n + 1) * 8); EA_ENSURE(h->d_loff, (n + 1) * 8);
            EA_ENSURE(h->d_contig, cbytes); EA_ENSURE(h->d_label, lbytes); EA_ENSURE(h->d_tlen, n_rows * 4); EA_ENSURE(h->d_toff, (n_rows + 1) * 8);
            if (scan_words * 8 > h->d_scan.cap) { // (the scan's state words are zero before its first use and left zero by every launch)
                EA_ENSURE(h->d_scan, scan_words * 8);
                PG_HIP_TRY(h, hipMemsetAsync(h->d_scan.p, 0, h->d_scan.cap, s));
            }
            PG_HIP_TRY(h, hipMemcpyAsync(h->d_refstart.p, h->ref_start.data(), n * 8, hipMemcpyHostToDevice, s));
            PG_HIP_TRY(h, hipMemcpyAsync(h->d_reverse.p, h->reverse.data(), n, hipMemcpyHostToDevice, s));
            PG_HIP_TRY(h, hipMemcpyAsync(h->d_coff.p, h->coff.data(), (n + 1) * 8, hipMemcpyHostToDevice, s));
            PG_HIP_TRY(h, hipMemcpyAsync(h->d_loff.p, h->loff.data(), (n + 1) * 8, hipMemcpyHostToDevice, s));
            if (cbytes) PG_HIP_TRY(h, hipMemcpyAsync(h->d_contig.p, contig_bytes, cbytes, hipMemcpyHostToDevice, s));
            if (lbytes) PG_HIP_TRY(h, hipMemcpyAsync(h->d_label.p, label_bytes, lbytes, hipMemcpyHostToDevice, s));
            C.contig = h->d_contig.p; C.contig_off = h->d_coff.p; C.label = h->d_label.p; C.label_off = h->d_loff.p; C.ref_start = h->d_refstart.p; C.reverse = h->d_reverse.p;
            const uint32_t tblocks = (uint32_t)((n_rows + 255) / 256);
            PG_HIP_TRY(h, hipEventRecord(h->ev[4], s));
            hipLaunchKernelGGL(k_ea_lens, dim3(tblocks), dim3(256), 0, s, C, h->d_tlen.p);
            PG_HIP_TRY(h, hipGetLastError());
            PG_HIP_TRY(h, pg_launch_scan_u32_u64(s, h->d_tlen.p, 1, n_rows, nullptr, h->d_toff.p, h->d_scan.p, nullptr, nullptr));
            PG_HIP_TRY(h, hipMemcpyAsync(&text_rows, h->d_toff.p + n_rows, 8, hipMemcpyDeviceToHost, s));
            PG_HIP_TRY(h, hipStreamSynchronize(s)); // (the text buffer is sized by the scan's total)
            EA_ENSURE(h->d_text, kHeaderLen + text_rows);
            hipLaunchKernelGGL(k_ea_write, dim3(tblocks), dim3(256), 0, s, C, h->d_toff.p, h->d_text.p + kHeaderLen);
            PG_HIP_TRY(h, hipGetLastError());
            PG_HIP_TRY(h, hipEventRecord(h->ev[5], s));
        } else EA_ENSURE(h->d_text, kHeaderLen);
        PG_HIP_TRY(h, hipMemcpyAsync(h->d_text.p, kHeader, kHeaderLen, hipMemcpyHostToDevice, s));
    }
#undef EA_ENSURE
    PG_HIP_TRY(h, hipStreamSynchronize(s));
    if (n_rows) {
        float ms = 0; PG_HIP_TRY(h, hipEventElapsedTime(&ms, h->ev[2], h->ev[3])); h->ms[1] += ms;
        if (want_text) { PG_HIP_TRY(h, hipEventElapsedTime(&ms, h->ev[4], h->ev[5])); h->ms[2] += ms; }
    }
    h->text_bytes = want_text ? kHeaderLen + text_rows : 0;
    out->n_reads = n; out->n_rows = n_rows; out->row_off = h->row_off.data();
    out->rows = n_rows ? reinterpret_cast<const pg_evalign_row *>(h->d_rows.p) : nullptr;
    out->rows_host = want_rows && n_rows ? h->rows_host.data() : nullptr;
    out->text = want_text ? h->d_text.p : nullptr; out->text_bytes = h->text_bytes;
    return PG_OK;
}

pg_status pg_evalign_copy_text(pg_evalign *h, char *dst, uint64_t cap) {
    if (!h) return pg_fail<pg_evalign>(nullptr, PG_ERR_INVALID_ARG, "pg_evalign_copy_text: null handle");
    if (!h->text_bytes) return pg_fail(h, PG_ERR_STATE, "pg_evalign_copy_text: the last submit produced no text (PG_EVALIGN_TEXT)");
    if (!dst || cap < h->text_bytes) return pg_fail(h, PG_ERR_INVALID_ARG, "pg_evalign_copy_text: the buffer holds %llu bytes, the text has %llu", (unsigned long long)cap, (unsigned long long)h->text_bytes);
    PG_HIP_TRY(h, hipSetDevice(h->device));
    PG_HIP_TRY(h, hipMemcpyAsync(dst, h->d_text.p, h->text_bytes, hipMemcpyDeviceToHost, h->s));
    PG_HIP_TRY(h, hipStreamSynchronize(h->s));
    return PG_OK;
}

static pg_status ea_walk(const pg_evalign_params *p, const uint32_t *levels, const uint32_t *stdvs, uint32_t k, const uint8_t *seq, uint64_t n_seq, const uint32_t *op_n, const uint8_t *op_t,
                         uint32_t lb, int64_t q, const int16_t *sig, uint64_t n_sig, double a, double b, pg_evalign_row *rows_out, uint64_t cap, uint64_t *n_rows) {
    if (!p || !levels || !stdvs || !n_rows || (lb && !op_n) || (n_seq && !seq) || (n_sig && !sig) || (cap && !rows_out) || k < 1 || k > PG_FIT_MAX_K) return PG_ERR_INVALID_ARG;
    *n_rows = 0;
    if (p->struct_size != sizeof(pg_evalign_params) || !pg_ea_params_ok(p->min_dur, p->max_dur, p->sample_rate) || p->sig_move_offset > 64) return PG_ERR_INVALID_ARG;
    double A, G;
    if (!std::isfinite(a) || !std::isfinite(b) || !pg_ea_read_scale(a, b, A, G)) return PG_ERR_INVALID_ARG;
    std::vector<PgEaRow> rows;
    const int st = pg_ea_walk_host(seq, n_seq, op_n, op_t, lb, q, sig, n_sig, levels, stdvs, k, p->sig_move_offset, p->rna != 0, p->min_dur, p->max_dur, a, b, rows);
    if (st == -1 || st == -2) return PG_ERR_INVALID_ARG;
    if (st != PG_FIT_OK) return PG_ERR_INPUT;
    *n_rows = rows.size();
    if (rows.size() > cap) return PG_ERR_INVALID_ARG;
    if (!rows.empty()) memcpy(rows_out, rows.data(), rows.size() * sizeof(PgEaRow));
    return PG_OK;
}

pg_status pg_evalign_walk(const pg_evalign_params *p, const uint32_t *levels, const uint32_t *stdvs, uint32_t k, const uint8_t *seq, uint32_t lb, const uint32_t *op_n, int64_t q,
                          const int16_t *sig, uint64_t n_sig, double a, double b, pg_evalign_row *rows_out, uint64_t cap, uint64_t *n_rows) {
    return ea_walk(p, levels, stdvs, k, seq, lb, op_n, nullptr, lb, q, sig, n_sig, a, b, rows_out, cap, n_rows);
}

pg_status pg_evalign_walk_gapped(const pg_evalign_params *p, const uint32_t *levels, const uint32_t *stdvs, uint32_t k, const uint8_t *seq, uint64_t n_seq, const uint32_t *op_n,
                                 const uint8_t *op_t, uint32_t lb, int64_t q, const int16_t *sig, uint64_t n_sig, double a, double b, pg_evalign_row *rows_out, uint64_t cap,
                                 uint64_t *n_rows) {
    static const uint8_t none = 0;
    if (lb && !op_t) return PG_ERR_INVALID_ARG;
    return ea_walk(p, levels, stdvs, k, seq, n_seq, op_n, lb ? op_t : &none, lb, q, sig, n_sig, a, b, rows_out, cap, n_rows);
}

uint64_t pg_evalign_row_text(const pg_evalign_row *row, const uint8_t *contig, uint32_t contig_len, const uint8_t *label, uint32_t label_len, const uint8_t *kmer, uint32_t k,
                             uint64_t n_seq, int64_t ref_start, int32_t reverse, uint32_t sample_rate, uint32_t level, uint32_t stdv, char *dst, uint64_t cap) {
    if (!row || !kmer || (contig_len && !contig) || (label_len && !label)) return 0;
    PgEaText t;
    t.contig = contig; t.contig_len = contig_len; t.label = label; t.label_len = label_len; t.kmer = kmer; t.k = k; t.S = (uint32_t)n_seq; t.first = row->first;
    t.reverse = reverse ? 1 : 0; t.event = row->event; t.n = row->n; t.sample_rate = sample_rate; t.L = level; t.SD = stdv; t.mean_u = row->mean_u; t.stdv_u = row->stdv_u;
    t.z_c = row->z_c; t.ref_start = ref_start; t.start = row->start;
    const uint32_t len = pg_ea_row_len(t);
    if (dst && cap >= len) pg_ea_row_write(dst, t);
    return len;
}

} // extern "C"
