// pg_dumptext.hip -- `poregen model`: the k-mer model from the TEXT of dump files. The inverse of pg_text.hip: a device parser that turns
// dump text back into the integers of 1e-8 units the "%.8f" print-out stands for, feeding the reduction of pg_model.hip.
//
// Replaces STEP 6 of the reference's pipeline run on existing directories (scripts/poregen.sh:54-85 calculate_mean_stddev_all: per file
// `tr ';,' '\n' | tail -n +2 | datamash median 1` and `... sstdev 1`; :33-52 calculate_dwell_times_medians: awk comma counts | datamash).
//
// A batch is one buffer of file bytes and file_off[n_files + 1]. The device handles the STRICT grammar, a file of
//     (-?D{1,8}.DDDDDDDD[,;])*      |value| < 4e7 (PG_MODEL_MAX_ABS), the last byte a ';'
// which is every file gmove writes without -d (src/gmove.cpp:938-944). Kernels per batch:
//   k_dt_count   16 bytes per lane: separators (',' ';') by ballot + popcount per wave tile of 1 KiB; the lane that holds a separator
//                reads its field backwards (at most 19 bytes, never in front of its file) and flags its file on a grammar violation
//   k_dt_scan    prefix sums of the tile counts (one workgroup)
//   k_dt_starts  separators / ';' in front of every file's first byte (tile prefix + the part of its tile in front of it)
//   k_dt_files   values and events per file (zero for a flagged file, or one that does not end in ';'), prefix sums -> val_base, ev_off
//   k_dt_parse   the lane that holds a separator parses its field into int64 units and writes units[val_base + rank in file]; at a ';'
//                also the event's end, samp_off[event + 1]
//   k_dt_evlen   ev_len[e] = samp_off[e + 1] - samp_off[e]
// then pg_launch_slot_model_units: the tiny / mid / short / long kernels of pg_model.hip over (ev_off, samp_off, ev_len, units).
// Files the device declines are finished on the host (pg_dumphost.h) when their batch is settled; see include/pgmove.h.
// The rule for one field and the bytes per lane / tile / workgroup are pg_dumptext.h, which the host test build compiles as well.
// PG_DMODEL_EVENTS adds the event table per batch: k_ev_stats / k_ev_carry (pg_evstat.hip) over (units, samp_off) leave every event's mean
// and spread, and the same reduction runs twice more over layouts in which every event is one value.
#include "../../include/pgmove.h"
#include <hip/hip_runtime.h>
#include "pg_hip_host.h"
#include "pg_internal.h"
#include "pg_model.h"
#include "pg_dumphost.h"
#include "pg_dumptext.h"
#include "pg_evstat.h"
#include "pg_modelcols.h"

#include <algorithm>
#include <cstring>
#include <string>
#include <vector>

namespace {

constexpr int kThreads = PG_DT_THREADS;
constexpr uint32_t kLane = PG_DT_LANE;            // bytes per lane
constexpr uint32_t kTile = PG_DT_TILE;            // bytes per wave: the granule of the separator prefix
constexpr uint32_t kBlockBytes = PG_DT_BLOCK;
constexpr int kScanThreads = 1024;
constexpr uint64_t kMaxBatchBytes = 1ull << 31;
constexpr uint32_t kMaxBatchFiles = 1u << 24;
constexpr uint32_t kMinField = PG_DT_MIN_FIELD;   // a file of the strict grammar holds at most bytes / 11 values
static_assert(kLane == 16 && kTile == 64 * kLane && kBlockBytes % kTile == 0, "a lane is one 16-byte load, a tile one wave of them");

using DtBatch = PgDtBatch; // one batch on the device (pg_internal.h)

template <bool kAligned> __device__ __forceinline__ uint4 load16(const uint8_t *__restrict__ p, uint64_t o, uint64_t n) {
    if (kAligned && o + 16 <= n) return *reinterpret_cast<const uint4 *>(p + o);
    uint32_t x[4] = {0, 0, 0, 0};
    for (int b = 0; b < 16; b++) if (o + b < n) x[b >> 2] |= (uint32_t)p[o + b] << (8 * (b & 3));
    return make_uint4(x[0], x[1], x[2], x[3]);
}

// the file that holds byte pos < file_off[n_files]: the one f with file_off[f] <= pos < file_off[f + 1] (file_off[0] = 0)
__device__ __forceinline__ uint32_t file_of(const uint64_t *__restrict__ file_off, uint32_t n_files, uint64_t pos) {
    uint32_t lo = 0, hi = n_files;
    while (hi - lo > 1) { const uint32_t mid = lo + (hi - lo) / 2; if (file_off[mid] <= pos) lo = mid; else hi = mid; }
    return lo;
}

// the separators among a lane's 16 bytes as bit masks (bit j = byte j); bytes at and beyond lim do not count
__device__ __forceinline__ void sep_masks(const uint4 &v, uint32_t lim, uint32_t &m_sep, uint32_t &m_semi) {
    const uint32_t w[4] = {v.x, v.y, v.z, v.w};
    m_sep = 0; m_semi = 0;
#pragma unroll
    for (uint32_t j = 0; j < 16; j++) {
        const uint32_t c = (w[j >> 2] >> (8 * (j & 3))) & 0xffu;
        m_semi |= (uint32_t)(c == ';') << j;
        m_sep |= (uint32_t)(c == ';' || c == ',') << j;
    }
    const uint32_t keep = lim >= 16 ? 0xffffu : ((1u << lim) - 1);
    m_sep &= keep; m_semi &= keep;
}

// A lane's file: the wave's first byte is looked up once (the same addresses in every lane), a lane that begins beyond that file's end
// looks for itself. Only waves that hold a file boundary diverge.
struct LaneFile { uint32_t f; uint64_t lo, hi; };
__device__ __forceinline__ LaneFile lane_file(const DtBatch &b, uint64_t wave_base, uint64_t base) {
    LaneFile lf;
    lf.f = file_of(b.file_off, b.n_files, wave_base);
    lf.hi = b.file_off[lf.f + 1];
    if (base >= lf.hi) { lf.f = file_of(b.file_off, b.n_files, base); lf.hi = b.file_off[lf.f + 1]; }
    lf.lo = b.file_off[lf.f];
    return lf;
}
__device__ __forceinline__ void next_file(const DtBatch &b, LaneFile &lf, uint64_t pos) {
    lf.f = file_of(b.file_off, b.n_files, pos); lf.lo = b.file_off[lf.f]; lf.hi = b.file_off[lf.f + 1];
}

template <bool kAligned> __global__ __launch_bounds__(kThreads) void k_dt_count(DtBatch b) {
    const uint32_t lane = threadIdx.x & 63;
    const uint64_t base = ((uint64_t)blockIdx.x * kThreads + threadIdx.x) * kLane, wave_base = base - (uint64_t)lane * kLane;
    uint32_t m_sep = 0, m_semi = 0;
    if (base < b.n) {
        const uint32_t lim = (uint32_t)min<uint64_t>(kLane, b.n - base);
        sep_masks(load16<kAligned>(b.p, base, b.n), lim, m_sep, m_semi);
        if (m_sep) {
            LaneFile lf = lane_file(b, wave_base, base);
            for (uint32_t m = m_sep; m; m &= m - 1) {
                const uint64_t pos = base + (uint32_t)__builtin_ctz(m);
                if (pos >= lf.hi) next_file(b, lf, pos);
                int64_t u; bool nz;
                if (!pg_dt_parse_field(b.p, pos, lf.lo, u, nz)) atomicOr(&b.fflags[lf.f], (uint32_t)DT_BAD);
                else if (nz) atomicOr(&b.fflags[lf.f], (uint32_t)DT_NEGZERO);
            }
        }
    }
    // the wave's separators: one ballot and one popcount per byte position (scalar work)
    uint32_t n_sep = 0, n_semi = 0;
#pragma unroll
    for (uint32_t j = 0; j < 16; j++) {
        n_sep += (uint32_t)__builtin_popcountll(__ballot((m_sep >> j) & 1u));
        n_semi += (uint32_t)__builtin_popcountll(__ballot((m_semi >> j) & 1u));
    }
    const uint64_t tile = wave_base / kTile;
    if (lane == 0 && tile < b.n_tiles) b.tile_pre[tile] = make_uint2(n_sep, n_semi);
}

// exclusive prefix of one pair per thread over the workgroup (kScanThreads threads); total = the sum over all of them
__device__ __forceinline__ uint2 block_excl_scan(uint2 v, uint2 &total) {
    __shared__ uint2 wsum[kScanThreads / 64];
    const uint32_t lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    uint2 inc = v;
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
        const uint32_t x = (uint32_t)__shfl_up((int)inc.x, o, 64), y = (uint32_t)__shfl_up((int)inc.y, o, 64);
        if ((int)lane >= o) { inc.x += x; inc.y += y; }
    }
    __syncthreads(); // wsum of an earlier call has been read
    if (lane == 63) wsum[w] = inc;
    __syncthreads();
    uint2 base = make_uint2(0, 0), tot = make_uint2(0, 0);
    for (uint32_t i = 0; i < kScanThreads / 64; i++) { if (i < w) { base.x += wsum[i].x; base.y += wsum[i].y; } tot.x += wsum[i].x; tot.y += wsum[i].y; }
    total = tot;
    return make_uint2(base.x + inc.x - v.x, base.y + inc.y - v.y);
}

// tile_pre[0 .. n_tiles): counts -> sums in front; tile_pre[n_tiles] = the totals. One workgroup, a contiguous run of tiles per thread.
__global__ __launch_bounds__(kScanThreads) void k_dt_scan(DtBatch b) {
    const uint32_t per = (b.n_tiles + kScanThreads - 1) / kScanThreads;
    const uint32_t t0 = min(threadIdx.x * per, b.n_tiles), t1 = min(t0 + per, b.n_tiles);
    uint2 s = make_uint2(0, 0);
    for (uint32_t t = t0; t < t1; t++) { const uint2 c = b.tile_pre[t]; s.x += c.x; s.y += c.y; }
    uint2 total;
    uint2 run = block_excl_scan(s, total);
    for (uint32_t t = t0; t < t1; t++) { const uint2 c = b.tile_pre[t]; b.tile_pre[t] = run; run.x += c.x; run.y += c.y; }
    if (threadIdx.x == 0) b.tile_pre[b.n_tiles] = total;
}

__device__ __forceinline__ uint32_t bytes_equal(uint32_t x, uint32_t c) { // bytes of x equal to c
    const uint32_t y = x ^ (c * 0x01010101u);
    return __popc(~(((y & 0x7f7f7f7fu) + 0x7f7f7f7fu) | y | 0x7f7f7f7fu));
}

// fstart[f] = separators / ';' in front of file_off[f], f in [0, n_files]: the tile's prefix and the bytes of the tile in front of it
template <bool kAligned> __global__ __launch_bounds__(kThreads) void k_dt_starts(DtBatch b) {
    const uint32_t f = blockIdx.x * kThreads + threadIdx.x;
    if (f > b.n_files) return;
    const uint64_t pos = b.file_off[f], t = pos / kTile;
    uint2 c = b.tile_pre[t]; // (t <= n_tiles: pos <= n)
    uint64_t o = t * kTile;
    if (kAligned)
        for (; o + 4 <= pos; o += 4) {
            const uint32_t x = *reinterpret_cast<const uint32_t *>(b.p + o);
            const uint32_t semi = bytes_equal(x, ';');
            c.x += semi + bytes_equal(x, ','); c.y += semi;
        }
    for (; o < pos; o++) { const uint32_t ch = b.p[o]; c.x += ch == ';' || ch == ','; c.y += ch == ';'; }
    b.fstart[f] = c;
}

// values and events per file -> val_base, ev_off (n_files + 1 entries each). A file that was flagged, or that does not end in ';',
// counts nothing: the reduction sees it as empty and the host finishes it. One workgroup, a contiguous run of files per thread.
__global__ __launch_bounds__(kScanThreads) void k_dt_files(DtBatch b) {
    const uint32_t per = (b.n_files + kScanThreads - 1) / kScanThreads;
    const uint32_t f0 = min(threadIdx.x * per, b.n_files), f1 = min(f0 + per, b.n_files);
    auto counts = [&](uint32_t f) {
        const uint64_t lo = b.file_off[f], hi = b.file_off[f + 1];
        uint32_t fl = b.fflags[f];
        if (hi > lo && b.p[hi - 1] != ';') fl |= DT_BAD;
        const uint2 s0 = b.fstart[f], s1 = b.fstart[f + 1];
        if ((uint64_t)(s1.x - s0.x) * kMinField > hi - lo) fl |= DT_BAD; // (cannot be for fields that passed: the buffers are sized by it)
        b.fflags[f] = fl;
        return (fl & DT_BAD) ? make_uint2(0, 0) : make_uint2(s1.x - s0.x, s1.y - s0.y);
    };
    uint2 s = make_uint2(0, 0);
    for (uint32_t f = f0; f < f1; f++) { const uint2 c = counts(f); s.x += c.x; s.y += c.y; }
    uint2 total;
    uint2 run = block_excl_scan(s, total);
    for (uint32_t f = f0; f < f1; f++) { const uint2 c = counts(f); b.val_base[f] = run.x; b.ev_off[f] = run.y; run.x += c.x; run.y += c.y; }
    if (threadIdx.x == 0) { b.val_base[b.n_files] = total.x; b.ev_off[b.n_files] = total.y; b.samp_off[0] = 0; }
}

template <bool kAligned> __global__ __launch_bounds__(kThreads) void k_dt_parse(DtBatch b) {
    const uint32_t lane = threadIdx.x & 63;
    const uint64_t base = ((uint64_t)blockIdx.x * kThreads + threadIdx.x) * kLane, wave_base = base - (uint64_t)lane * kLane;
    uint32_t m_sep = 0, m_semi = 0;
    if (base < b.n) sep_masks(load16<kAligned>(b.p, base, b.n), (uint32_t)min<uint64_t>(kLane, b.n - base), m_sep, m_semi);
    // separators of the wave's lower lanes: the ballot of every byte position, counted below this lane
    uint32_t pre_sep = 0, pre_semi = 0;
#pragma unroll
    for (uint32_t j = 0; j < 16; j++) {
        const uint64_t a = __ballot((m_sep >> j) & 1u), c = __ballot((m_semi >> j) & 1u);
        pre_sep += __builtin_amdgcn_mbcnt_hi((uint32_t)(a >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)a, 0u));
        pre_semi += __builtin_amdgcn_mbcnt_hi((uint32_t)(c >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)c, 0u));
    }
    if (!m_sep) return;
    const uint2 tp = b.tile_pre[wave_base / kTile];
    LaneFile lf = lane_file(b, wave_base, base);
    uint2 fs = b.fstart[lf.f];
    uint64_t vb = b.val_base[lf.f], eb = b.ev_off[lf.f];
    bool bad = b.fflags[lf.f] & DT_BAD;
    for (uint32_t m = m_sep; m; m &= m - 1) {
        const uint32_t j = (uint32_t)__builtin_ctz(m), below = (1u << j) - 1;
        const uint64_t pos = base + j;
        if (pos >= lf.hi) { next_file(b, lf, pos); fs = b.fstart[lf.f]; vb = b.val_base[lf.f]; eb = b.ev_off[lf.f]; bad = b.fflags[lf.f] & DT_BAD; }
        if (bad) continue;
        int64_t u; bool nz;
        (void)pg_dt_parse_field(b.p, pos, lf.lo, u, nz); // (valid: k_dt_count looked at it)
        const uint64_t at = vb + (tp.x + pre_sep + __popc(m_sep & below) - fs.x);
        if (at >= b.cap_values) continue; // (never: a value takes 11 bytes)
        b.units[at] = u;
        if ((m_semi >> j) & 1u) {
            const uint64_t e = eb + (tp.y + pre_semi + __popc(m_semi & below) - fs.y);
            if (e < b.cap_values) b.samp_off[e + 1] = at + 1;
        }
    }
}

__global__ __launch_bounds__(kThreads) void k_dt_evlen(DtBatch b) {
    const uint64_t ne = min(b.ev_off[b.n_files], b.cap_values);
    for (uint64_t e = (uint64_t)blockIdx.x * kThreads + threadIdx.x; e < ne; e += (uint64_t)gridDim.x * kThreads)
        b.ev_len[e] = (uint32_t)(b.samp_off[e + 1] - b.samp_off[e]);
}

struct Slot { // what one batch leaves for its settling
    bool pending = false;
    uint32_t n_files = 0;
    uint64_t n_bytes = 0;
    int location = PG_LOC_HOST;
    const uint8_t *dev_bytes = nullptr; // PG_LOC_DEVICE: the caller's memory
    std::vector<uint64_t> file_off;
    PgPinned<uint8_t> stage;            // PG_LOC_HOST: the batch's bytes (the upload's source, the host path's input)
    PgPinned<uint64_t> off_stage;
    PgPinned<> dl_model, dl_dwell, dl_flags, dl_totals;
    PgPinned<> dl_emean, dl_esd, dl_edw_m, dl_edw_s, dl_eflags, dl_evoff, dl_vmean, dl_vsd; // PG_DMODEL_EVENTS (the last two: PG_DMODEL_EVENTS_KEEP)
    PgEvent t0, t1, t2, t2e, t3, t4, done;
};

} // namespace

struct pg_dmodel {
    int device = 0;
    uint32_t flags = 0;
    PgStream st;
    Slot slot[2];
    int next = 0;
    // device buffers of the batch in flight (one stream: a batch's kernels run behind the previous batch's downloads)
    PgDev<uint8_t> d_bytes;
    PgDev<> d_file_off, d_tile, d_fflags, d_fstart, d_val_base, d_ev_off, d_units, d_samp_off, d_ev_len, d_out, d_dwell, d_scratch;
    // PG_DMODEL_EVENTS: every event's mean and spread, the files' refusal flags, the tiles' carries, the one-value-per-event layouts
    // (filled when they grow: id_n entries hold), the two reductions' results
    PgDev<> d_ev_mean, d_ev_sd, d_evflags, d_carry, d_id_off, d_len1, d_eout_m, d_eout_s, d_edw_m, d_edw_s;
    uint64_t id_n = 0;
    // results since the last finish
    bool finished = false;
    PgModelCols r;
    std::vector<uint32_t> host_files;
    std::vector<std::string> host_med, host_sd;
    std::vector<uint8_t> file_buf;
    pg_model_result result{};
    pg_dmodel_info info{};
    // the event table since the last finish (PG_DMODEL_EVENTS)
    PgModelCols e_mean, e_sd;
    std::vector<uint32_t> e_status;
    std::vector<uint64_t> e_n;
    std::vector<int64_t> e_vmean, e_vsd; // PG_DMODEL_EVENTS_KEEP: every event's numbers, file after file
    std::vector<std::string> e_msg;
    pg_model_result e_rm{}, e_rs{};
    double event_ms = 0, event_reduce_ms = 0;
    std::string err;
};

namespace {

void dm_clear(pg_dmodel *h) {
    h->r.clear();
    h->host_files.clear(); h->host_med.clear(); h->host_sd.clear();
    h->info = pg_dmodel_info{};
    h->result = pg_model_result{};
    h->e_mean.clear(); h->e_sd.clear(); h->e_status.clear(); h->e_n.clear(); h->e_vmean.clear(); h->e_vsd.clear(); h->e_msg.clear();
    h->e_rm = pg_model_result{}; h->e_rs = pg_model_result{}; h->event_ms = 0; h->event_reduce_ms = 0;
    h->finished = false;
}

// one file finished by the pipeline's rules on its bytes
void dm_host_file(pg_dmodel *h, const char *bytes, size_t len) {
    PgDumpHostStats hs; PgDumpHostDwell hd;
    pg_dump_host_stats(bytes, len, (h->flags & PG_MODEL_KEEP_FIRST) != 0, hs);
    pg_dump_host_dwell(bytes, len, hd);
    h->host_files.push_back((uint32_t)h->r.size());
    h->host_med.push_back(hs.median); h->host_sd.push_back(hs.sstdev);
    h->r.push_rounded(hs.n, hs.median.empty() ? NAN : (double)hs.median_ld, hs.sstdev.empty() ? NAN : (double)hs.sstdev_ld, hd.n,
                      hd.n ? ((double)hd.mid_lo + (double)hd.mid_hi) / 2.0 : NAN);
}

// wait for the slot's batch, take its results over, finish on the host what the device declined
pg_status dm_settle(pg_dmodel *h, Slot &s) {
    if (!s.pending) return PG_OK;
    s.pending = false;
    PG_HIP_TRY(h, hipEventSynchronize(s.done));
    if (h->flags & PG_DMODEL_PROFILE) {
        float a = 0, b = 0;
        PG_HIP_TRY(h, hipEventElapsedTime(&a, s.t0, s.t1)); PG_HIP_TRY(h, hipEventElapsedTime(&b, s.t1, s.t2));
        h->info.parse_ms += a; h->info.model_ms += b;
        if (h->flags & PG_DMODEL_EVENTS) {
            PG_HIP_TRY(h, hipEventElapsedTime(&a, s.t2e, s.t3)); PG_HIP_TRY(h, hipEventElapsedTime(&b, s.t3, s.t4));
            h->event_ms += a; h->event_reduce_ms += b;
        }
    }
    const bool events = (h->flags & PG_DMODEL_EVENTS) != 0;
    if (events && (h->flags & PG_DMODEL_EVENTS_KEEP)) {
        const uint64_t ne = s.dl_totals.as<uint64_t>()[1];
        h->e_vmean.insert(h->e_vmean.end(), s.dl_vmean.as<int64_t>(), s.dl_vmean.as<int64_t>() + ne);
        h->e_vsd.insert(h->e_vsd.end(), s.dl_vsd.as<int64_t>(), s.dl_vsd.as<int64_t>() + ne);
    }
    const PgSlotModel *mo = s.dl_model.as<PgSlotModel>();
    const PgSlotDwell *dw = s.dl_dwell.as<PgSlotDwell>();
    const uint32_t *fl = s.dl_flags.as<uint32_t>();
    h->info.n_values += s.dl_totals.as<uint64_t>()[0];
    h->info.n_bytes += s.n_bytes; h->info.n_batches++;
    for (uint32_t i = 0; i < s.n_files; i++) {
        const PgSlotModel &m = mo[i]; const PgSlotDwell &d = dw[i];
        const bool host = (fl[i] & DT_BAD) || (d.flags & (PG_MODEL_BAD_VALUE | PG_MODEL_BAD_SPREAD | PG_MODEL_BAD_COUNT)) ||
                          ((fl[i] & DT_NEGZERO) && m.n && m.mid_lo == 0 && m.mid_hi == 0); // datamash would print the median's sign: "-0"
        if (events) { // no host path: a file the device does not finish, or whose events it refuses, has no event table
            const PgSlotModel &em = s.dl_emean.as<PgSlotModel>()[i], &es = s.dl_esd.as<PgSlotModel>()[i];
            const uint32_t declined = (s.dl_edw_m.as<PgSlotDwell>()[i].flags | s.dl_edw_s.as<PgSlotDwell>()[i].flags) & (PG_MODEL_BAD_VALUE | PG_MODEL_BAD_SPREAD | PG_MODEL_BAD_COUNT);
            uint32_t st = host ? (uint32_t)PG_EVENTS_HOST_FILE : (s.dl_eflags.as<uint32_t>()[i] & 15u) << 1; // (a host file has no events to speak of)
            if (!st && declined) st = PG_EVENTS_DECLINED;
            const uint64_t *eo = s.dl_evoff.as<uint64_t>();
            h->e_status.push_back(st); h->e_n.push_back(eo[i + 1] - eo[i]); // (the parser's count: the slices of pg_dmodel_events_values)
            h->e_mean.push(st ? PgSlotModel{} : em); h->e_sd.push(st ? PgSlotModel{} : es);
        }
        if (host) {
            const uint64_t lo = s.file_off[i], len = s.file_off[i + 1] - lo;
            const char *bytes = reinterpret_cast<const char *>(s.stage.p) + lo;
            if (s.location == PG_LOC_DEVICE) {
                h->file_buf.resize(len ? len : 1);
                if (len) PG_HIP_TRY(h, hipMemcpy(h->file_buf.data(), s.dev_bytes + lo, len, hipMemcpyDeviceToHost));
                bytes = reinterpret_cast<const char *>(h->file_buf.data());
            }
            dm_host_file(h, bytes, len);
            continue;
        }
        h->r.push(m, &d);
    }
    return PG_OK;
}

template <class B> bool too_small(const B &b, size_t bytes) { return bytes > b.cap; }

} // namespace

// the parse kernels of one batch, in order, on st: b.fflags zeroed and b.file_off in place before them
hipError_t pg_launch_dump_parse(hipStream_t st, const PgDtBatch &b) {
    const bool al = ((uintptr_t)b.p & 15) == 0;
    const size_t nf1 = (size_t)b.n_files + 1;
    const uint32_t byte_blocks = (uint32_t)((b.n + kBlockBytes - 1) / kBlockBytes), file_blocks = (uint32_t)((nf1 + kThreads - 1) / kThreads);
    (void)hipGetLastError();
    if (byte_blocks) {
        if (al) hipLaunchKernelGGL(k_dt_count<true>, dim3(byte_blocks), dim3(kThreads), 0, st, b);
        else hipLaunchKernelGGL(k_dt_count<false>, dim3(byte_blocks), dim3(kThreads), 0, st, b);
    }
    hipLaunchKernelGGL(k_dt_scan, dim3(1), dim3(kScanThreads), 0, st, b);
    if (al) hipLaunchKernelGGL(k_dt_starts<true>, dim3(file_blocks), dim3(kThreads), 0, st, b);
    else hipLaunchKernelGGL(k_dt_starts<false>, dim3(file_blocks), dim3(kThreads), 0, st, b);
    hipLaunchKernelGGL(k_dt_files, dim3(1), dim3(kScanThreads), 0, st, b);
    if (byte_blocks) {
        if (al) hipLaunchKernelGGL(k_dt_parse<true>, dim3(byte_blocks), dim3(kThreads), 0, st, b);
        else hipLaunchKernelGGL(k_dt_parse<false>, dim3(byte_blocks), dim3(kThreads), 0, st, b);
        const uint32_t ev_blocks = (uint32_t)std::min<uint64_t>((b.cap_values + kThreads - 1) / kThreads, 4096);
        hipLaunchKernelGGL(k_dt_evlen, dim3(ev_blocks), dim3(kThreads), 0, st, b);
    }
    return hipGetLastError();
}

extern "C" {

const char *pg_dmodel_last_error(const pg_dmodel *h) { return h ? h->err.c_str() : pg_create_error<pg_dmodel>().c_str(); }

pg_status pg_dmodel_create(int32_t device, uint32_t flags, pg_dmodel **out) {
    if (!out) return pg_fail<pg_dmodel>(nullptr, PG_ERR_INVALID_ARG, "pg_dmodel_create: null argument");
    *out = nullptr;
    if (flags & ~(uint32_t)(PG_MODEL_KEEP_FIRST | PG_DMODEL_PROFILE | PG_DMODEL_EVENTS | PG_DMODEL_EVENTS_KEEP)) return pg_fail<pg_dmodel>(nullptr, PG_ERR_INVALID_ARG, "pg_dmodel_create: unknown flags 0x%x", flags);
    if (pg_status st = pg_select_device<pg_dmodel>(device)) return st;
    pg_dmodel *h = new pg_dmodel();
    h->device = device; h->flags = flags | ((flags & PG_DMODEL_EVENTS_KEEP) ? (uint32_t)PG_DMODEL_EVENTS : 0u);
    auto init = [&]() -> pg_status {
        PG_HIP_TRY(h, hipStreamCreateWithFlags(&h->st.h, hipStreamNonBlocking));
        for (Slot &s : h->slot) {
            for (PgEvent *e : {&s.t0, &s.t1, &s.t2}) PG_HIP_TRY(h, hipEventCreate(&e->h));
            if (h->flags & PG_DMODEL_EVENTS) for (PgEvent *e : {&s.t2e, &s.t3, &s.t4}) PG_HIP_TRY(h, hipEventCreate(&e->h));
            PG_HIP_TRY(h, hipEventCreateWithFlags(&s.done.h, hipEventDisableTiming));
        }
        return PG_OK;
    };
    if (pg_status st = init()) return pg_create_failed(h, st, pg_dmodel_destroy);
    *out = h;
    return PG_OK;
}

void pg_dmodel_destroy(pg_dmodel *h) {
    if (!h) return;
    (void)hipSetDevice(h->device);
    if (h->st) (void)hipStreamSynchronize(h->st);
    delete h;
}

pg_status pg_dmodel_submit(pg_dmodel *h, const void *bytes, const uint64_t *file_off, uint32_t n_files, int32_t location) {
    if (!h) return pg_fail<pg_dmodel>(nullptr, PG_ERR_INVALID_ARG, "pg_dmodel_submit: null handle");
    if (location != PG_LOC_HOST && location != PG_LOC_DEVICE) return pg_fail(h, PG_ERR_INVALID_ARG, "pg_dmodel_submit: location must be PG_LOC_HOST or PG_LOC_DEVICE");
    if (h->finished) dm_clear(h);
    if (!n_files) return PG_OK;
    if (!file_off) return pg_fail(h, PG_ERR_INVALID_ARG, "pg_dmodel_submit: null file_off");
    if (n_files > kMaxBatchFiles) return pg_fail(h, PG_ERR_INVALID_ARG, "pg_dmodel_submit: more than %u files in one call", kMaxBatchFiles);
    if (file_off[0] != 0) return pg_fail(h, PG_ERR_INVALID_ARG, "pg_dmodel_submit: file_off[0] must be 0");
    for (uint32_t i = 0; i < n_files; i++)
        if (file_off[i + 1] < file_off[i]) return pg_fail(h, PG_ERR_INVALID_ARG, "pg_dmodel_submit: file_off decreases at file %u", i);
    const uint64_t n = file_off[n_files];
    if (n > kMaxBatchBytes) return pg_fail(h, PG_ERR_INVALID_ARG, "pg_dmodel_submit: more than 2^31 bytes in one call");
    if (n && !bytes) return pg_fail(h, PG_ERR_INVALID_ARG, "pg_dmodel_submit: null bytes");
    if (h->r.size() + h->slot[0].n_files * h->slot[0].pending + h->slot[1].n_files * h->slot[1].pending + (uint64_t)n_files > 0xffffffffull)
        return pg_fail(h, PG_ERR_INVALID_ARG, "pg_dmodel_submit: more than 2^32 files since the last finish");
    PG_HIP_TRY(h, hipSetDevice(h->device));
    if (location == PG_LOC_DEVICE && n && pg_ptr_kind(bytes, h->device) != PG_PTR_DEVICE)
        return pg_fail(h, PG_ERR_INVALID_ARG, "pg_dmodel_submit: PG_LOC_DEVICE bytes are not device memory of device %d", h->device);

    Slot &s = h->slot[h->next], &prev = h->slot[h->next ^ 1];
    h->next ^= 1;
    if (pg_status st = dm_settle(h, s)) return st; // (settled by the submit behind it already, unless that one failed)

    const uint32_t n_tiles = (uint32_t)((n + kTile - 1) / kTile);
    const uint64_t cap_values = n / kMinField + 1;
    const size_t nf1 = (size_t)n_files + 1;
    const size_t scratch = pg_slot_model_scratch_bytes(n_files);
    // the device buffers are shared by the batches: one that has to grow is freed, so the batch in flight is settled first
    const bool events = (h->flags & PG_DMODEL_EVENTS) != 0, keep_events = (h->flags & PG_DMODEL_EVENTS_KEEP) != 0;
    const size_t carry = pg_ev_carry_bytes(cap_values);
    const bool grow_events = events && (too_small(h->d_ev_mean, cap_values * 8) || too_small(h->d_ev_sd, cap_values * 8) || too_small(h->d_evflags, nf1 * 4) || too_small(h->d_carry, carry) ||
                                        too_small(h->d_id_off, (cap_values + 1) * 8) || too_small(h->d_len1, cap_values * 4) || too_small(h->d_eout_m, nf1 * sizeof(PgSlotModel)) ||
                                        too_small(h->d_eout_s, nf1 * sizeof(PgSlotModel)) || too_small(h->d_edw_m, nf1 * sizeof(PgSlotDwell)) || too_small(h->d_edw_s, nf1 * sizeof(PgSlotDwell)));
    const bool grow = grow_events || too_small(h->d_bytes, n + 64) || too_small(h->d_file_off, nf1 * 8) || too_small(h->d_tile, ((size_t)n_tiles + 1) * 8) ||
                      too_small(h->d_fflags, nf1 * 4) || too_small(h->d_fstart, nf1 * 8) || too_small(h->d_val_base, nf1 * 8) || too_small(h->d_ev_off, nf1 * 8) ||
                      too_small(h->d_units, cap_values * 8) || too_small(h->d_samp_off, (cap_values + 1) * 8) || too_small(h->d_ev_len, cap_values * 4) ||
                      too_small(h->d_out, nf1 * sizeof(PgSlotModel)) || too_small(h->d_dwell, nf1 * sizeof(PgSlotDwell)) || too_small(h->d_scratch, scratch);
    if (grow) {
        if (pg_status st = dm_settle(h, prev)) return st;
        PG_HIP_TRY(h, hipStreamSynchronize(h->st));
        auto room = [](size_t b) { return b + b / 4 + 256; };
        PG_HIP_TRY(h, h->d_bytes.ensure(n + 64, room(n + 64))); PG_HIP_TRY(h, h->d_file_off.ensure(nf1 * 8, room(nf1 * 8)));
        PG_HIP_TRY(h, h->d_tile.ensure(((size_t)n_tiles + 1) * 8, room(((size_t)n_tiles + 1) * 8))); PG_HIP_TRY(h, h->d_fflags.ensure(nf1 * 4, room(nf1 * 4)));
        PG_HIP_TRY(h, h->d_fstart.ensure(nf1 * 8, room(nf1 * 8))); PG_HIP_TRY(h, h->d_val_base.ensure(nf1 * 8, room(nf1 * 8)));
        PG_HIP_TRY(h, h->d_ev_off.ensure(nf1 * 8, room(nf1 * 8))); PG_HIP_TRY(h, h->d_units.ensure(cap_values * 8, room(cap_values * 8)));
        PG_HIP_TRY(h, h->d_samp_off.ensure((cap_values + 1) * 8, room((cap_values + 1) * 8))); PG_HIP_TRY(h, h->d_ev_len.ensure(cap_values * 4, room(cap_values * 4)));
        PG_HIP_TRY(h, h->d_out.ensure(nf1 * sizeof(PgSlotModel), room(nf1 * sizeof(PgSlotModel)))); PG_HIP_TRY(h, h->d_dwell.ensure(nf1 * sizeof(PgSlotDwell), room(nf1 * sizeof(PgSlotDwell))));
        PG_HIP_TRY(h, h->d_scratch.ensure(scratch, room(scratch)));
        if (events) {
            PG_HIP_TRY(h, h->d_ev_mean.ensure(cap_values * 8, room(cap_values * 8))); PG_HIP_TRY(h, h->d_ev_sd.ensure(cap_values * 8, room(cap_values * 8)));
            PG_HIP_TRY(h, h->d_evflags.ensure(nf1 * 4, room(nf1 * 4))); PG_HIP_TRY(h, h->d_carry.ensure(carry, room(carry)));
            if (too_small(h->d_id_off, (cap_values + 1) * 8) || too_small(h->d_len1, cap_values * 4)) {
                h->id_n = 0;
                PG_HIP_TRY(h, h->d_id_off.ensure((cap_values + 1) * 8, room((cap_values + 1) * 8))); PG_HIP_TRY(h, h->d_len1.ensure(cap_values * 4, room(cap_values * 4)));
            }
            PG_HIP_TRY(h, h->d_eout_m.ensure(nf1 * sizeof(PgSlotModel), room(nf1 * sizeof(PgSlotModel)))); PG_HIP_TRY(h, h->d_eout_s.ensure(nf1 * sizeof(PgSlotModel), room(nf1 * sizeof(PgSlotModel))));
            PG_HIP_TRY(h, h->d_edw_m.ensure(nf1 * sizeof(PgSlotDwell), room(nf1 * sizeof(PgSlotDwell)))); PG_HIP_TRY(h, h->d_edw_s.ensure(nf1 * sizeof(PgSlotDwell), room(nf1 * sizeof(PgSlotDwell))));
        }
    }
    if (events) {
        PG_HIP_TRY(h, s.dl_emean.ensure(nf1 * sizeof(PgSlotModel), nf1 * sizeof(PgSlotModel) * 5 / 4)); PG_HIP_TRY(h, s.dl_esd.ensure(nf1 * sizeof(PgSlotModel), nf1 * sizeof(PgSlotModel) * 5 / 4));
        PG_HIP_TRY(h, s.dl_edw_m.ensure(nf1 * sizeof(PgSlotDwell), nf1 * sizeof(PgSlotDwell) * 5 / 4)); PG_HIP_TRY(h, s.dl_edw_s.ensure(nf1 * sizeof(PgSlotDwell), nf1 * sizeof(PgSlotDwell) * 5 / 4));
        PG_HIP_TRY(h, s.dl_eflags.ensure(nf1 * 4, nf1 * 5)); PG_HIP_TRY(h, s.dl_evoff.ensure(nf1 * 8, nf1 * 10));
        if (keep_events) { PG_HIP_TRY(h, s.dl_vmean.ensure(cap_values * 8, cap_values * 10)); PG_HIP_TRY(h, s.dl_vsd.ensure(cap_values * 8, cap_values * 10)); }
    }
    PG_HIP_TRY(h, s.off_stage.ensure(nf1 * 8, nf1 * 8 + nf1 * 2)); PG_HIP_TRY(h, s.dl_totals.ensure(16));
    PG_HIP_TRY(h, s.dl_model.ensure(nf1 * sizeof(PgSlotModel), nf1 * sizeof(PgSlotModel) * 5 / 4)); PG_HIP_TRY(h, s.dl_dwell.ensure(nf1 * sizeof(PgSlotDwell), nf1 * sizeof(PgSlotDwell) * 5 / 4));
    PG_HIP_TRY(h, s.dl_flags.ensure(nf1 * 4, nf1 * 5));

    s.n_files = n_files; s.n_bytes = n; s.location = location; s.dev_bytes = nullptr;
    s.file_off.assign(file_off, file_off + nf1);
    memcpy(s.off_stage.p, file_off, nf1 * 8);
    const uint8_t *p = h->d_bytes.p;
    if (location == PG_LOC_DEVICE) { if (n) { p = static_cast<const uint8_t *>(bytes); s.dev_bytes = p; } }
    else if (n) {
        PG_HIP_TRY(h, s.stage.ensure(n, n + n / 4 + 256));
        memcpy(s.stage.p, bytes, n);
        PG_HIP_TRY(h, hipMemcpyAsync(h->d_bytes.p, s.stage.p, n, hipMemcpyHostToDevice, h->st));
    }
    PG_HIP_TRY(h, hipMemcpyAsync(h->d_file_off.p, s.off_stage.p, nf1 * 8, hipMemcpyHostToDevice, h->st));
    PG_HIP_TRY(h, hipMemsetAsync(h->d_fflags.p, 0, nf1 * 4, h->st));

    DtBatch b{};
    b.p = p; b.n = n; b.file_off = h->d_file_off.as<uint64_t>(); b.n_files = n_files; b.n_tiles = n_tiles;
    b.tile_pre = h->d_tile.as<uint2>(); b.fflags = h->d_fflags.as<uint32_t>(); b.fstart = h->d_fstart.as<uint2>();
    b.val_base = h->d_val_base.as<uint64_t>(); b.ev_off = h->d_ev_off.as<uint64_t>();
    b.units = h->d_units.as<int64_t>(); b.samp_off = h->d_samp_off.as<uint64_t>(); b.ev_len = h->d_ev_len.as<uint32_t>();
    b.cap_values = cap_values;
    PG_HIP_TRY(h, hipEventRecord(s.t0, h->st));
    PG_HIP_TRY(h, pg_launch_dump_parse(h->st, b));
    PG_HIP_TRY(h, hipEventRecord(s.t1, h->st));
    const int all_kinds[PG_MODEL_KINDS] = {1 << 20, 1 << 20, 1 << 20, 1 << 20}; // the counts are not on the host: every kernel looks
    PG_HIP_TRY(h, pg_launch_slot_model_units(h->st, n_files, all_kinds, b.ev_off, b.samp_off, b.ev_len, b.units, (h->flags & PG_MODEL_KEEP_FIRST) ? 0u : 1u,
                                             h->d_out.as<PgSlotModel>(), h->d_dwell.as<PgSlotDwell>(), h->d_scratch.p));
    PG_HIP_TRY(h, hipEventRecord(s.t2, h->st));
    PG_HIP_TRY(h, hipMemcpyAsync(s.dl_model.p, h->d_out.p, (size_t)n_files * sizeof(PgSlotModel), hipMemcpyDeviceToHost, h->st));
    PG_HIP_TRY(h, hipMemcpyAsync(s.dl_dwell.p, h->d_dwell.p, (size_t)n_files * sizeof(PgSlotDwell), hipMemcpyDeviceToHost, h->st));
    PG_HIP_TRY(h, hipMemcpyAsync(s.dl_flags.p, h->d_fflags.p, (size_t)n_files * 4, hipMemcpyDeviceToHost, h->st));
    PG_HIP_TRY(h, hipMemcpyAsync(s.dl_totals.p, b.val_base + n_files, 8, hipMemcpyDeviceToHost, h->st));
    if (events) {
        PG_HIP_TRY(h, hipMemcpyAsync(s.dl_totals.as<uint64_t>() + 1, b.ev_off + n_files, 8, hipMemcpyDeviceToHost, h->st));
        PG_HIP_TRY(h, hipMemcpyAsync(s.dl_evoff.p, b.ev_off, nf1 * 8, hipMemcpyDeviceToHost, h->st));
        // the sample reduction's timing ends at t2; from here to t3 the new kernels, to t4 the two reductions over one value per event
        int64_t *ev_mean = h->d_ev_mean.as<int64_t>(), *ev_sd = h->d_ev_sd.as<int64_t>();
        uint64_t *id_off = h->d_id_off.as<uint64_t>(); uint32_t *len1 = h->d_len1.as<uint32_t>();
        if (h->id_n < cap_values) {
            h->id_n = std::min<uint64_t>(h->d_id_off.cap / 8 - 1, h->d_len1.cap / 4);
            PG_HIP_TRY(h, pg_launch_ev_identity(h->st, h->id_n, id_off, len1));
        }
        PG_HIP_TRY(h, hipMemsetAsync(h->d_evflags.p, 0, nf1 * 4, h->st));
        PG_HIP_TRY(h, hipEventRecord(s.t2e, h->st)); // (the downloads, the identity layouts and the flags are not the new kernels' time)
        PG_HIP_TRY(h, pg_launch_ev_stats_units(h->st, n_files, b.ev_off, b.samp_off, b.units, cap_values, cap_values, ev_mean, ev_sd, h->d_evflags.as<uint32_t>(), h->d_carry.p));
        PG_HIP_TRY(h, hipEventRecord(s.t3, h->st));
        PG_HIP_TRY(h, pg_launch_slot_model_units(h->st, n_files, all_kinds, b.ev_off, id_off, len1, ev_mean, 0u, h->d_eout_m.as<PgSlotModel>(), h->d_edw_m.as<PgSlotDwell>(), h->d_scratch.p));
        PG_HIP_TRY(h, pg_launch_slot_model_units(h->st, n_files, all_kinds, b.ev_off, id_off, len1, ev_sd, 0u, h->d_eout_s.as<PgSlotModel>(), h->d_edw_s.as<PgSlotDwell>(), h->d_scratch.p));
        PG_HIP_TRY(h, hipEventRecord(s.t4, h->st));
        PG_HIP_TRY(h, hipMemcpyAsync(s.dl_emean.p, h->d_eout_m.p, (size_t)n_files * sizeof(PgSlotModel), hipMemcpyDeviceToHost, h->st));
        PG_HIP_TRY(h, hipMemcpyAsync(s.dl_esd.p, h->d_eout_s.p, (size_t)n_files * sizeof(PgSlotModel), hipMemcpyDeviceToHost, h->st));
        PG_HIP_TRY(h, hipMemcpyAsync(s.dl_edw_m.p, h->d_edw_m.p, (size_t)n_files * sizeof(PgSlotDwell), hipMemcpyDeviceToHost, h->st));
        PG_HIP_TRY(h, hipMemcpyAsync(s.dl_edw_s.p, h->d_edw_s.p, (size_t)n_files * sizeof(PgSlotDwell), hipMemcpyDeviceToHost, h->st));
        PG_HIP_TRY(h, hipMemcpyAsync(s.dl_eflags.p, h->d_evflags.p, (size_t)n_files * 4, hipMemcpyDeviceToHost, h->st));
        if (keep_events) {
            PG_HIP_TRY(h, hipMemcpyAsync(s.dl_vmean.p, ev_mean, cap_values * 8, hipMemcpyDeviceToHost, h->st));
            PG_HIP_TRY(h, hipMemcpyAsync(s.dl_vsd.p, ev_sd, cap_values * 8, hipMemcpyDeviceToHost, h->st));
        }
    }
    PG_HIP_TRY(h, hipEventRecord(s.done, h->st));
    s.pending = true;
    return dm_settle(h, prev); // results stay in submission order: prev was submitted before s
}

pg_status pg_dmodel_sync(pg_dmodel *h) {
    if (!h) return pg_fail<pg_dmodel>(nullptr, PG_ERR_INVALID_ARG, "pg_dmodel_sync: null handle");
    PG_HIP_TRY(h, hipSetDevice(h->device));
    // the older batch first: h->next is the slot the next submit takes, i.e. the older of the two
    if (pg_status st = dm_settle(h, h->slot[h->next])) return st;
    if (pg_status st = dm_settle(h, h->slot[h->next ^ 1])) return st;
    PG_HIP_TRY(h, hipStreamSynchronize(h->st));
    return PG_OK;
}

pg_status pg_dmodel_finish(pg_dmodel *h, pg_model_result *out, pg_dmodel_info *info) {
    if (!h) return pg_fail<pg_dmodel>(nullptr, PG_ERR_INVALID_ARG, "pg_dmodel_finish: null handle");
    if (!out) return pg_fail(h, PG_ERR_INVALID_ARG, "pg_dmodel_finish: null argument");
    if (h->finished) dm_clear(h);
    const pg_status st = pg_dmodel_sync(h);
    if (st != PG_OK) { h->slot[0].pending = h->slot[1].pending = false; dm_clear(h); return st; }
    pg_model_result &r = h->result;
    h->r.fill(r, h->flags & PG_MODEL_KEEP_FIRST);
    h->info.n_files = h->r.size(); h->info.n_host_files = h->host_files.size(); h->info.host_files = h->host_files.data();
    *out = r;
    if (info) *info = h->info;
    h->finished = true;
    return PG_OK;
}

size_t pg_dmodel_format(const pg_dmodel *h, uint32_t file, int32_t which, char *buf, size_t cap) {
    if (!h || !h->finished || !buf || cap == 0 || file >= h->result.n_slots) return 0;
    buf[0] = 0;
    if (which == PG_MODEL_TEXT_MEDIAN || which == PG_MODEL_TEXT_SSTDEV) {
        const auto it = std::lower_bound(h->host_files.begin(), h->host_files.end(), file);
        if (it != h->host_files.end() && *it == file) {
            const std::string &t = (which == PG_MODEL_TEXT_MEDIAN ? h->host_med : h->host_sd)[(size_t)(it - h->host_files.begin())];
            if (t.size() >= cap) return 0;
            memcpy(buf, t.c_str(), t.size() + 1);
            return t.size();
        }
    }
    return pg_model_format(&h->result, file, which, buf, cap);
}

// ---- the event table --------------------------------------------------------------------------------------------------------------------
const char *pg_events_status_text(uint32_t st) {
    static thread_local std::string m;
    m.clear();
    if (!st) return "";
    if (st & PG_EVENTS_HOST_FILE) m += " poregen model finishes it on the host (outside the strict grammar, or declined by the reduction);";
    if (st & PG_EVENTS_ONE_SAMPLE) m += " an event with one sample has no standard deviation;";
    if (st & PG_EVENTS_TOO_LONG) m += " an event is longer than " + std::to_string(PG_EV_MAX_LEN) + " samples;";
    if (st & PG_EVENTS_TOO_WIDE) m += " a sample lies 2^41 units or further from its event's first sample;";
    if (st & PG_EVENTS_BAD_VALUE) m += " a sample is outside the fixed-point view;";
    if (st & PG_EVENTS_DECLINED) m += " the reduction declines its event means or spreads (more than 2^23 events, or values 2^40 units from the first);";
    if (m.empty()) return ""; // (bits this library does not know)
    m.pop_back();
    return m.c_str() + 1;
}
static std::string events_message(uint32_t file, uint32_t st) { return "file " + std::to_string(file) + ": " + pg_events_status_text(st); }

pg_status pg_dmodel_finish_events(pg_dmodel *h, pg_model_result *means, pg_model_result *sds, const uint32_t **status, const uint64_t **n_events) {
    if (!h) return pg_fail<pg_dmodel>(nullptr, PG_ERR_INVALID_ARG, "pg_dmodel_finish_events: null handle");
    if (!(h->flags & PG_DMODEL_EVENTS)) return pg_fail(h, PG_ERR_INVALID_ARG, "pg_dmodel_finish_events: the handle was created without PG_DMODEL_EVENTS");
    if (!means || !sds) return pg_fail(h, PG_ERR_INVALID_ARG, "pg_dmodel_finish_events: null argument");
    if (!h->finished) { pg_model_result r; if (pg_status st = pg_dmodel_finish(h, &r, nullptr)) return st; }
    h->e_mean.fill(h->e_rm, PG_MODEL_KEEP_FIRST); h->e_sd.fill(h->e_rs, PG_MODEL_KEEP_FIRST); // (an event table keeps every file's first event)
    h->e_msg.assign(h->e_status.size(), std::string());
    for (size_t i = 0; i < h->e_status.size(); i++) if (h->e_status[i]) h->e_msg[i] = events_message((uint32_t)i, h->e_status[i]);
    *means = h->e_rm; *sds = h->e_rs;
    if (status) *status = h->e_status.data();
    if (n_events) *n_events = h->e_n.data();
    return PG_OK;
}

size_t pg_dmodel_format_events(const pg_dmodel *h, uint32_t file, int32_t column, char *buf, size_t cap) {
    if (!h || !h->finished || !buf || cap == 0 || column < 0 || column > PG_EVENTS_COL_SD_SSTDEV) return 0;
    buf[0] = 0;
    return pg_model_format(column < PG_EVENTS_COL_SD_MEDIAN ? &h->e_rm : &h->e_rs, file, (column & 1) ? PG_MODEL_TEXT_SSTDEV : PG_MODEL_TEXT_MEDIAN, buf, cap);
}

const char *pg_dmodel_events_refusal(const pg_dmodel *h, uint32_t file) { return h && file < h->e_msg.size() ? h->e_msg[file].c_str() : ""; }

pg_status pg_dmodel_events_values(const pg_dmodel *h, const int64_t **mean, const int64_t **sd, uint64_t *n) {
    if (!h || !mean || !sd || !n || !h->finished || !(h->flags & PG_DMODEL_EVENTS_KEEP)) return PG_ERR_INVALID_ARG;
    *mean = h->e_vmean.data(); *sd = h->e_vsd.data(); *n = h->e_vmean.size();
    return PG_OK;
}

pg_status pg_dmodel_events_ms(const pg_dmodel *h, double *event_ms, double *reduce_ms) {
    if (!h || !h->finished) return PG_ERR_INVALID_ARG;
    if (event_ms) *event_ms = h->event_ms;
    if (reduce_ms) *reduce_ms = h->event_reduce_ms;
    return PG_OK;
}

} // extern "C"
