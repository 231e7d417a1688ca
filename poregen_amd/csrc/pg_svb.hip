// pg_svb.hip -- svb-zd signal blocks of BLOW5 records decoded on the device: the blocks arrive as they lie in the (inflated) records,
// int16 samples leave in device memory (layout and rule: pg_svb.h; the host's decoder of the same blocks: host/io.cpp).
//
// The work is two dependent running sums per read: over the byte lengths (where a value's data bytes lie) and over the deltas (the
// samples). A read is cut into pieces of kPiece values, one wave (= one workgroup) each; a wave takes a piece in steps of 256 values,
// one control byte = 4 values per lane, and both sums are wave64 DPP scans (pg_dev.h) with the carries kept in registers. Pieces
// behind the first need the two sums of everything in front of them in their read:
//   k_svb_lens        : the data bytes of every piece that has a successor (control bytes only)
//   k_svb_scan        : per long read (one wave), the exclusive sum over its pieces -> each piece's data offset
//   k_svb_decode<0>   : the sum of the deltas of every piece that has a successor (the data bytes, decoded a first time)
//   k_svb_scan        : -> each piece's first running sum
//   k_svb_decode<1>   : every piece: decode, scan, store
// A batch without a read longer than kPiece -- configs[1]'s 4 000-sample reads -- runs the last kernel alone. Nothing is handed from
// workgroup to workgroup inside a launch.
//
// Bytes are loaded as bytes: a block starts at any offset, and no load may leave it. The host has checked (pg_svb_check) that the
// control bytes lie inside the block and that the span of samples holds `count` values, so control loads and stores need no further
// check; a data byte is loaded only in front of the block's end. A read whose byte lengths sum to more than its data bytes is
// flagged in bad[]; the values whose bytes are missing decode as if those bytes were 0, inside the read's own span.
#include "../../include/pgmove.h"
#include <hip/hip_runtime.h>
#include "pg_svb.h"
#include "pg_sigdec.h"
#include "pg_dev.h"

#include <algorithm>
#include <cstring>
#include <string>
#include <vector>

namespace {

constexpr int kWave = WAVE;
constexpr int kThreads = 256;                       // the per-read kernels
constexpr uint32_t kPiece = PG_SVB_PIECE_VALUES;
constexpr uint32_t kStep = PG_SVB_WAVE_VALUES;
static_assert(kStep == kWave * PG_SVB_LANE_VALUES && kPiece % kStep == 0 && PG_SVB_LANE_VALUES == 4, "one control byte per lane and step");

struct SvbBatch {
    const uint8_t *blocks;
    const uint64_t *block_off;   // n_reads + 1
    const uint32_t *cnt;         // checked counts (0: nothing to decode)
    const uint2 *extra;          // (read, piece) of pieces 1..
    const uint2 *longs;          // (read, index of its piece 1 in extra)
    uint32_t n_reads, n_long;
};

// the piece of workgroup b. kAll: every read's piece 0, then extra; else the long reads' piece 0, then extra. id: the piece's slot in
// the per-piece arrays (piece 0: the read's number, a later piece: n_reads + its index in extra)
template <bool kAll> __device__ __forceinline__ void piece_of(const SvbBatch &B, uint32_t b, uint32_t &r, uint32_t &p, uint32_t &id) {
    const uint32_t n_first = kAll ? B.n_reads : B.n_long;
    if (b < n_first) { r = kAll ? b : B.longs[b].x; p = 0; id = r; }
    else { const uint2 e = B.extra[b - n_first]; r = e.x; p = e.y; id = B.n_reads + (b - n_first); }
}

// the count field of every block, byte by byte (device blocks: the host checks it before anything else looks at the block)
__global__ __launch_bounds__(kThreads) void k_svb_heads(const uint8_t *__restrict__ blocks, const uint64_t *__restrict__ block_off, uint32_t n_reads,
                                                        uint32_t *__restrict__ cnt) {
    const uint32_t r = blockIdx.x * kThreads + threadIdx.x;
    if (r >= n_reads) return;
    const uint64_t b0 = block_off[r], len = block_off[r + 1] - b0;
    uint32_t c = 0;
    if (len >= 4) c = (uint32_t)blocks[b0] | ((uint32_t)blocks[b0 + 1] << 8) | ((uint32_t)blocks[b0 + 2] << 16) | ((uint32_t)blocks[b0 + 3] << 24);
    cnt[r] = c;
}

__global__ __launch_bounds__(kWave) void k_svb_lens(const SvbBatch B, uint32_t *__restrict__ pbytes) {
    uint32_t r, p, id;
    piece_of<false>(B, blockIdx.x, r, p, id);
    if (((uint64_t)p + 1) * kPiece >= B.cnt[r]) return;              // the read's last piece: nothing follows it
    const uint8_t *__restrict__ ctrl = B.blocks + B.block_off[r] + 4 + (uint64_t)p * (kPiece / 4);
    uint32_t sum = 0;
#pragma unroll
    for (uint32_t i = 0; i < kPiece / 4 / kWave; i++) {              // a full piece: kPiece / 4 control bytes, all inside the block
        const uint32_t c = ctrl[i * kWave + threadIdx.x];
        sum += 4u + (c & 3u) + ((c >> 2) & 3u) + ((c >> 4) & 3u) + (c >> 6);
    }
    for (int o = 32; o > 0; o >>= 1) sum += __shfl_xor(sum, o);
    if (threadIdx.x == 0) pbytes[id] = sum;
}

// one wave per long read: out[piece] = the sum of in[] over the read's pieces in front of it (pieces 1..; piece 0 starts at 0),
// 64 pieces per step
__device__ __forceinline__ uint32_t wave_incl_scan(uint32_t v) { return wave_incl_scan_u32(v); }
__device__ __forceinline__ uint64_t wave_incl_scan(uint64_t v) { return wave_incl_scan_u64(v); }
template <class T> __global__ __launch_bounds__(kWave) void k_svb_scan(const SvbBatch B, const uint32_t *__restrict__ in, T *__restrict__ out) {
    const uint32_t r = B.longs[blockIdx.x].x, first = B.n_reads + B.longs[blockIdx.x].y;
    const uint32_t np = (uint32_t)(((uint64_t)B.cnt[r] + kPiece - 1) / kPiece);
    T carry = 0;
    for (uint32_t p0 = 0; p0 < np; p0 += kWave) {                     // (uniform: the scan needs every lane)
        const uint32_t p = p0 + threadIdx.x;
        const T x = p + 1 < np ? (T)in[p ? first + (p - 1) : r] : (T)0;   // (the last piece has no sum of its own)
        const T incl = wave_incl_scan(x);
        if (p >= 1 && p < np) out[first + (p - 1)] = carry + (incl - x);
        carry += __shfl(incl, kWave - 1);
    }
}

// kWrite: every piece, samples stored. Else: the pieces that have a successor, the sum of their deltas to pdelta[].
template <bool kWrite>
__global__ __launch_bounds__(kWave) void k_svb_decode(const SvbBatch B, const uint64_t *__restrict__ poff, const uint32_t *__restrict__ pcarry,
                                                      uint32_t *__restrict__ pdelta, const uint64_t *__restrict__ sig_off, int16_t *__restrict__ sig,
                                                      uint8_t *__restrict__ bad) {
    uint32_t r, p, id;
    piece_of<kWrite>(B, blockIdx.x, r, p, id);
    const uint32_t cnt = B.cnt[r];
    const uint64_t v0 = (uint64_t)p * kPiece;
    if (v0 >= cnt) return;                                            // (an empty read, or a bad one: uniform over the wave)
    if (!kWrite && v0 + kPiece >= cnt) return;
    const uint32_t nv = (uint32_t)min((uint64_t)kPiece, cnt - v0);
    const uint64_t b0 = B.block_off[r], nctrl = pg_svb_nctrl(cnt);
    const uint64_t avail = B.block_off[r + 1] - b0 - 4 - nctrl;      // data bytes of the block (pg_svb_check: >= cnt)
    const uint8_t *__restrict__ ctrl = B.blocks + b0 + 4 + (v0 >> 2);
    const uint8_t *__restrict__ data = B.blocks + b0 + 4 + nctrl;
    int16_t *__restrict__ out = kWrite ? sig + sig_off[r] + v0 : nullptr;
    uint64_t doff = p ? poff[id] : 0;                                 // the piece's first data byte
    uint32_t carry = (kWrite && p) ? pcarry[id] : 0;                 // the running sum in front of the piece
    const uint32_t lane = threadIdx.x;
    bool is_bad = false;
    for (uint32_t s0 = 0; s0 < nv; s0 += kStep) {                    // (uniform: the scans below need every lane)
        const uint32_t vi = s0 + lane * 4;
        const uint32_t c = vi < nv ? ctrl[vi >> 2] : 0u;
        uint32_t len[4], tot = 0;
#pragma unroll
        for (int k = 0; k < 4; k++) { len[k] = vi + k < nv ? ((c >> (2 * k)) & 3u) + 1u : 0u; tot += len[k]; }
        const uint32_t incl = wave_incl_scan_u32(tot);
        uint64_t q = doff + (incl - tot);
        if (q + tot > avail) is_bad = true;
        uint32_t run = 0, pre[4];
#pragma unroll
        for (int k = 0; k < 4; k++) {
            uint32_t v = 0;
#pragma unroll
            for (uint32_t j = 0; j < 4; j++)
                if (j < len[k] && q + j < avail) v |= (uint32_t)data[q + j] << (8 * j);
            q += len[k];
            run += (v >> 1) ^ (0u - (v & 1u));                        // zig-zag; a value past nv has no bytes: delta 0
            pre[k] = run;
        }
        const uint32_t incl2 = wave_incl_scan_u32(run);
        if (kWrite) {
            const uint32_t base = carry + (incl2 - run);
            if (vi + 3 < nv && (((uintptr_t)(out + vi)) & 7) == 0) {  // four samples, 8-byte aligned (the same answer in every full lane)
                const uint32_t a = ((base + pre[0]) & 0xffffu) | ((base + pre[1]) << 16), b = ((base + pre[2]) & 0xffffu) | ((base + pre[3]) << 16);
                *reinterpret_cast<uint2 *>(out + vi) = make_uint2(a, b);
            } else {
#pragma unroll
                for (int k = 0; k < 4; k++) if (vi + k < nv) out[vi + k] = (int16_t)(uint16_t)(base + pre[k]);
            }
        }
        carry += (uint32_t)__builtin_amdgcn_readlane((int)incl2, kWave - 1);
        doff += (uint32_t)__builtin_amdgcn_readlane((int)incl, kWave - 1);
    }
    if (is_bad) bad[r] = 1;
    if (!kWrite && lane == 0) pdelta[id] = carry;
}

#define SVB_FAIL(code, ...) do { char b_[400]; snprintf(b_, sizeof b_, __VA_ARGS__); err = b_; return (code); } while (0)
#define SVB_HIP(expr) do { const hipError_t e_ = (expr); if (e_ != hipSuccess) SVB_FAIL(PG_ERR_HIP, "%s failed: %s", #expr, hipGetErrorString(e_)); } while (0)

} // namespace

pg_status PgSvbCore::prepare(int device, hipStream_t s, const void *blocks, uint64_t n_block_bytes, const uint64_t *block_off, uint64_t n,
                             int32_t location, std::string &err, bool upload) {
    prepared = false;
    if (n >= (1ull << 31)) SVB_FAIL(PG_ERR_INVALID_ARG, "%llu reads in one batch (at most 2^31 - 1)", (unsigned long long)n);
    if (location != PG_LOC_HOST && location != PG_LOC_DEVICE) SVB_FAIL(PG_ERR_INVALID_ARG, "location must be PG_LOC_HOST or PG_LOC_DEVICE");
    if (n && !block_off) SVB_FAIL(PG_ERR_INVALID_ARG, "null block_off");
    n_reads = n;
    cnt.assign(n, 0); bad0.assign(n, 0);
    if (!n) { prepared = true; return PG_OK; }
    for (uint64_t r = 0; r < n; r++)
        if (block_off[r + 1] < block_off[r]) SVB_FAIL(PG_ERR_INPUT, "block_off decreases at read %llu", (unsigned long long)r);
    if (block_off[n] > n_block_bytes) SVB_FAIL(PG_ERR_INVALID_ARG, "block_off runs past the %llu block bytes", (unsigned long long)n_block_bytes);
    if (block_off[n] && !blocks) SVB_FAIL(PG_ERR_INVALID_ARG, "null blocks");
    const uint64_t first = block_off[0], used = block_off[n] - first;
    SVB_HIP(d_boff.ensure((n + 1) * sizeof(uint64_t)));
    SVB_HIP(d_cnt.ensure(n * sizeof(uint32_t)));
    SVB_HIP(hipMemcpyAsync(d_boff.p, block_off, (n + 1) * sizeof(uint64_t), hipMemcpyHostToDevice, s));
    if (location == PG_LOC_DEVICE) {
        if (used && pg_ptr_kind(blocks, device) != PG_PTR_DEVICE) SVB_FAIL(PG_ERR_INVALID_ARG, "PG_LOC_DEVICE blocks must be device memory of device %d", device);
        blocks_dev = (const uint8_t *)blocks;
        hipLaunchKernelGGL(k_svb_heads, dim3((uint32_t)((n + kThreads - 1) / kThreads)), dim3(kThreads), 0, s, blocks_dev, d_boff.p, (uint32_t)n, d_cnt.p);
        SVB_HIP(hipGetLastError());
        SVB_HIP(hipMemcpyAsync(cnt.data(), d_cnt.p, n * sizeof(uint32_t), hipMemcpyDeviceToHost, s));
        SVB_HIP(hipStreamSynchronize(s));
    } else {
        // the bytes the offsets cover, at the same offsets on the device (nothing in front of block_off[0] is copied)
        SVB_HIP(d_blocks.ensure(std::max<uint64_t>(block_off[n], 1), std::max<uint64_t>(block_off[n] + block_off[n] / 4, 1)));
        if (used && upload) {
            const uint8_t *from = (const uint8_t *)blocks + first;
            if (pg_ptr_kind(blocks, device) != PG_PTR_PINNED) {
                SVB_HIP(hipStreamSynchronize(s));                     // (an earlier batch may still be copied out of the staging buffer)
                SVB_HIP(h_stage.ensure(used, used + used / 4));
                memcpy(h_stage.p, from, used);
                from = h_stage.p;
            }
            SVB_HIP(hipMemcpyAsync(d_blocks.p + first, from, used, hipMemcpyHostToDevice, s));
        }
        blocks_dev = d_blocks.p;
        const uint8_t *hb = (const uint8_t *)blocks;
        for (uint64_t r = 0; r < n; r++)
            if (block_off[r + 1] - block_off[r] >= 4) memcpy(&cnt[r], hb + block_off[r], 4);
    }
    for (uint64_t r = 0; r < n; r++)
        if (pg_svb_check(block_off[r + 1] - block_off[r], cnt[r]) != PG_SVB_OK) { cnt[r] = 0; bad0[r] = 1; }
    SVB_HIP(hipMemcpyAsync(d_cnt.p, cnt.data(), n * sizeof(uint32_t), hipMemcpyHostToDevice, s));
    prepared = upload;
    return PG_OK;
}

pg_status PgSvbCore::run(hipStream_t s, int16_t *sig_out, const uint64_t *sig_off, uint8_t *bad_out, std::string &err) {
    if (!prepared) SVB_FAIL(PG_ERR_STATE, "no prepared batch");
    prepared = false;
    const uint64_t n = n_reads;
    if (!n) return PG_OK;
    if (!sig_off || !bad_out) SVB_FAIL(PG_ERR_INVALID_ARG, "null argument");
    extra.clear(); longs.clear();
    for (uint64_t r = 0; r < n; r++) {
        if (sig_off[r + 1] < sig_off[r]) SVB_FAIL(PG_ERR_INPUT, "sig_off decreases at read %llu", (unsigned long long)r);
        if (sig_off[r + 1] - sig_off[r] < cnt[r])
            SVB_FAIL(PG_ERR_INVALID_ARG, "read %llu has %u samples and a span of %llu", (unsigned long long)r, cnt[r], (unsigned long long)(sig_off[r + 1] - sig_off[r]));
        if (cnt[r] > kPiece) {
            longs.push_back(make_uint2((uint32_t)r, (uint32_t)extra.size()));
            for (uint32_t p = 1; (uint64_t)p * kPiece < cnt[r]; p++) extra.push_back(make_uint2((uint32_t)r, p));
        }
    }
    if (sig_off[n] > sig_off[0] && !sig_out) SVB_FAIL(PG_ERR_INVALID_ARG, "null sig_out");
    const size_t n_extra = extra.size(), n_long = longs.size(), n_ids = n + n_extra;
    if (n_ids > 0x7fffffffull) SVB_FAIL(PG_ERR_INVALID_ARG, "batch too large");
    SVB_HIP(d_soff.ensure((n + 1) * sizeof(uint64_t)));
    SVB_HIP(d_bad.ensure(n));
    SVB_HIP(h_bad.ensure(n));
    SVB_HIP(hipMemcpyAsync(d_soff.p, sig_off, (n + 1) * sizeof(uint64_t), hipMemcpyHostToDevice, s));
    SVB_HIP(hipMemsetAsync(d_bad.p, 0, n, s));
    SvbBatch B{blocks_dev, d_boff.p, d_cnt.p, nullptr, nullptr, (uint32_t)n, (uint32_t)n_long};
    if (n_long) {
        SVB_HIP(d_extra.ensure(n_extra * sizeof(uint2)));
        SVB_HIP(d_long.ensure(n_long * sizeof(uint2)));
        SVB_HIP(d_pbytes.ensure(n_ids * sizeof(uint32_t)));
        SVB_HIP(d_pdelta.ensure(n_ids * sizeof(uint32_t)));
        SVB_HIP(d_pcarry.ensure(n_ids * sizeof(uint32_t)));
        SVB_HIP(d_poff.ensure(n_ids * sizeof(uint64_t)));
        SVB_HIP(hipMemcpyAsync(d_extra.p, extra.data(), n_extra * sizeof(uint2), hipMemcpyHostToDevice, s));
        SVB_HIP(hipMemcpyAsync(d_long.p, longs.data(), n_long * sizeof(uint2), hipMemcpyHostToDevice, s));
        B.extra = d_extra.p; B.longs = d_long.p;
        const dim3 pieces((uint32_t)(n_long + n_extra)), per_read((uint32_t)n_long);
        hipLaunchKernelGGL(k_svb_lens, pieces, dim3(kWave), 0, s, B, d_pbytes.p);
        SVB_HIP(hipGetLastError());
        hipLaunchKernelGGL(k_svb_scan<uint64_t>, per_read, dim3(kWave), 0, s, B, d_pbytes.p, d_poff.p);
        SVB_HIP(hipGetLastError());
        hipLaunchKernelGGL(k_svb_decode<false>, pieces, dim3(kWave), 0, s, B, d_poff.p, (const uint32_t *)nullptr, d_pdelta.p, (const uint64_t *)nullptr,
                           (int16_t *)nullptr, d_bad.p);
        SVB_HIP(hipGetLastError());
        hipLaunchKernelGGL(k_svb_scan<uint32_t>, per_read, dim3(kWave), 0, s, B, d_pdelta.p, d_pcarry.p);
        SVB_HIP(hipGetLastError());
    }
    hipLaunchKernelGGL(k_svb_decode<true>, dim3((uint32_t)n_ids), dim3(kWave), 0, s, B, d_poff.p, d_pcarry.p, (uint32_t *)nullptr, d_soff.p, sig_out, d_bad.p);
    SVB_HIP(hipGetLastError());
    SVB_HIP(hipMemcpyAsync(h_bad.p, d_bad.p, n, hipMemcpyDeviceToHost, s));
    SVB_HIP(hipStreamSynchronize(s));
    for (uint64_t r = 0; r < n; r++) bad_out[r] = (bad0[r] || h_bad.p[r]) ? 1 : 0;
    return PG_OK;
}

// ---- pg_sigdec_*: the decoder alone -----------------------------------------------------------------------------------------------

struct pg_sigdec {
    int device = 0;
    PgStream s;
    PgSvbCore core;
    std::string err;
};

extern "C" {

const char *pg_sigdec_last_error(const pg_sigdec *h) { return h ? h->err.c_str() : pg_create_error<pg_sigdec>().c_str(); }

pg_status pg_sigdec_create(int32_t device, pg_sigdec **out) {
    if (!out) return pg_fail<pg_sigdec>(nullptr, PG_ERR_INVALID_ARG, "pg_sigdec_create: null argument");
    *out = nullptr;
    if (pg_status st = pg_select_device<pg_sigdec>(device)) return st;
    pg_sigdec *h = new pg_sigdec();
    h->device = device;
    const hipError_t e = hipStreamCreateWithFlags(&h->s.h, hipStreamNonBlocking);
    if (e != hipSuccess) {
        pg_fail(h, PG_ERR_HIP, "pg_sigdec_create: %s", hipGetErrorString(e));
        return pg_create_failed(h, PG_ERR_HIP, pg_sigdec_destroy);
    }
    *out = h;
    return PG_OK;
}

void pg_sigdec_destroy(pg_sigdec *h) {
    if (!h) return;
    (void)hipSetDevice(h->device);
    if (h->s) (void)hipStreamSynchronize(h->s);
    delete h;
}

pg_status pg_sigdec_counts(pg_sigdec *h, const void *blocks, uint64_t n_block_bytes, const uint64_t *block_off, uint64_t n_reads, int32_t location,
                           uint32_t *counts_out) {
    if (!h) return pg_fail<pg_sigdec>(nullptr, PG_ERR_INVALID_ARG, "pg_sigdec_counts: null handle");
    if (n_reads && !counts_out) return pg_fail(h, PG_ERR_INVALID_ARG, "pg_sigdec_counts: null argument");
    PG_HIP_TRY(h, hipSetDevice(h->device));
    std::string err;
    if (pg_status st = h->core.prepare(h->device, h->s, blocks, n_block_bytes, block_off, n_reads, location, err, false)) return pg_fail(h, st, "pg_sigdec_counts: %s", err.c_str());
    PG_HIP_TRY(h, hipStreamSynchronize(h->s));
    for (uint64_t r = 0; r < n_reads; r++) counts_out[r] = h->core.count(r);
    return PG_OK;
}

pg_status pg_sigdec_decode(pg_sigdec *h, const void *blocks, uint64_t n_block_bytes, const uint64_t *block_off, uint64_t n_reads, int32_t location,
                           int16_t *sig_out_device, const uint64_t *sig_off, uint8_t *bad_out) {
    if (!h) return pg_fail<pg_sigdec>(nullptr, PG_ERR_INVALID_ARG, "pg_sigdec_decode: null handle");
    PG_HIP_TRY(h, hipSetDevice(h->device));
    std::string err;
    if (pg_status st = h->core.prepare(h->device, h->s, blocks, n_block_bytes, block_off, n_reads, location, err)) return pg_fail(h, st, "pg_sigdec_decode: %s", err.c_str());
    if (n_reads && sig_off && sig_off[n_reads] > sig_off[0] && pg_ptr_kind(sig_out_device, h->device) != PG_PTR_DEVICE) {
        (void)hipStreamSynchronize(h->s);
        return pg_fail(h, PG_ERR_INVALID_ARG, "pg_sigdec_decode: sig_out must be device memory of device %d", h->device);
    }
    const pg_status st = h->core.run(h->s, sig_out_device, sig_off, bad_out, err);
    if (st) { (void)hipStreamSynchronize(h->s); return pg_fail(h, st, "pg_sigdec_decode: %s", err.c_str()); }
    return PG_OK;
}

} // extern "C"
