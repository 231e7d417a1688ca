// pg_svbenc.hip -- int16 samples in device memory encoded into the svb-zd signal blocks of BLOW5 records, on the device (layout and rule:
// pg_svb.h; the decoder of the same blocks: pg_svb.hip; the host's statement of the rule: pg_svb_encode_host).
//
// Unlike decoding, one running sum couples the values: the deltas are local (a value needs the sample in front of it, nothing else), and
// the byte lengths give the data offsets. A read is cut into pieces of kPiece values, one wave (= one workgroup) each -- an empty read
// has one piece, which writes its count --; a wave takes its piece in steps of 256 values, one control byte = 4 values per lane, and the
// sum over the byte lengths is a wave64 DPP scan (pg_dev.h) with the carry in a register.
//   k_enc<false> : the data bytes of every piece (2 bytes read per sample, one number written per piece)
//   host         : the sizes come back (4 bytes per piece), one pass over them gives every read's block offset and every piece's data
//                  offset, and those go up (8 bytes per piece and per read). One stream synchronisation between the two launches.
//   k_enc<true>  : the count, the control bytes and the data bytes of every piece
// Nothing is handed from wave to wave inside a launch: no look-back, no atomics.
//
// The blocks of a batch lie back to back, so two pieces of a read and two reads' blocks meet at any byte address. A wave stores no byte
// outside its own piece's control and data ranges: the count, the control bytes and the data bytes all go out as byte stores. (Measured
// against staging a step's data bytes in the wave's LDS and writing the dwords that lie wholly inside the step's range as dwords: the
// emit kernel 0.227 against 0.211 ms on 200 M samples, 16 us of a call of 650 us and of a command of half a second -- DESIGN.md §21.4.
// The simpler one stays.)
#include "../../include/pgmove.h"
#include <hip/hip_runtime.h>
#include "pg_svb.h"
#include "pg_hip_host.h"
#include "pg_dev.h"

#include <algorithm>
#include <string>
#include <vector>

namespace {

constexpr int kWave = WAVE;
constexpr uint32_t kPiece = PG_SVB_PIECE_VALUES;
constexpr uint32_t kStep = PG_SVB_WAVE_VALUES;
constexpr uint64_t kMaxBatchSamples = 1ull << 28;  // what `simulate` generates at most in one batch
static_assert(kStep == kWave * PG_SVB_LANE_VALUES && kPiece % kStep == 0 && PG_SVB_LANE_VALUES == 4, "one control byte per lane and step");

struct EncBatch {
    const int16_t *sig;
    const uint64_t *sig_off;       // n_reads + 1
    const uint32_t *piece_read;    // the read of every piece
    const uint32_t *piece_first;   // the first piece of every read (n_reads + 1)
};

// kEmit: the block bytes of the piece. Else: psize[piece] = its data bytes.
// block_off: every read's block; pdata: the piece's first data byte, counted from the start of blocks
template <bool kEmit>
__global__ __launch_bounds__(kWave) void k_enc(const EncBatch B, uint32_t *__restrict__ psize, const uint64_t *__restrict__ block_off,
                                               const uint64_t *__restrict__ pdata, uint8_t *__restrict__ blocks) {
    const uint32_t pid = blockIdx.x, lane = threadIdx.x;
    const uint32_t r = B.piece_read[pid], p = pid - B.piece_first[r];
    const uint64_t s_first = B.sig_off[r], cnt = B.sig_off[r + 1] - s_first;   // (the host: cnt < 2^32)
    const uint64_t v0 = (uint64_t)p * kPiece;
    const uint32_t nv = (uint32_t)min((uint64_t)kPiece, cnt - v0);             // (0: an empty read's only piece)
    const int16_t *__restrict__ in = B.sig + s_first + v0;
    uint8_t *__restrict__ ctrl = nullptr;
    uint64_t doff = 0;
    if (kEmit) {
        const uint64_t b0 = block_off[r];
        if (p == 0 && lane < 4) blocks[b0 + lane] = (uint8_t)((uint32_t)cnt >> (8 * lane));
        ctrl = blocks + b0 + 4 + (v0 >> 2);
        doff = pdata[pid];
    }
    int32_t carry = (p && nv) ? (int32_t)in[-1] : 0;                          // the sample in front of the piece; of a read: 0
    uint32_t sum = 0;
    for (uint32_t s0 = 0; s0 < nv; s0 += kStep) {                             // (uniform: the scan below needs every lane)
        const uint32_t vi = s0 + lane * 4;
        int32_t s[4] = {0, 0, 0, 0};
        if (vi + 3 < nv && (((uintptr_t)(in + vi)) & 7) == 0) {               // four samples, 8-byte aligned (the same answer in every full lane)
            const uint2 q = *reinterpret_cast<const uint2 *>(in + vi);
            s[0] = (int32_t)(int16_t)(q.x & 0xffffu); s[1] = (int32_t)q.x >> 16; s[2] = (int32_t)(int16_t)(q.y & 0xffffu); s[3] = (int32_t)q.y >> 16;
        } else {
#pragma unroll
            for (int k = 0; k < 4; k++) if (vi + k < nv) s[k] = (int32_t)in[vi + k];
        }
        const int32_t up = __shfl_up(s[3], 1, kWave);
        int32_t prev = lane ? up : carry;
        uint32_t v[4], len[4], tot = 0, c = 0;
#pragma unroll
        for (int k = 0; k < 4; k++) {
            v[k] = pg_svb_zigzag(s[k] - prev);
            prev = s[k];
            len[k] = vi + k < nv ? pg_svb_min_len(v[k]) : 0u;                   // a value past the piece has no bytes and code 0
            if (len[k]) c |= (len[k] - 1u) << (2 * k);
            tot += len[k];
        }
        carry = __builtin_amdgcn_readlane(s[3], kWave - 1);                    // (looked at only when a step follows: then this one is full)
        if (!kEmit) { sum += tot; continue; }

        if (vi < nv) ctrl[vi >> 2] = (uint8_t)c;
        const uint32_t incl = wave_incl_scan_u32(tot);
        const uint32_t total = (uint32_t)__builtin_amdgcn_readlane((int)incl, kWave - 1);
        uint8_t *dst = blocks + doff + (incl - tot);                          // this lane's data bytes; the step's: total from blocks + doff
#pragma unroll
        for (int k = 0; k < 4; k++) {
#pragma unroll
            for (uint32_t j = 0; j < 3; j++) if (j < len[k]) dst[j] = (uint8_t)(v[k] >> (8 * j));
            dst += len[k];
        }
        doff += total;
    }
    if (!kEmit) {
        for (int o = 32; o > 0; o >>= 1) sum += __shfl_xor(sum, o);
        if (lane == 0) psize[pid] = sum;
    }
}

} // namespace

struct pg_sigenc {
    int device = 0;
    PgStream own;
    hipStream_t s = nullptr;
    PgEvent ev[4];
    double lens_ms = 0, emit_ms = 0;
    PgDev<int16_t> d_sig;
    PgDev<uint8_t> d_blocks;
    PgDev<uint64_t> d_soff, d_boff, d_pdata;
    PgDev<uint32_t> d_pread, d_pfirst, d_psize;
    PgPinned<uint32_t> h_psize;
    std::vector<uint32_t> piece_read, piece_first;
    std::vector<uint64_t> block_off, pdata;
    std::string err;
};

// what is wrong with the offsets of a batch (why, at), or PG_OK and the samples they span
static pg_status sigenc_check_offsets(const uint64_t *sig_off, uint64_t n, uint64_t *total, const char **why, uint64_t *at) {
    for (uint64_t r = 0; r < n; r++) {
        *at = r;
        if (sig_off[r + 1] < sig_off[r]) { *why = "sig_off decreases"; return PG_ERR_INPUT; }
        if (sig_off[r + 1] - sig_off[r] > 0xffffffffull) { *why = "a read of more than 2^32 - 1 samples"; return PG_ERR_UNSUPPORTED; }
    }
    *total = n ? sig_off[n] - sig_off[0] : 0;
    return PG_OK;
}

extern "C" {

const char *pg_sigenc_last_error(const pg_sigenc *h) { return h ? h->err.c_str() : pg_create_error<pg_sigenc>().c_str(); }

pg_status pg_sigenc_create(int32_t device, pg_sigenc **out) {
    if (!out) return pg_fail<pg_sigenc>(nullptr, PG_ERR_INVALID_ARG, "pg_sigenc_create: null argument");
    *out = nullptr;
    if (pg_status st = pg_select_device<pg_sigenc>(device)) return st;
    pg_sigenc *h = new pg_sigenc();
    h->device = device;
    hipError_t e = hipStreamCreateWithFlags(&h->own.h, hipStreamNonBlocking);
    for (int i = 0; i < 4 && e == hipSuccess; i++) e = hipEventCreate(&h->ev[i].h);
    if (e != hipSuccess) {
        pg_fail(h, PG_ERR_HIP, "pg_sigenc_create: %s", hipGetErrorString(e));
        return pg_create_failed(h, PG_ERR_HIP, pg_sigenc_destroy);
    }
    h->s = h->own;
    *out = h;
    return PG_OK;
}

void pg_sigenc_destroy(pg_sigenc *h) {
    if (!h) return;
    (void)hipSetDevice(h->device);
    if (h->s) (void)hipStreamSynchronize(h->s);
    delete h;
}

pg_status pg_sigenc_set_stream(pg_sigenc *h, void *hip_stream) {
    if (!h) return pg_fail<pg_sigenc>(nullptr, PG_ERR_INVALID_ARG, "pg_sigenc_set_stream: null handle");
    PG_HIP_TRY(h, hipSetDevice(h->device));
    PG_HIP_TRY(h, hipStreamSynchronize(h->s));
    h->s = hip_stream ? (hipStream_t)hip_stream : (hipStream_t)h->own;
    return PG_OK;
}

void *pg_sigenc_stream(const pg_sigenc *h) { return h ? (void *)h->s : nullptr; }

pg_status pg_sigenc_kernel_ms(pg_sigenc *h, double *lens_ms, double *emit_ms) {
    if (!h) return pg_fail<pg_sigenc>(nullptr, PG_ERR_INVALID_ARG, "pg_sigenc_kernel_ms: null handle");
    if (lens_ms) *lens_ms = h->lens_ms;
    if (emit_ms) *emit_ms = h->emit_ms;
    h->lens_ms = h->emit_ms = 0;
    return PG_OK;
}

uint64_t pg_sigenc_bound(const uint64_t *sig_off, uint64_t n_reads) {
    if (!n_reads) return 0;
    if (!sig_off) return UINT64_MAX;
    uint64_t sum = 0;
    for (uint64_t r = 0; r < n_reads; r++) {
        if (sig_off[r + 1] < sig_off[r]) return UINT64_MAX;
        sum += pg_svb_bound(sig_off[r + 1] - sig_off[r]);
    }
    return sum;
}

pg_status pg_sigenc_encode(pg_sigenc *h, const int16_t *sig, const uint64_t *sig_off, uint64_t n, int32_t location, pg_sigenc_result *out) {
    if (!h) return pg_fail<pg_sigenc>(nullptr, PG_ERR_INVALID_ARG, "pg_sigenc_encode: null handle");
    if (!out || out->struct_size != sizeof(pg_sigenc_result))
        return pg_fail(h, PG_ERR_INVALID_ARG, "pg_sigenc_encode: out is null or its struct_size is not %zu", sizeof(pg_sigenc_result));
    out->n_block_bytes = 0; out->blocks = nullptr; out->block_off = nullptr;
    if (location != PG_LOC_HOST && location != PG_LOC_DEVICE) return pg_fail(h, PG_ERR_INVALID_ARG, "pg_sigenc_encode: location must be PG_LOC_HOST or PG_LOC_DEVICE");
    if (n >= (1ull << 31)) return pg_fail(h, PG_ERR_INVALID_ARG, "pg_sigenc_encode: %llu reads in one batch (at most 2^31 - 1)", (unsigned long long)n);
    if (n && !sig_off) return pg_fail(h, PG_ERR_INVALID_ARG, "pg_sigenc_encode: null sig_off");
    // ---- refused before anything is allocated
    uint64_t total = 0, at = 0; const char *why = nullptr;
    if (pg_status st = sigenc_check_offsets(sig_off, n, &total, &why, &at)) return pg_fail(h, st, "pg_sigenc_encode: %s at read %llu", why, (unsigned long long)at);
    if (total > kMaxBatchSamples)
        return pg_fail(h, PG_ERR_UNSUPPORTED, "pg_sigenc_encode: %llu samples in one call (at most 2^28: encode fewer reads at a time)", (unsigned long long)total);
    if (total && !sig) return pg_fail(h, PG_ERR_INVALID_ARG, "pg_sigenc_encode: null sig");
    h->block_off.assign(n + 1, 0);
    out->block_off = h->block_off.data();
    if (!n) return PG_OK;

    PG_HIP_TRY(h, hipSetDevice(h->device));
    const hipStream_t s = h->s;
    if (location == PG_LOC_DEVICE && total && pg_ptr_kind(sig, h->device) != PG_PTR_DEVICE)
        return pg_fail(h, PG_ERR_INVALID_ARG, "pg_sigenc_encode: PG_LOC_DEVICE sig must be device memory of device %d", h->device);
    PG_HIP_TRY(h, hipStreamSynchronize(s));                                  // (an earlier call's copies out of the host vectors below)

    // ---- the pieces: ceil(samples / kPiece) per read, one for an empty read
    h->piece_first.resize(n + 1); h->piece_read.clear();
    for (uint64_t r = 0; r < n; r++) {
        h->piece_first[r] = (uint32_t)h->piece_read.size();
        const uint64_t cnt = sig_off[r + 1] - sig_off[r], np = cnt ? (cnt + kPiece - 1) / kPiece : 1;
        h->piece_read.insert(h->piece_read.end(), np, (uint32_t)r);
    }
    const size_t n_pieces = h->piece_read.size();                             // <= n + 2^28 / kPiece < 2^32
    h->piece_first[n] = (uint32_t)n_pieces;

    const int16_t *sig_dev = sig;
    if (location == PG_LOC_HOST) {                                            // the samples the offsets span, at the same offsets
        PG_HIP_TRY(h, h->d_sig.ensure(std::max<uint64_t>(total, 1) * 2, std::max<uint64_t>(total + total / 4, 1) * 2));
        if (total) PG_HIP_TRY(h, hipMemcpyAsync(h->d_sig.p, sig + sig_off[0], total * 2, hipMemcpyHostToDevice, s));
        sig_dev = reinterpret_cast<const int16_t *>(reinterpret_cast<uintptr_t>(h->d_sig.p) - 2 * sig_off[0]);
    }
    PG_HIP_TRY(h, h->d_soff.ensure((n + 1) * 8));
    PG_HIP_TRY(h, h->d_boff.ensure((n + 1) * 8));
    PG_HIP_TRY(h, h->d_pfirst.ensure((n + 1) * 4));
    PG_HIP_TRY(h, h->d_pread.ensure(n_pieces * 4, n_pieces * 4 + n_pieces));
    PG_HIP_TRY(h, h->d_psize.ensure(n_pieces * 4, n_pieces * 4 + n_pieces));
    PG_HIP_TRY(h, h->d_pdata.ensure(n_pieces * 8, n_pieces * 8 + 2 * n_pieces));
    PG_HIP_TRY(h, h->h_psize.ensure(n_pieces * 4, n_pieces * 4 + n_pieces));
    PG_HIP_TRY(h, hipMemcpyAsync(h->d_soff.p, sig_off, (n + 1) * 8, hipMemcpyHostToDevice, s));
    PG_HIP_TRY(h, hipMemcpyAsync(h->d_pfirst.p, h->piece_first.data(), (n + 1) * 4, hipMemcpyHostToDevice, s));
    PG_HIP_TRY(h, hipMemcpyAsync(h->d_pread.p, h->piece_read.data(), n_pieces * 4, hipMemcpyHostToDevice, s));
    const EncBatch B{sig_dev, h->d_soff.p, h->d_pread.p, h->d_pfirst.p};
    const dim3 grid((uint32_t)n_pieces), block(kWave);

    PG_HIP_TRY(h, hipEventRecord(h->ev[0], s));
    hipLaunchKernelGGL(k_enc<false>, grid, block, 0, s, B, h->d_psize.p, (const uint64_t *)nullptr, (const uint64_t *)nullptr, (uint8_t *)nullptr);
    PG_HIP_TRY(h, hipGetLastError());
    PG_HIP_TRY(h, hipEventRecord(h->ev[1], s));
    PG_HIP_TRY(h, hipMemcpyAsync(h->h_psize.p, h->d_psize.p, n_pieces * 4, hipMemcpyDeviceToHost, s));
    PG_HIP_TRY(h, hipStreamSynchronize(s));

    // ---- the scan: every read's block, every piece's first data byte
    h->pdata.resize(n_pieces);
    uint64_t at_byte = 0;
    for (uint64_t r = 0; r < n; r++) {
        h->block_off[r] = at_byte;
        at_byte += 4 + pg_svb_nctrl((uint32_t)(sig_off[r + 1] - sig_off[r]));
        for (uint32_t p = h->piece_first[r]; p < h->piece_first[r + 1]; p++) { h->pdata[p] = at_byte; at_byte += h->h_psize.p[p]; }
    }
    h->block_off[n] = at_byte;
    PG_HIP_TRY(h, h->d_blocks.ensure(at_byte, at_byte + at_byte / 4));
    PG_HIP_TRY(h, hipMemcpyAsync(h->d_boff.p, h->block_off.data(), (n + 1) * 8, hipMemcpyHostToDevice, s));
    PG_HIP_TRY(h, hipMemcpyAsync(h->d_pdata.p, h->pdata.data(), n_pieces * 8, hipMemcpyHostToDevice, s));
    PG_HIP_TRY(h, hipEventRecord(h->ev[2], s));
    hipLaunchKernelGGL(k_enc<true>, grid, block, 0, s, B, (uint32_t *)nullptr, h->d_boff.p, h->d_pdata.p, h->d_blocks.p);
    PG_HIP_TRY(h, hipGetLastError());
    PG_HIP_TRY(h, hipEventRecord(h->ev[3], s));
    PG_HIP_TRY(h, hipStreamSynchronize(s));
    float ms = 0;
    PG_HIP_TRY(h, hipEventElapsedTime(&ms, h->ev[0], h->ev[1])); h->lens_ms += ms;
    PG_HIP_TRY(h, hipEventElapsedTime(&ms, h->ev[2], h->ev[3])); h->emit_ms += ms;
    out->n_block_bytes = at_byte; out->blocks = h->d_blocks.p;
    return PG_OK;
}

} // extern "C"
